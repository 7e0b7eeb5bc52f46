"""CPU tests of the sliding-window / attention-sink plumbing: the checkpoint reader's `sliding_window`, the loader's sharding of the
sink logits, the struct and symbol declarations, and the reference arithmetic the GPU tests compare against."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint, loader
from lmdeploy_amd.turbomind.engine import make_model_config
from oracle import tm_oracle as o
from tests.attention_window_reference import WindowConfig, make_window_weights, sink_attention, window_decode, window_prefill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f16 = np.float16


def _config(tmp_path, arch, **extra):
    c = {'architectures': [arch], 'hidden_size': 256, 'num_hidden_layers': 2, 'num_attention_heads': 2, 'num_key_value_heads': 2,
         'intermediate_size': 512, 'vocab_size': 640, 'rms_norm_eps': 1e-5, 'rope_theta': 10000.0, 'max_position_embeddings': 32768,
         'head_dim': 128}
    c.update(extra)
    with open(os.path.join(tmp_path, 'config.json'), 'w') as f:
        json.dump(c, f)
    return checkpoint.read_config(str(tmp_path))


def test_read_config_mistral_sliding_window(tmp_path):
    assert _config(tmp_path, 'MistralForCausalLM', sliding_window=4096).window == 4096        # Mistral-7B-v0.1
    assert _config(tmp_path, 'MistralForCausalLM', sliding_window=None).window == 0           # v0.2 and later: null
    assert _config(tmp_path, 'MistralForCausalLM').window == 0
    assert _config(tmp_path, 'MistralForCausalLM', sliding_window=0).window == 0
    with pytest.raises(ValueError, match='sliding_window'):
        _config(tmp_path, 'MistralForCausalLM', sliding_window=-1)
    with pytest.raises(ValueError, match='sliding_window'):
        _config(tmp_path, 'MistralForCausalLM', sliding_window='4096')


def test_read_config_other_architectures(tmp_path):
    mx = _config(tmp_path, 'MixtralForCausalLM', sliding_window=None, num_local_experts=4, num_experts_per_tok=2)
    assert mx.window == 0 and mx.moe_experts == 4
    assert _config(tmp_path, 'MixtralForCausalLM', sliding_window=1024, num_local_experts=4, num_experts_per_tok=2).window == 1024
    assert _config(tmp_path, 'LlamaForCausalLM', sliding_window=4096).window == 0             # a stray key on a Llama is ignored
    assert checkpoint.ModelConfig(hidden=256, layers=1, q_heads=2, kv_heads=2, head_dim=128, inter=512, vocab=64).window == 0
    with pytest.raises(NotImplementedError, match='use_sliding_window'):                      # the Qwen refusal is unchanged
        _config(tmp_path, 'Qwen2ForCausalLM', use_sliding_window=True, sliding_window=4096)
    assert _config(tmp_path, 'Qwen2ForCausalLM', use_sliding_window=False, sliding_window=32768).window == 0


def test_model_config_carries_window_and_sinks(tmp_path):
    mc = make_model_config(_config(tmp_path, 'MistralForCausalLM', sliding_window=4096), 1)
    assert (mc.attn_window, mc.attn_sinks, mc.attn_bias, mc.qk_norm) == (4096, 0, 0, 0)
    cfg = WindowConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=64, inter=512, vocab=64, attn_sinks=1, layer_windows=(48, 0))
    mc = make_model_config(cfg)
    assert (mc.attn_window, mc.attn_sinks) == (0, 1)
    plain = make_model_config(o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=64, inter=512, vocab=64))
    assert (plain.attn_window, plain.attn_sinks) == (0, 0)


@pytest.mark.parametrize('tp', [1, 2, 4])
def test_loader_shards_sinks_like_the_q_heads(tp):
    cfg = WindowConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=64, attn_sinks=1)
    w = make_window_weights(cfg, seed=2)
    assert all(L['sinks'].shape == (4,) and L['sinks'].dtype == f16 for L in w['layers'])
    assert all((L['sinks'] >= -2).all() and (L['sinks'] <= 4).all() for L in w['layers'])
    shards = [loader.export_weights(cfg, w, tp, r) for r in range(tp)]
    for i, L in enumerate(w['layers']):
        parts = [s[f'layers.{i}.attention.sinks'] for s in shards]
        assert all(p.shape == (4 // tp,) and p.dtype == f16 and p.flags['C_CONTIGUOUS'] for p in parts)
        assert np.array_equal(np.concatenate(parts), L['sinks'])
    plain = loader.export_weights(cfg, o.make_synthetic_weights(cfg, seed=2), 1, 0)
    assert not any('sinks' in k for k in plain)


def test_ffi_structs_and_symbols_match_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'tm_mi355x.h')).read()
    body = re.search(r'typedef struct tm_model_config \{(.*?)\} tm_model_config;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n.strip() for decl in body.split(';') if decl.strip() for n in decl.split(None, 1)[1].split(',')]
    fields = [f[0] for f in _ffi.ModelConfig._fields_]
    assert fields == names and ctypes.sizeof(_ffi.ModelConfig) == 4 * len(names)
    i = names.index('attn_window')
    assert names[i:i + 2] == ['attn_window', 'attn_sinks'] and names[i - 1] == 'moe_shared_inter'
    assert dict(_ffi.ModelConfig._fields_)['attn_window'] is ctypes.c_int and dict(_ffi.ModelConfig._fields_)['attn_sinks'] is ctypes.c_int
    declared = set(re.findall(r'\b(tm_[a-z0-9_]+)\s*\(', hdr)) - {'tm_status'}
    new = {'tm_decode_attention_window', 'tm_prefill_attention_window', 'tm_engine_set_layer_windows'}
    assert new <= declared and new <= set(_ffi.EXPORTED_SYMBOLS) and declared == set(_ffi.EXPORTED_SYMBOLS)
    lib = _ffi.load()
    for name in new:
        assert hasattr(lib, name)
    # the windowed calls are the old signatures plus (window, sinks) in front of the stream
    sig = _ffi._SIGNATURES
    assert sig['tm_decode_attention_window'][1] == sig['tm_decode_attention'][1][:-1] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert sig['tm_prefill_attention_window'][1] == sig['tm_prefill_attention_hd'][1][:-1] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # each new entry point cites the reference lines it stands for
    for name in ('tm_decode_attention_window', 'tm_prefill_attention_window'):
        comment = hdr[:hdr.index('int ' + name)].rsplit('/*', 1)[1]
        assert 'attention_params.h:55-72' in comment and 'attention_universal.h' in comment, name


def test_negative_windows_are_status_codes():
    lib = _ffi.load()
    one = ctypes.c_int(1)
    p = ctypes.addressof(one)
    kc = _ffi.KvCache(p, p, 0, 2, 64, 64, 8)
    assert lib.tm_decode_attention_window(p, p, 128, p, 1, 2, 0.0, 1, None, ctypes.byref(kc), -1, None, None) == 1
    assert 'window' in _ffi.last_error()
    assert lib.tm_prefill_attention_window(p, p, 128, p, p, 64, p, p, p, 1, 1, 2, 2, 64, 0.0, -1, None, None) == 1
    assert 'window' in _ffi.last_error()
    mc = make_model_config(WindowConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=64, inter=512, vocab=64, window=-5))
    cfg = _ffi.EngineConfig(mc, 1, 0, 0, 1, 128, 8, 64, 0.5, 0, 64, 0, 0)
    h = ctypes.c_void_p()
    assert lib.tm_engine_create(ctypes.byref(h), ctypes.byref(cfg)) == 1 and 'attn_window' in _ffi.last_error()


def _kv(rng, Hkv, n, D):
    return rng.standard_normal((Hkv, n, D)).astype(f16), rng.standard_normal((Hkv, n, D)).astype(f16)


def test_window_reference_is_the_oracle_on_the_cropped_context():
    rng = np.random.default_rng(0)
    Hq, Hkv, D, n = 4, 2, 64, 150
    K, V = _kv(rng, Hkv, n, D)
    q = rng.standard_normal((Hq, D)).astype(f16)
    full = o.decode_attention(q, K, V, None, 1)
    for W in (0, n, n + 1, 4096):
        assert np.array_equal(window_decode(q, K, V, W).view(np.uint16), full.view(np.uint16)), W
    assert np.array_equal(window_decode(q, K, V, 33).view(np.uint16), o.decode_attention(q, K[:, -33:], V[:, -33:], None, 1).view(np.uint16))
    assert not np.array_equal(window_decode(q, K, V, 33), full)
    # W = 1: the query sees its own token alone -> the output is that token's V
    assert np.array_equal(window_decode(q, K, V, 1), np.repeat(V[:, -1], Hq // Hkv, 0))
    # against the unfused float64 restatement with an explicit mask 0 <= q_pos - k_pos < W
    s = np.einsum('hd,hnd->hn', q.astype(np.float64), np.repeat(K, Hq // Hkv, 0).astype(np.float64)) / np.sqrt(D)
    s[:, :n - 33] = -np.inf
    p = np.exp(s - s.max(-1, keepdims=True))
    ref = np.einsum('hn,hnd->hd', p / p.sum(-1, keepdims=True), np.repeat(V, Hq // Hkv, 0).astype(np.float64))
    assert np.abs(window_decode(q, K, V, 33).astype(np.float64) - ref).max() <= 2e-3
    # prefill: row i at position hist + i is the decode of that position
    qs = rng.standard_normal((5, Hq, D)).astype(f16)
    out = window_prefill(qs, K, V, n - 5, 16)
    assert np.array_equal(out[2], window_decode(qs[2], K[:, :n - 2], V[:, :n - 2], 16))
    assert np.array_equal(window_prefill(qs, K, V, n - 5, 0), o.prefill_attention(qs, K, V, n - 5, None))


def test_sink_reference():
    rng = np.random.default_rng(1)
    Hq, Hkv, D, n = 4, 2, 64, 70
    K, V = _kv(rng, Hkv, n, D)
    q = rng.standard_normal((Hq, D)).astype(f16)
    none = o.attention_reference_unfused(q, K, V).astype(f16)
    assert np.array_equal(sink_attention(q, K, V, np.full(Hq, -np.inf)), none)                 # a -inf sink is no sink
    assert np.abs(window_decode(q, K, V, 0, None, np.full(Hq, -np.inf, f16)).astype(np.float32)
                  - o.decode_attention(q, K, V, None, 1).astype(np.float32)).max() <= 2e-3     # ... up to the tiled fp16 P rounding
    # a sink scales the output by sum exp(s) / (sum exp(s) + exp(sink)) and leaves its direction alone
    sinks = np.array([-2.0, 0.0, 1.5, 4.0], f16)
    s = np.einsum('hd,hnd->hn', q.astype(np.float64), np.repeat(K, Hq // Hkv, 0).astype(np.float64)) / np.sqrt(D)
    z = np.exp(s).sum(-1)
    want = o.attention_reference_unfused(q, K, V) * (z / (z + np.exp(sinks.astype(np.float64))))[:, None]
    assert np.abs(sink_attention(q, K, V, sinks).astype(np.float64) - want).max() <= 1e-3
    assert np.abs(sink_attention(q, K, V, np.full(Hq, 60.0))).max() <= 1e-3                    # a huge sink takes all the mass
