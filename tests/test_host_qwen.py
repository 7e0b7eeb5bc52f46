"""Qwen2 / Qwen3 dense decoders on the host side: config reading and refusals, HF weight reading (AWQ and fp16), the
q / k / v bias and q / k norm permutations, tensor-parallel sharding of the bias, and the C-ABI model config."""
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
from tests.qwen_reference import QwenConfig, hf_qwen_tensors, tm_weights_from_hf, write_qwen_checkpoint

f16 = np.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_cfg(path, **c):
    base = {'hidden_size': 512, 'num_hidden_layers': 2, 'num_attention_heads': 4, 'num_key_value_heads': 2,
            'intermediate_size': 1024, 'vocab_size': 256, 'rms_norm_eps': 1e-6, 'rope_theta': 1000000.0}
    base.update(c)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(base, f)


def test_read_config_qwen2(tmp_path):
    _write_cfg(tmp_path, architectures=['Qwen2ForCausalLM'], hidden_size=3584, num_attention_heads=28, num_key_value_heads=4,
               tie_word_embeddings=False, use_sliding_window=False, eos_token_id=151643, max_position_embeddings=32768)
    with open(os.path.join(tmp_path, 'generation_config.json'), 'w') as f:
        json.dump({'eos_token_id': [151645, 151643]}, f)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.arch, mc.attn_bias, mc.qk_norm, mc.head_dim, mc.q_heads, mc.kv_heads) == ('qwen2', 1, 0, 128, 28, 4)
    assert (mc.rope.base, mc.rope.type, mc.rms_eps, mc.tie_word_embeddings) == (1e6, 'default', 1e-6, False)
    assert mc.eos_token_id == [151643, 151645]
    mcfg = make_model_config(mc)
    assert (mcfg.attn_bias, mcfg.qk_norm) == (1, 0)


@pytest.mark.parametrize('attention_bias', [False, True])
def test_read_config_qwen3(tmp_path, attention_bias):
    _write_cfg(tmp_path, architectures=['Qwen3ForCausalLM'], hidden_size=2560, num_attention_heads=32, num_key_value_heads=8,
               head_dim=128, attention_bias=attention_bias, tie_word_embeddings=True, eos_token_id=151645)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.arch, mc.attn_bias, mc.qk_norm, mc.head_dim, mc.tie_word_embeddings) == ('qwen3', int(attention_bias), 1, 128, True)
    assert mc.eos_token_id == 151645 and mc.rope.base == 1e6
    mcfg = make_model_config(mc)
    assert (mcfg.attn_bias, mcfg.qk_norm) == (int(attention_bias), 1)


@pytest.mark.parametrize('arch,extra', [
    ('Qwen2MoeForCausalLM', {}),
    ('Qwen3MoeForCausalLM', {'head_dim': 128}),
    ('Qwen2ForCausalLM', {'use_sliding_window': True}),
    ('Qwen2ForCausalLM', {'rope_scaling': {'type': 'yarn', 'factor': 4.0, 'original_max_position_embeddings': 32768}}),
    ('Qwen3ForCausalLM', {'head_dim': 128, 'rope_scaling': {'rope_type': 'dynamic', 'factor': 2.0}}),
    ('Qwen2ForCausalLM', {'hidden_size': 896, 'num_attention_heads': 14}),     # Qwen2.5-0.5B: head_dim 64
])
def test_read_config_qwen_refusals(tmp_path, arch, extra):
    _write_cfg(tmp_path, architectures=[arch], **extra)
    with pytest.raises(NotImplementedError):
        checkpoint.read_config(str(tmp_path))


def test_model_config_defaults_keep_todays_path():
    """configs without the new fields (the oracle's) hand the engine attn_bias = qk_norm = 0"""
    cfg = o.ModelConfig(hidden=256, layers=1, q_heads=4, kv_heads=2, head_dim=128, inter=256, vocab=64)
    mcfg = make_model_config(cfg)
    assert (mcfg.attn_bias, mcfg.qk_norm) == (0, 0)
    q = make_model_config(QwenConfig(hidden=256, layers=1, q_heads=4, kv_heads=2, head_dim=128, inter=256, vocab=64, attn_bias=1,
                                     qk_norm=1))
    assert (q.attn_bias, q.qk_norm) == (1, 1)


def test_ffi_model_config_matches_header():
    """_ffi.ModelConfig mirrors struct tm_model_config field for field (every field is 4 bytes wide)"""
    hdr = open(os.path.join(ROOT, 'include', 'tm_mi355x.h')).read()
    body = re.search(r'typedef struct tm_model_config \{(.*?)\} tm_model_config;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n.strip() for decl in body.split(';') if decl.strip() for n in decl.split(None, 1)[1].split(',')]
    assert [f[0] for f in _ffi.ModelConfig._fields_] == names
    assert ctypes.sizeof(_ffi.ModelConfig) == 4 * len(names)
    assert names[-2:] == ['attn_bias', 'qk_norm']


def test_load_hf_awq_qwen2(tmp_path):
    """AWQ Qwen2: projections quantised, biases fp16; the q / k bias is permuted like the q / k columns"""
    rng = np.random.default_rng(0)
    H, Hq, Hkv, I, V = 256, 4, 2, 256, 96
    hf = hf_qwen_tensors(rng, 'qwen2', H, Hq, Hkv, I, V)
    quant = write_qwen_checkpoint(str(tmp_path), 'qwen2', hf, H, Hq, Hkv, I, V, awq=True)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.quantized, mc.weight_format, mc.attn_bias, mc.qk_norm) == (True, 'u4', 1, 0)
    w = checkpoint.load_hf_weights(str(tmp_path), mc)
    L = w['layers'][0]
    a = 'model.layers.0.self_attn.'
    exp_b = np.concatenate([o.permute_qk_for_interleaved_rope(hf[a + 'q_proj.bias'], Hq, 128),
                            o.permute_qk_for_interleaved_rope(hf[a + 'k_proj.bias'], Hkv, 128), hf[a + 'v_proj.bias']])
    assert L['qkv_bias'].dtype == f16 and np.array_equal(L['qkv_bias'], exp_b)
    assert not np.array_equal(L['qkv_bias'][:Hq * 128], hf[a + 'q_proj.bias'])       # the permutation is not the identity
    ref = tm_weights_from_hf(hf, QwenConfig(hidden=H, layers=1, q_heads=Hq, kv_heads=Hkv, head_dim=128, inter=I, vocab=V,
                                            attn_bias=1), quant)
    assert np.array_equal(L['w_qkv']['q'], ref['layers'][0]['w_qkv']['q'])
    assert 'q_norm' not in L
    assert np.array_equal(w['output'], hf['lm_head.weight'].T)
    slots = loader.export_weights(mc, w)
    assert slots['layers.0.attention.w_qkv.bias'].shape == ((Hq + 2 * Hkv) * 128,)
    assert 'layers.0.attention.q_norm.weight' not in slots


def test_load_hf_fp16_qwen3_tied(tmp_path):
    """fp16 Qwen3 with tied embeddings: q_norm / k_norm permuted as one head; the lm_head is the embedding table"""
    rng = np.random.default_rng(1)
    H, Hq, Hkv, I, V = 256, 4, 2, 256, 96
    hf = hf_qwen_tensors(rng, 'qwen3', H, Hq, Hkv, I, V, tie=True)
    write_qwen_checkpoint(str(tmp_path), 'qwen3', hf, H, Hq, Hkv, I, V, tie=True)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.quantized, mc.attn_bias, mc.qk_norm, mc.tie_word_embeddings) == (False, 0, 1, True)
    w = checkpoint.load_hf_weights(str(tmp_path), mc)
    L = w['layers'][0]
    a = 'model.layers.0.self_attn.'
    for n in ('q_norm', 'k_norm'):
        assert np.array_equal(L[n], o.permute_qk_for_interleaved_rope(hf[a + n + '.weight'], 1, 128))
        assert np.array_equal(L[n][0::2], hf[a + n + '.weight'][:64]) and np.array_equal(L[n][1::2], hf[a + n + '.weight'][64:])
    assert 'qkv_bias' not in L
    assert np.array_equal(w['output'], hf['model.embed_tokens.weight'].T)
    ref = tm_weights_from_hf(hf, QwenConfig(hidden=H, layers=1, q_heads=Hq, kv_heads=Hkv, head_dim=128, inter=I, vocab=V, qk_norm=1))
    assert np.array_equal(L['w_qkv']['w'], ref['layers'][0]['w_qkv']['w'])
    for tp in (1, 2):
        for r in range(tp):
            slots = loader.export_weights(mc, w, tp, r)
            assert np.array_equal(slots['layers.0.attention.q_norm.weight'], L['q_norm'])      # replicated
            assert np.array_equal(slots['layers.0.attention.k_norm.weight'], L['k_norm'])
            assert 'layers.0.attention.w_qkv.bias' not in slots


@pytest.mark.parametrize('Hq,Hkv,tp', [(4, 2, 2), (8, 2, 4), (8, 4, 2), (28, 4, 4), (8, 1, 2)])
def test_export_bias_shards_reassemble(Hq, Hkv, tp):
    """every rank's bias = its Q | K | V column slices of w_qkv (kv heads replicated when Hkv < tp); the ranks' q parts concatenate to
    the whole q bias, and each rank's k / v part is the bias of the kv head its q heads read"""
    D = 128
    cfg = QwenConfig(hidden=256, layers=1, q_heads=Hq, kv_heads=Hkv, head_dim=D, inter=512, vocab=64, attn_bias=1)
    rng = np.random.default_rng(Hq * 10 + tp)
    n = (Hq + 2 * Hkv) * D
    bias = rng.standard_normal(n).astype(f16)
    w = o.make_synthetic_weights(cfg, seed=0, quantized=False)
    w['layers'][0]['qkv_bias'] = bias
    qs, hq_l = [], Hq // tp
    for r in range(tp):
        sl = loader.export_weights(cfg, w, tp, r)
        b = sl['layers.0.attention.w_qkv.bias']
        wq = sl['layers.0.attention.w_qkv.weight']
        hkv_l = max(1, Hkv // tp)
        assert b.shape == (wq.shape[1],) == ((hq_l + 2 * hkv_l) * D,)
        qs.append(b[:hq_l * D])
        kv0 = r * hkv_l if Hkv >= tp else r // (tp // Hkv)
        assert np.array_equal(b[hq_l * D:(hq_l + hkv_l) * D], bias[(Hq + kv0) * D:(Hq + kv0 + hkv_l) * D])
        assert np.array_equal(b[(hq_l + hkv_l) * D:], bias[(Hq + Hkv + kv0) * D:(Hq + Hkv + kv0 + hkv_l) * D])
        # the rank's q heads belong to its kv head(s)
        assert (r * hq_l) // (Hq // Hkv) >= kv0 and (r * hq_l + hq_l - 1) // (Hq // Hkv) < kv0 + hkv_l
    assert np.array_equal(np.concatenate(qs), bias[:Hq * D])
