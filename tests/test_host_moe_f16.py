"""Unquantised (fp16 / bf16) mixture-of-experts checkpoints on the host side: read_config accepts Qwen3-MoE, Qwen2-MoE and Mixtral
checkpoints without a quantization_config (weight_format 'f16'), the reader returns every expert as fp16 [K][N] -- w13 with gate and
up interleaved column by column, w2 as [inter][hidden], bf16 converted as the dense reader converts it --, export_weights emits
`.weight` slots only and halves `inter` consistently at tp = 2, and a quantised shared-expert gate stays refused.
Tiny checkpoints in tmp_path: H 256, expert width 128 (256 for the tp = 2 case), 4 experts, 1 layer."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint, loader
from lmdeploy_amd.turbomind.engine import make_model_config
from tests.qwen2_moe_reference import hf_qwen2_moe_tensors, qwen2_moe_config_json
from tests.qwen_moe_reference import hf_qwen_moe_tensors, qwen_moe_config_json

torch = pytest.importorskip('torch')
safetensors_torch = pytest.importorskip('safetensors.torch', reason='safetensors is not importable on this machine')

f16 = np.float16
H, HQ, HKV, E, K, V, S = 256, 4, 2, 4, 2, 96, 128
PROJ = {'qwen3': ('mlp', ('gate_proj', 'up_proj', 'down_proj')), 'qwen2': ('mlp', ('gate_proj', 'up_proj', 'down_proj')),
        'mixtral': ('block_sparse_moe', ('w1', 'w3', 'w2'))}


def _hf(family, rng, I):
    """HF-layout fp16 tensors ([out, in]) and the config.json of a 1-layer checkpoint without a quantization_config"""
    if family == 'qwen2':
        return hf_qwen2_moe_tensors(rng, H, HQ, HKV, I, S, E, V, 1), qwen2_moe_config_json(H, HQ, HKV, I, S, E, K, V, 1, 'hf')
    t = hf_qwen_moe_tensors(rng, H, HQ, HKV, I, E, V, 1)
    if family == 'qwen3':
        return t, qwen_moe_config_json(H, HQ, HKV, I, E, K, V, 1, 'hf')
    # Mixtral (models/mixtral.py:73-106): the same tensors under block_sparse_moe.gate / .experts.X.{w1, w3, w2}; no q / k norm
    ren = {'gate_proj': 'w1', 'up_proj': 'w3', 'down_proj': 'w2'}
    out = {}
    for name, v in t.items():
        if '_norm.weight' in name and 'self_attn' in name:
            continue
        if '.mlp.' in name:
            name = name.replace('.mlp.', '.block_sparse_moe.')
            for a, b in ren.items():
                name = name.replace(a, b)
        out[name] = v
    cfg = {'architectures': ['MixtralForCausalLM'], 'hidden_size': H, 'num_hidden_layers': 1, 'num_attention_heads': HQ,
           'num_key_value_heads': HKV, 'intermediate_size': I, 'num_local_experts': E, 'num_experts_per_tok': K, 'vocab_size': V,
           'rms_norm_eps': 1e-5, 'rope_theta': 1000000.0, 'max_position_embeddings': 32768, 'head_dim': 128}
    return out, cfg


def _write(path, tensors, cfg, dtype):
    """model.safetensors in `dtype` (the fp16 values are exact in bf16 only after rounding: the file holds what torch rounds them
    to) + config.json; returns the tensors as stored, as torch tensors"""
    stored = {k: torch.from_numpy(v).to(dtype) for k, v in tensors.items()}
    safetensors_torch.save_file(stored, os.path.join(path, 'model.safetensors'))
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(dict(cfg, torch_dtype='bfloat16' if dtype == torch.bfloat16 else 'float16'), f)
    return stored


def _as_dense_reader(t):
    """what checkpoint._linear(..., quantized=False) makes of a stored [out, in] tensor: bf16 -> fp32 (exact) -> fp16, transposed"""
    return np.ascontiguousarray(t.float().numpy().astype(f16).T)


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
@pytest.mark.parametrize('family', ['qwen3', 'qwen2', 'mixtral'])
def test_read_unquantised_moe_checkpoint(tmp_path, family, dtype):
    I = 128
    rng = np.random.default_rng(3)
    hf, cfg = _hf(family, rng, I)
    stored = _write(str(tmp_path), hf, cfg, getattr(torch, dtype))
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.weight_format, mc.quantized, mc.moe_experts, mc.moe_top_k, mc.inter, mc.hidden) == ('f16', False, E, K, I, H)
    assert mc.arch == {'qwen3': 'qwen3', 'qwen2': 'qwen2', 'mixtral': 'llama'}[family]
    assert mc.moe_shared_inter == (S if family == 'qwen2' else 0)
    assert make_model_config(mc, 1).moe_experts == E
    w = checkpoint.load_hf_weights(str(tmp_path), mc)
    m, (gn, un, dn) = PROJ[family]
    L = w['layers'][0]
    p = f'model.layers.0.{m}'
    assert L['moe_gate'].dtype == f16 and np.array_equal(L['moe_gate'], _as_dense_reader(stored[p + '.gate.weight']))
    assert len(L['experts']) == E
    for x in range(E):
        w13, w2 = L['experts'][x]['w1w3'], L['experts'][x]['w2']
        assert set(w13) == {'w'} and set(w2) == {'w'}
        assert w13['w'].dtype == f16 and w13['w'].shape == (H, 2 * I) and w2['w'].dtype == f16 and w2['w'].shape == (I, H)
        g, u, d = (_as_dense_reader(stored[f'{p}.experts.{x}.{n}.weight']) for n in (gn, un, dn))
        assert np.array_equal(w13['w'][:, 0::2], g) and np.array_equal(w13['w'][:, 1::2], u), f'expert {x}: gate / up interleave'
        assert np.array_equal(w2['w'], d), f'expert {x}: w2'
        if dtype == 'float16':     # nothing is rounded on the way
            assert np.array_equal(w13['w'][:, 0::2], hf[f'{p}.experts.{x}.{gn}.weight'].T)
    # the dense linears of the same checkpoint go through the same conversion
    assert np.array_equal(L['wo']['w'], _as_dense_reader(stored['model.layers.0.self_attn.o_proj.weight']))
    if family == 'qwen2':          # the shared expert: a dense fp16 FFN of width S, its gate [1, H] -> [H]
        assert L['w1w3']['w'].shape == (H, 2 * S) and L['w2']['w'].shape == (S, H)
        assert np.array_equal(L['w1w3']['w'][:, 1::2], _as_dense_reader(stored[p + '.shared_expert.up_proj.weight']))
        assert np.array_equal(L['shared_gate'], stored[p + '.shared_expert_gate.weight'].float().numpy().astype(f16)[0])
    slots = loader.export_weights(mc, w, 1, 0)
    for x in range(E):
        q = f'layers.0.moe_ffn.experts.{x}'
        assert slots[q + '.w1w3.weight'].dtype == f16 and slots[q + '.w1w3.weight'].shape == (H, 2 * I)
        assert slots[q + '.w2.weight'].shape == (I, H)
        assert np.array_equal(slots[q + '.w1w3.weight'], L['experts'][x]['w1w3']['w'])
    assert sum(1 for s in slots if '.moe_ffn.experts.' in s) == 2 * E      # no scales / zeros slots
    assert not any(s.endswith(('.qweight', '.scales', '.zeros')) for s in slots)


@pytest.mark.parametrize('family', ['qwen3', 'mixtral'])
def test_unquantised_experts_shard_over_tp2(tmp_path, family):
    """expert width 256 at tp = 2: rank r owns the inter columns [128 r, 128 (r + 1)) of gate AND up (pairs stay together) and the
    same rows of w2; width 128 (64 per rank) is refused"""
    I = 256
    rng = np.random.default_rng(5)
    hf, cfg = _hf(family, rng, I)
    _write(str(tmp_path), hf, cfg, torch.float16)
    mc = checkpoint.read_config(str(tmp_path))
    w = checkpoint.load_hf_weights(str(tmp_path), mc)
    m, (gn, un, dn) = PROJ[family]
    half = I // 2
    for r in range(2):
        slots = loader.export_weights(mc, w, 2, r)
        for x in (0, E - 1):
            p, q = f'model.layers.0.{m}.experts.{x}', f'layers.0.moe_ffn.experts.{x}'
            g, u, d = (hf[f'{p}.{n}.weight'].T for n in (gn, un, dn))
            w13, w2 = slots[q + '.w1w3.weight'], slots[q + '.w2.weight']
            assert w13.shape == (H, 2 * half) and w2.shape == (half, H)
            assert np.array_equal(w13[:, 0::2], g[:, r * half:(r + 1) * half]) and np.array_equal(w13[:, 1::2], u[:, r * half:(r + 1) * half])
            assert np.array_equal(w2, d[r * half:(r + 1) * half])
    mc.inter = 128
    w128 = dict(w, layers=[dict(w['layers'][0], experts=[dict(w1w3=dict(w=e_['w1w3']['w'][:, :256]), w2=dict(w=e_['w2']['w'][:128]))
                                                        for e_ in w['layers'][0]['experts']])])
    with pytest.raises(ValueError, match='multiple of 128'):
        loader.export_weights(mc, w128, 2, 0)


def test_quantised_shared_gate_still_refused(tmp_path):
    """an otherwise unquantised Qwen2-MoE checkpoint whose shared_expert_gate carries AWQ tensors"""
    rng = np.random.default_rng(6)
    hf, cfg = _hf('qwen2', rng, 128)
    sg = 'model.layers.0.mlp.shared_expert_gate'
    tensors = {k: torch.from_numpy(v) for k, v in hf.items() if k != sg + '.weight'}
    tensors[sg + '.qweight'] = torch.zeros((H, 1), dtype=torch.int32)
    safetensors_torch.save_file(tensors, os.path.join(str(tmp_path), 'model.safetensors'))
    with open(os.path.join(str(tmp_path), 'config.json'), 'w') as f:
        json.dump(dict(cfg, torch_dtype='float16'), f)
    mc = checkpoint.read_config(str(tmp_path))
    with pytest.raises(NotImplementedError, match='shared_expert_gate'):
        checkpoint.load_hf_weights(str(tmp_path), mc)


@pytest.mark.parametrize('cfg', [qwen_moe_config_json(2048, 32, 4, 768, 128, 8, 151936, 48, 'hf'),
                                 qwen2_moe_config_json(2048, 16, 16, 1408, 5632, 60, 4, 151936, 24, 'hf')],
                         ids=['Qwen3-30B-A3B', 'Qwen1.5-MoE-A2.7B'])
def test_read_config_published_bf16(tmp_path, cfg):
    """the config.json of the checkpoints as published (no quantization_config): accepted as 'f16'"""
    with open(os.path.join(str(tmp_path), 'config.json'), 'w') as f:
        json.dump(dict(cfg, torch_dtype='bfloat16'), f)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.weight_format, mc.quantized, mc.moe_experts) == ('f16', False, cfg['num_experts'])
    assert make_model_config(mc, 1).weight_type == 1


def test_grouped_tile_table_answers_for_f16():
    """`G 33 ...` lines (kind 32 + TM_WEIGHT_F16) carry the measured row tile of the fp16 experts: 16 / 32 / 64 rows at decode-sized
    forwards; other heights and prefill-sized keys are ignored; tm_debug_grouped_tile reads them back"""
    lib = _ffi.load()

    def tile(K, N, tokens):
        r = _ffi.C.c_int(-1)
        _ffi.check(lib.tm_debug_grouped_tile(1, K, N, tokens, _ffi.C.byref(r)))
        return r.value
    import tempfile
    assert tile(2304, 1792, 64) == 0
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, 't.txt')
        with open(f, 'w') as fh:
            fh.write('G 33 0 2304 1792 64 32 0 0 0\n'
                     'G 33 0 2304 1792 8 16 0 0 0\n'
                     'G 33 0 2304 1792 16 48 0 0 0\n'        # invalid: no 48-row tile
                     'G 33 0 2304 1792 128 64 0 0 0\n')      # invalid: the row tile is a decode-batch choice
        assert lib.tm_gemm_import(f.encode()) == 0
    assert (tile(2304, 1792, 64), tile(2304, 1792, 8), tile(2304, 1792, 16), tile(2304, 1792, 128)) == (32, 16, 0, 0)
    assert tile(2304, 1792, 32) == 0


@pytest.mark.parametrize('dtype', [None, 'float32'])
@pytest.mark.parametrize('cfg', [qwen_moe_config_json(2048, 32, 4, 768, 128, 8, 151936, 48, 'hf'),
                                 qwen2_moe_config_json(2048, 16, 16, 1408, 5632, 60, 4, 151936, 24, 'hf')], ids=['qwen3', 'qwen2'])
def test_read_config_needs_a_16_bit_dtype(tmp_path, cfg, dtype):
    """no quantization_config and no fp16 / bf16 torch_dtype (float32 experts, or a quantised export that lost its
    quantization_config): refused with the reason; `dtype`, the key newer exports write, is read like `torch_dtype`"""
    c = dict(cfg) if dtype is None else dict(cfg, torch_dtype=dtype)
    with open(os.path.join(str(tmp_path), 'config.json'), 'w') as f:
        json.dump(c, f)
    with pytest.raises(NotImplementedError, match='unquantised experts'):
        checkpoint.read_config(str(tmp_path))
    with open(os.path.join(str(tmp_path), 'config.json'), 'w') as f:
        json.dump(dict(cfg, dtype='bfloat16'), f)
    assert checkpoint.read_config(str(tmp_path)).weight_format == 'f16'
