"""MXFP4 W4A4 dense models on the host: the reference module's own checks and the mutations that must change its answers, a toy
Quark checkpoint through read_config / load_hf_weights / export_weights with every refusal named, config acceptance, and the new
symbols in the header, the ctypes table and INTEGRATION.md."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.loader import export_weights
from tests import mxfp4_dense_reference as r

f16, f32 = np.float16, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference module ------------------------------------------------------------------------------------------------------
def test_e2m1_rounding_known_answers():
    """every representable value comes back; every midpoint goes to the even mantissa; saturation at 6; the sign of zero is kept"""
    vals = r.e2m1_value(np.arange(16))
    assert np.array_equal(vals[:8], [0, 0.5, 1, 1.5, 2, 3, 4, 6]) and np.array_equal(vals[8:], -vals[:8])
    assert np.array_equal(r.e2m1_rne_sat(vals), np.arange(16))
    mid = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    assert np.array_equal(r.e2m1_rne_sat(mid), [0, 2, 2, 4, 4, 6, 6]) and np.array_equal(r.e2m1_rne_sat(-mid), [8, 10, 10, 12, 12, 14, 14])
    assert np.array_equal(r.e2m1_rne_sat(np.nextafter(mid, 10)), [1, 2, 3, 4, 5, 6, 7])
    assert np.array_equal(r.e2m1_rne_sat(np.nextafter(mid, 0)), [0, 1, 2, 3, 4, 5, 6])
    assert np.array_equal(r.e2m1_rne_sat([6.0, 7.9, 1e9, -1e9]), [7, 7, 7, 15])
    assert np.array_equal(r.e2m1_rne_sat([0.0, -0.0]), [0, 8])


def test_quant_known_answers():
    """the scale rule: amax in [4, 8) 2^e shares the byte e + 127; a zero group gets byte 0 and keeps its zeros' signs; the nibble order"""
    x = np.zeros((1, 128), f16)
    x[0, :4] = [6.0, -1.0, 0.26, 7.5]           # amax 7.5 -> e = 0; 7.5 saturates to 6, 0.26 rounds to 0.5
    x[0, 32:35] = [3.99, -2.0, 0.0]             # amax 3.99 -> e = -1: 3.99 / 0.5 = 7.98 -> 6, -2 / 0.5 = -4
    x[0, 64] = 2.0**-24                         # the smallest subnormal: e = -26, code 4.0
    x[0, 97] = -0.0
    b, s = r.quant(x)
    assert s.tolist() == [[127, 126, 101, 0]]
    c = r.unpack_codes(b)[0]
    assert c[:4].tolist() == [7, 10, 1, 7] and c[32:35].tolist() == [7, 14, 0] and c[64] == 6 and c[97] == 8
    assert b[0, 0] == 7 | (10 << 4) and b[0, 1] == 1 | (7 << 4)
    assert np.array_equal(r.dequant(b, s)[0, :4], [6.0, -1.0, 0.5, 6.0])


def test_exact_operands_are_exactly_summable():
    """the shapes tests/test_gpu_mxfp4_dense.py runs, up to its largest M"""
    for K, N, gated in [(128, 96, False), (640, 256, True), (4096, 64, False)]:
        blocks, scales = r.exact_weight(K, N, gated)
        for M in (1, 130):
            r.assert_exactly_summable(r.exact_x(M, K, gated), blocks, scales, gated)
    sx = r.quant(r.exact_x(7, 640))[1].astype(int)
    assert len(np.unique(sx)) == 5 and (sx[1:] != sx[:-1]).all()        # neighbouring rows differ (5 g drops out of a(m, g) mod 5) ...
    sw = r.exact_weight(640, 96)[1].astype(int)
    assert (sw[1:] != sw[:-1]).all() and (sw[:, 1:] != sw[:, :-1]).all()    # ... neighbouring columns and groups through c(n, g)


@pytest.mark.parametrize('mut', r.MUTATIONS)
def test_mutations_change_the_answers(mut):
    """scale rule off by one, ties away from even, nibbles swapped, a scale from the neighbouring group: each moves the exact
    operands' outputs (ties_away: operands with elements on the midpoints, which the exact ones avoid by construction)"""
    K, N = 640, 96
    blocks, scales = r.exact_weight(K, N)
    x = r.exact_x(33, K)
    if mut == 'ties_away':                  # two elements behind every group's pivot sit on the midpoints 1.25 and 2.5 of its scale
        x = x.astype(np.float64).reshape(33, K // 32, 32)
        m, g = np.meshgrid(np.arange(33), np.arange(K // 32), indexing='ij')
        for off, v in ((1, 1.25), (2, 2.5)):
            x[m, g, ((5 * m + 3 * g) % 32 + off) % 32] = v * np.exp2(r.row_exp(33, K // 32))
        x = x.reshape(33, K).astype(f16)
    want = r.linear(x, blocks, scales).astype(f32)
    got = r.linear(x, blocks, scales, mut=mut).astype(f32)
    assert np.isfinite(got).all() and (got != want).mean() > 0.2, mut


# ---- reader and loader -----------------------------------------------------------------------------------------------------------
def _load(path):
    cfg = checkpoint.read_config(path)
    w = checkpoint.load_hf_weights(path, cfg)
    return cfg, w, export_weights(cfg, w)


@pytest.mark.parametrize('geo', [{}, dict(head_dim=64, q_heads=4, kv_heads=2)], ids=['d128', 'd64'])
def test_reader_and_loader(tmp_path, geo):
    """the toy Quark checkpoint: weight_format mxfp4, the weights the reference module assembles from the same tensors (q / k rows
    permuted, q | k | v stacked, gate / up rows interleaved), uint8 blocks / scales slots, KV scales read past, lm_head fp16"""
    ck = r.write_checkpoint(str(tmp_path), seed=3, **geo)
    assert 'model.layers.0.self_attn.k_proj.output_scale' in ck
    cfg, w, slots = _load(str(tmp_path))
    assert cfg.weight_format == 'mxfp4' and cfg.quantized and cfg.head_dim == geo.get('head_dim', 128) and cfg.moe_experts == 0
    ref = r.tm_weights(ck, r.oracle_config(ck, 16))
    for i, (a, b) in enumerate(zip(w['layers'], ref['layers'])):
        for k in ('w_qkv', 'wo', 'w1w3', 'w2'):
            assert set(a[k]) == {'blocks', 'scales'}
            assert np.array_equal(a[k]['blocks'], b[k]['blocks']) and np.array_equal(a[k]['scales'], b[k]['scales']), (i, k)
    nq = (cfg.q_heads + 2 * cfg.kv_heads) * cfg.head_dim
    for name, shape in (('attention.w_qkv', (nq, 256)), ('attention.wo', (256, cfg.q_heads * cfg.head_dim)), ('feed_forward.w1w3', (1024, 256)),
                        ('feed_forward.w2', (256, 512))):
        b, s = slots[f'layers.1.{name}.blocks'], slots[f'layers.1.{name}.scales']
        assert b.dtype == np.uint8 and b.shape == (shape[0], shape[1] // 2) and s.dtype == np.uint8 and s.shape == (shape[0], shape[1] // 32)
    g, u = ck['model.layers.1.mlp.gate_proj.weight'], ck['model.layers.1.mlp.up_proj.weight_scale']
    assert np.array_equal(slots['layers.1.feed_forward.w1w3.blocks'][0::2], g) and np.array_equal(slots['layers.1.feed_forward.w1w3.scales'][1::2], u)
    assert slots['output.weight'].dtype == f16 and not any(k.endswith('output_scale') for k in slots)
    with pytest.raises(ValueError, match='tp = 2'):
        export_weights(cfg, w, 2, 0)


def _edit_config(path, fn):
    f = os.path.join(path, 'config.json')
    with open(f) as fh:
        c = json.load(fh)
    fn(c)
    with open(f, 'w') as fh:
        json.dump(c, fh)


def _q(c):
    return c['quantization_config']


REFUSALS = [
    ('int4 weights', lambda c: _q(c)['global_quant_config']['weight'].update(dtype='int4'), 'global_quant_config.weight.dtype'),
    ('per-channel weights', lambda c: _q(c)['global_quant_config']['weight'].update(qscheme='per_channel'), 'global_quant_config.weight.qscheme'),
    ('group 64', lambda c: _q(c)['global_quant_config']['weight'].update(group_size=64), 'global_quant_config.weight.group_size'),
    ('float scales', lambda c: _q(c)['global_quant_config']['weight'].update(scale_format='float32'), 'global_quant_config.weight.scale_format'),
    ('dynamic weights', lambda c: _q(c)['global_quant_config']['weight'].update(is_dynamic=True), 'global_quant_config.weight.is_dynamic'),
    ('static inputs', lambda c: _q(c)['global_quant_config']['input_tensors'].update(is_dynamic=False), 'global_quant_config.input_tensors.is_dynamic'),
    ('fp8 inputs', lambda c: _q(c)['global_quant_config']['input_tensors'].update(dtype='fp8_e4m3'), 'global_quant_config.input_tensors.dtype'),
    ('weight-only', lambda c: _q(c)['global_quant_config'].update(input_tensors=None), 'global_quant_config.input_tensors'),
    ('no global config', lambda c: _q(c).pop('global_quant_config'), 'global_quant_config'),
    ('decoder linear excluded', lambda c: _q(c)['exclude'].append('model.layers.0.mlp.down_proj'), 'exclude'),
    ('layer config changes a linear', lambda c: _q(c)['layer_quant_config'].update({'*down_proj': dict(weight=dict(dtype='fp8_e4m3'))}),
     "layer_quant_config['*down_proj']"),
    ('layer config changes k_proj weights', lambda c: _q(c)['layer_quant_config']['*k_proj']['weight'].update(dtype='int8'),
     "layer_quant_config['*k_proj']"),
    ('mixtral', lambda c: c.update(architectures=['MixtralForCausalLM'], num_local_experts=4, num_experts_per_tok=2), 'MixtralForCausalLM'),
    ('qwen3 moe', lambda c: c.update(architectures=['Qwen3MoeForCausalLM']), 'Qwen3MoeForCausalLM'),
    ('gpt-oss', lambda c: c.update(architectures=['GptOssForCausalLM']), 'GptOssForCausalLM'),
]


@pytest.mark.parametrize('what,edit,needle', REFUSALS, ids=[x[0] for x in REFUSALS])
def test_refusals(tmp_path, what, edit, needle):
    r.write_checkpoint(str(tmp_path), layers=1)
    assert checkpoint.read_config(str(tmp_path)).weight_format == 'mxfp4'
    _edit_config(str(tmp_path), edit)
    with pytest.raises((NotImplementedError, KeyError)) as ei:
        checkpoint.read_config(str(tmp_path))
    assert isinstance(ei.value, NotImplementedError) and needle in str(ei.value), repr(ei.value)


def test_tp_and_tensor_refusals(tmp_path):
    """tp = 2 is refused by the reader; a scale byte 255 and tensors of a foreign dtype or shape by the loader, by name"""
    import torch
    from safetensors.torch import load_file, save_file
    r.write_checkpoint(str(tmp_path), layers=1)
    with pytest.raises(NotImplementedError, match='tp = 2'):
        checkpoint.read_config(str(tmp_path), 2)
    cfg = checkpoint.read_config(str(tmp_path))
    f = os.path.join(str(tmp_path), 'model.safetensors')
    good = load_file(f)
    t = dict(good)
    s = t['model.layers.0.mlp.up_proj.weight_scale'].clone()
    s[3, 1] = 255
    t['model.layers.0.mlp.up_proj.weight_scale'] = s
    save_file(t, f)
    with pytest.raises(ValueError, match='up_proj.weight_scale: scale byte 255'):
        checkpoint.load_hf_weights(str(tmp_path), cfg)
    t = dict(good)
    t['model.layers.0.self_attn.o_proj.weight_scale'] = good['model.layers.0.self_attn.o_proj.weight_scale'][:, :-1].contiguous()
    save_file(t, f)
    with pytest.raises(ValueError, match='o_proj'):
        checkpoint.load_hf_weights(str(tmp_path), cfg)
    t = dict(good)
    t['model.layers.0.self_attn.q_proj.weight'] = torch.zeros((256, 256), dtype=torch.float16)
    save_file(t, f)
    with pytest.raises(ValueError, match='q_proj'):
        checkpoint.load_hf_weights(str(tmp_path), cfg)


def test_qwen_readers_take_the_layout(tmp_path):
    """the dense Qwen3 reader: same quantization_config, per-head q / k norms next to the MXFP4 projections"""
    import torch
    from safetensors.torch import load_file, save_file
    r.write_checkpoint(str(tmp_path), layers=1, arch='Qwen3ForCausalLM')
    f = os.path.join(str(tmp_path), 'model.safetensors')
    t = load_file(f)
    for n in ('q_norm', 'k_norm'):
        t[f'model.layers.0.self_attn.{n}.weight'] = torch.ones(128, dtype=torch.float16)
    save_file(t, f)
    cfg, w, slots = _load(str(tmp_path))
    assert cfg.arch == 'qwen3' and cfg.weight_format == 'mxfp4' and cfg.qk_norm == 1
    assert slots['layers.0.attention.w_qkv.blocks'].dtype == np.uint8


# ---- config acceptance and the C-ABI's documents ---------------------------------------------------------------------------------------
def test_config_accepts_mxfp4():
    from lmdeploy_amd import TurbomindEngineConfig
    assert TurbomindEngineConfig(model_format='mxfp4').model_format == 'mxfp4'
    with pytest.raises(NotImplementedError, match='mxfp4'):
        TurbomindEngineConfig(model_format='mxfp6')
    assert 'mxfp4' in TurbomindEngineConfig.__doc__ and 'quark' in TurbomindEngineConfig.__doc__
    assert checkpoint.ModelConfig(hidden=256, layers=1, q_heads=2, kv_heads=1, head_dim=128, inter=256, vocab=512,
                                  weight_format='mxfp4').weight_format == 'mxfp4'


SYMBOLS = ('tm_linear_prepare_mxfp4', 'tm_quant_mxfp4_rows', 'tm_linear_mxfp4_workspace', 'tm_linear_forward_mxfp4')


def test_symbols_are_declared_bound_and_documented():
    from lmdeploy_amd import _ffi
    header = open(os.path.join(ROOT, 'include', 'tm_mi355x.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for s in SYMBOLS:
        assert s + '(' in header, s
        assert s in _ffi._SIGNATURES, s
        assert '`' + s + '`' in doc, s
    assert 'MoE expert weights only' not in header
    assert len(_ffi._SIGNATURES['tm_linear_forward_mxfp4'][1]) == 10 and len(_ffi._SIGNATURES['tm_quant_mxfp4_rows'][1]) == 7
