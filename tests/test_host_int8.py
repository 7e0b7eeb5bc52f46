"""INT8 W8A8 checkpoints on the host: the four new C-ABI symbols at every layer of the boundary, both config dialects and every
accepted scale shape through read_config / load_hf_weights (codes times scales against the written dequantised weights, through the
q / k permutation, the q | k | v concatenation and the gate / up interleave), tp = 2 shards, every refusal with its needle, and the
reference module's own arithmetic (tests/int8_reference.py)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.loader import export_weights
from tests import int8_reference as r

f16, f32 = np.float16, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('tm_quant_int8_token', 'tm_linear_prepare_int8', 'tm_linear_int8_workspace', 'tm_linear_forward_int8')


def test_boundary_symbols():
    """the four entry points are declared in the header, exported by the built library, bound in _ffi and described in INTEGRATION.md"""
    header = open(os.path.join(ROOT, 'include', 'tm_mi355x.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib = ctypes.CDLL(os.path.join(ROOT, 'lmdeploy_amd', 'lib', 'libtm_mi355x.so'))
    for s in SYMBOLS:
        assert re.search(r'\b' + s + r'\(', header), s + ' is not declared in tm_mi355x.h'
        assert hasattr(lib, s), s + ' is not exported by libtm_mi355x.so'
        assert s in _ffi._SIGNATURES, s + ' is not bound in _ffi'
        assert '`' + s + '`' in integration, s + ' is not in INTEGRATION.md'
    assert re.search(r'TM_WEIGHT_I8\s*=\s*4\b', header)


def _load(path, tp=1, rank=0):
    cfg = checkpoint.read_config(path, tp)
    w = checkpoint.load_hf_weights(path, cfg)
    return cfg, w, export_weights(cfg, w, tp, rank)


def _deq(lin):
    assert set(lin) == {'i8', 'cs'}, sorted(lin)
    assert lin['i8'].dtype == np.int8 and lin['cs'].dtype == f32 and lin['cs'].shape == (lin['i8'].shape[1],)
    return lin['i8'].astype(f32) * lin['cs'][None, :]


MODELS = {'llama': {}, 'llama-d64': dict(head_dim=64, q_heads=4, kv_heads=2), 'qwen2': dict(arch='Qwen2ForCausalLM')}
FORMS = [('smooth_quant', 'channel', '[N,1]', f32), ('compressed-tensors', 'channel', '[N,1]', f32),
         ('compressed-tensors', 'channel', '[N]', f16), ('compressed-tensors', 'tensor', '[]', f32),
         ('compressed-tensors', 'tensor', '[1]', f16)]


@pytest.mark.parametrize('dialect,strategy,scale_shape,scale_dtype', FORMS, ids=[f'{d}-{s}-{sh}-{np.dtype(t).name}' for d, s, sh, t in FORMS])
@pytest.mark.parametrize('model', list(MODELS))
def test_reader_and_loader(tmp_path, model, dialect, strategy, scale_shape, scale_dtype):
    """both dialects, every accepted scale shape and two scale dtypes, Llama with head_dim 128 and 64 and Qwen2 with its bias:
    weight_format 'int8', codes times scales equal to the written dequantised weights in the engine's layout, int8 / fp32 slots"""
    geo = MODELS[model]
    ck = r.write_checkpoint(str(tmp_path), dialect=dialect, strategy=strategy, scale_shape=scale_shape, scale_dtype=scale_dtype, seed=3, **geo)
    cfg, w, slots = _load(str(tmp_path))
    assert cfg.weight_format == 'int8' and cfg.quantized and cfg.fp8_scale_mode == 0 and cfg.head_dim == geo.get('head_dim', 128)
    ref = r.tm_weights(ck, r.oracle_config(ck, 16))
    for i, (a, b) in enumerate(zip(w['layers'], ref['layers'])):
        for k in ('w_qkv', 'wo', 'w1w3', 'w2'):
            assert np.array_equal(_deq(a[k]), b[k]['deq']), f'layers.{i}.{k}: codes * scales differ from the written weights'
            assert np.array_equal(a[k]['i8'], b[k]['i8']) and np.array_equal(a[k]['cs'], b[k]['cs']), f'layers.{i}.{k}'
        assert ('qkv_bias' in a) == (model == 'qwen2')
        if model == 'qwen2':
            assert np.array_equal(a['qkv_bias'], b['qkv_bias'])
    assert np.array_equal(w['output'], ref['output']) and w['output'].dtype == f16       # lm_head stays fp16
    nq = (cfg.q_heads + 2 * cfg.kv_heads) * cfg.head_dim
    assert slots['layers.0.attention.w_qkv.weight'].dtype == np.int8 and slots['layers.0.attention.w_qkv.weight'].shape == (256, nq)
    assert slots['layers.0.attention.w_qkv.scales'].dtype == f32 and slots['layers.0.attention.w_qkv.scales'].shape == (nq,)
    assert slots['layers.1.feed_forward.w1w3.scales'].shape == (2 * cfg.inter,) and slots['layers.1.feed_forward.w2.scales'].shape == (256,)
    assert slots['output.weight'].dtype == f16


def test_scales_move_with_their_columns(tmp_path):
    """per-tensor scales: q, k and v carry three different scalars, each repeated over its own columns; per-channel: the q scales are
    permuted (not the identity), gate scales on the even and up scales on the odd columns of w1w3"""
    ck = r.write_checkpoint(str(tmp_path / 't'), dialect='compressed-tensors', strategy='tensor', seed=6)
    cfg, w, _ = _load(str(tmp_path / 't'))
    nq, nkv = cfg.q_heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    s = [float(ck[f'model.layers.0.self_attn.{n}_proj.weight_scale']) for n in 'qkv']
    assert len(set(s)) == 3
    assert np.array_equal(w['layers'][0]['w_qkv']['cs'], np.repeat(np.asarray(s, f32), [nq, nkv, nkv]))
    ck = r.write_checkpoint(str(tmp_path / 'c'), dialect='smooth_quant', seed=7)
    cfg, w, _ = _load(str(tmp_path / 'c'))
    L, p = w['layers'][1], 'model.layers.1.'
    sq = ck[p + 'self_attn.q_proj.scale'].reshape(-1)
    assert not np.array_equal(L['w_qkv']['cs'][:nq], sq) and np.array_equal(np.sort(L['w_qkv']['cs'][:nq]), np.sort(sq))
    assert np.array_equal(L['w1w3']['cs'][0::2], ck[p + 'mlp.gate_proj.scale'].reshape(-1))
    assert np.array_equal(L['w1w3']['cs'][1::2], ck[p + 'mlp.up_proj.scale'].reshape(-1))


def test_static_scales_are_read_past(tmp_path):
    """input_scale / k_scale / v_scale tensors and a kv_cache_scheme: the same slots as without them"""
    kw = dict(dialect='compressed-tensors', strategy='tensor', seed=8)
    r.write_checkpoint(str(tmp_path / 'dyn'), **kw)
    ck = r.write_checkpoint(str(tmp_path / 'static'), static=True, **kw)
    assert 'model.layers.0.self_attn.k_proj.k_scale' in ck and 'model.layers.0.mlp.up_proj.input_scale' in ck
    (_, _, a), (_, _, b) = _load(str(tmp_path / 'dyn')), _load(str(tmp_path / 'static'))
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('dialect', ['smooth_quant', 'compressed-tensors'])
def test_shards_tp2(tmp_path, dialect):
    """tp = 2 is not refused: column-parallel shards slice the scales with their columns, row-parallel shards keep them whole, and
    the two ranks' w_qkv and wo pieces put together are the unsharded linears"""
    r.write_checkpoint(str(tmp_path), dialect=dialect, q_heads=4, kv_heads=2, seed=9)
    cfg = checkpoint.read_config(str(tmp_path), 2)
    w = checkpoint.load_hf_weights(str(tmp_path), cfg)
    ranks = [export_weights(cfg, w, 2, rk) for rk in (0, 1)]
    D, I = cfg.head_dim, cfg.inter
    nq, nkv = cfg.q_heads * D, cfg.kv_heads * D
    for li, L in enumerate(w['layers']):
        p = f'layers.{li}.'
        qkv_w, qkv_s = np.empty_like(L['w_qkv']['i8']), np.empty_like(L['w_qkv']['cs'])
        for rk, s in enumerate(ranks):
            cols = np.r_[rk * nq // 2:(rk + 1) * nq // 2, nq + rk * nkv // 2:nq + (rk + 1) * nkv // 2,
                         nq + nkv + rk * nkv // 2:nq + nkv + (rk + 1) * nkv // 2]
            assert s[p + 'attention.w_qkv.weight'].dtype == np.int8 and s[p + 'attention.w_qkv.weight'].shape == (cfg.hidden, len(cols))
            qkv_w[:, cols], qkv_s[cols] = s[p + 'attention.w_qkv.weight'], s[p + 'attention.w_qkv.scales']
            assert np.array_equal(s[p + 'attention.wo.scales'], L['wo']['cs'])
            assert np.array_equal(s[p + 'feed_forward.w1w3.weight'], L['w1w3']['i8'][:, rk * I:(rk + 1) * I])
            assert np.array_equal(s[p + 'feed_forward.w1w3.scales'], L['w1w3']['cs'][rk * I:(rk + 1) * I])
            assert np.array_equal(s[p + 'feed_forward.w2.weight'], L['w2']['i8'][rk * I // 2:(rk + 1) * I // 2])
            assert np.array_equal(s[p + 'feed_forward.w2.scales'], L['w2']['cs'])
        assert np.array_equal(qkv_w, L['w_qkv']['i8']) and np.array_equal(qkv_s, L['w_qkv']['cs'])
        assert np.array_equal(np.concatenate([s[p + 'attention.wo.weight'] for s in ranks]), L['wo']['i8'])


def _edit_config(path, fn):
    f = os.path.join(path, 'config.json')
    with open(f) as fh:
        c = json.load(fh)
    fn(c)
    with open(f, 'w') as fh:
        json.dump(c, fh)


def _q(c):
    return c['quantization_config']


def _group(c):
    return _q(c)['config_groups']['group_0']


REFUSALS = [
    ('fp8 quant_dtype', 'smooth_quant', lambda c: _q(c).update(quant_dtype='float8_e4m3fn'), 'float8_e4m3fn'),
    ('decoder linear not converted', 'smooth_quant', lambda c: _q(c)['modules_to_not_convert'].append('down_proj'), 'down_proj'),
    ('4 bits', 'compressed-tensors', lambda c: _group(c)['weights'].update(num_bits=4), 'weights.num_bits'),
    ('group strategy', 'compressed-tensors', lambda c: _group(c)['weights'].update(strategy='group', group_size=128), 'weights.strategy'),
    ('asymmetric weights', 'compressed-tensors', lambda c: _group(c)['weights'].update(symmetric=False), 'weights.symmetric'),
    ('asymmetric activations', 'compressed-tensors', lambda c: _group(c)['input_activations'].update(symmetric=False),
     'input_activations.symmetric'),
    ('two groups', 'compressed-tensors', lambda c: _q(c)['config_groups'].update(group_1=_group(c)), 'config_groups'),
    ('decoder linear ignored', 'compressed-tensors', lambda c: _q(c)['ignore'].append('model.layers.0.mlp.down_proj'), 'down_proj'),
    ('float activations', 'compressed-tensors', lambda c: _group(c)['input_activations'].update(type='float'), 'input_activations.type'),
    ('weight-only', 'compressed-tensors', lambda c: _group(c).update(input_activations=None), 'input_activations'),
]


@pytest.mark.parametrize('what,dialect,edit,needle', REFUSALS, ids=[x[0] for x in REFUSALS])
def test_refusals(tmp_path, what, dialect, edit, needle):
    """each config is accepted as written and refused after the edit, with the offending key or name in the message"""
    r.write_checkpoint(str(tmp_path), dialect=dialect, layers=1)
    assert checkpoint.read_config(str(tmp_path)).weight_format == 'int8'
    _edit_config(str(tmp_path), edit)
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert needle in str(ei.value), str(ei.value)


@pytest.mark.parametrize('dialect', ['smooth_quant', 'compressed-tensors'])
@pytest.mark.parametrize('arch', ['MixtralForCausalLM', 'Qwen2MoeForCausalLM', 'Qwen3MoeForCausalLM'])
def test_moe_architectures_are_refused(tmp_path, arch, dialect):
    r.write_checkpoint(str(tmp_path), dialect=dialect, layers=1, arch=arch, experts=4)
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert arch in str(ei.value) and 'dense models only' in str(ei.value), str(ei.value)


def test_model_format_int8():
    """model_format='int8' is accepted by the engine config; both dialects' key names live in one table"""
    from lmdeploy_amd import TurbomindEngineConfig
    assert TurbomindEngineConfig(model_format='int8').model_format == 'int8'
    assert checkpoint.INT8['smooth_quant']['scale_suffix'] == '.scale' and checkpoint.INT8['compressed-tensors']['format'] == 'int-quantized'


# ---- the reference module checks itself -----------------------------------------------------------------------------------------
def test_reference_accumulator_bound():
    """acc in int64 equals the wrapping int32 sum, at the worst case of the contract: K = 32768, every product 127 * 128 (or its
    negative), |acc| = 32768 * 127 * 128 < 2^31"""
    K = r.K_MAX
    xq = np.full((2, K), -127, np.int8)
    xq[1] = 127
    wq = np.full((K, 2), -128, np.int8)
    wq[:, 1] = 127
    a = r.acc_i64(xq, wq)                                     # asserts < 2^31 itself
    assert np.abs(a).max() == K * 127 * 128 == 532676608 and K * 127 * 128 < 2**31
    a32 = (xq.astype(np.int32)[:, :, None] * wq.astype(np.int32)[None, :, :]).sum(axis=1, dtype=np.int32)
    assert np.array_equal(a32.astype(np.int64), a)
    rng = np.random.default_rng(0)
    xq, wq = rng.integers(-127, 128, (5, 640)).astype(np.int8), rng.integers(-128, 128, (640, 7)).astype(np.int8)
    a32 = np.zeros((5, 7), np.int32)
    for k0 in range(0, 640, 128):                             # any split of K sums to the same integers
        a32 += xq[:, k0:k0 + 128].astype(np.int32) @ wq[k0:k0 + 128].astype(np.int32)
    assert np.array_equal(a32.astype(np.int64), r.acc_i64(xq, wq))


def test_reference_quantiser_rules():
    """the four traps of the contract show on the reference itself: |x / sx| above 127 (the clamp), exact ties rounded away from
    zero where RNE would differ, the division against the reciprocal, and floor(q + 0.5f) in fp32"""
    a = 3
    tie = np.r_[(np.arange(-126, 127) + 0.5) * 2.0**a, 127 * 2.0**a].astype(f16)
    assert np.array_equal(tie.astype(np.float64), np.r_[(np.arange(-126, 127) + 0.5) * 2.0**a, 127 * 2.0**a])
    q, sx = r.quant(tie[None])
    assert sx[0] == f32(2.0**a)
    k = np.arange(-126, 127)
    assert np.array_equal(q[0, :-1], np.where(k >= 0, k + 1, k)) and q[0, -1] == 127
    assert int((np.rint((np.arange(-126, 127) + 0.5)) != q[0, :-1]).sum()) == 127        # RNE differs in 127 places
    q, sx = r.quant(np.full((1, 128), 2.0**-24, f16) * np.where(np.arange(128) % 2, -1, 1).astype(f16))
    assert sx[0] == f32(1e-7) / f32(127) and np.array_equal(np.abs(q[0]), np.full(128, 76))
    q, sx = r.quant(np.zeros((1, 128), f16))
    assert not q.any() and sx[0] == f32(1e-7) / f32(127)
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((64, 4224)) * rng.uniform(0.01, 30, (64, 1))).astype(f16)
    q, sx = r.quant(x)
    ratio = np.abs(x.astype(f32) / sx[:, None])
    assert ratio.max() > 127.0 and np.abs(q.astype(int)).max() == 127
    recip = np.clip(np.copysign(np.floor(np.abs((x.astype(f32) * (f32(127) / (sx * f32(127)))[:, None]).astype(np.float64)) + 0.5),
                                x.astype(np.float64)), -127, 127)
    assert (recip != q).any(), 'multiplying by 127 / absmax must differ from the division somewhere'
    assert np.floor(f32(0.49999997) + f32(0.5)) == 1.0        # the fp32 shortcut's trap; quant() rounds in float64
