"""W4A16 dialects on the host: GPTQ and compressed-tensors pack-quantized checkpoints read into the same (q, s, z) as AWQ.

The same linears written in the three dialects (w4_formats_reference) must give byte-identical export slots at group 128; group 32
(compressed-tensors) must give the slots a direct numpy construction gives; every refusal names its key or tensor, and the needles older
tests pin on 8-bit compressed-tensors configs keep their wording.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests import w4_formats_reference as r
from lmdeploy_amd import TurbomindEngineConfig
from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.loader import (AWQ_ORDER, export_weights, pack_u4_row, unpack_awq_gemm, unpack_u4_cols, unpack_u4_rows)

f16 = np.float16
# words that differ in every nibble, and whose top nibble sets the sign bit
WORDS = np.array([[0x76543210, 0xFEDCBA98], [0x89ABCDEF, 0x01234567]], np.uint32).view(np.int32)


def _nib(word, i):
    return (int(np.uint32(word)) >> (4 * i)) & 15


def test_unpack_orders():
    cols = unpack_u4_cols(WORDS)                    # [2, 16]: element 8c + j = nibble j of word c
    rows = unpack_u4_rows(WORDS)                    # [16, 2]: row 8r + i = nibble i of word r
    awq = unpack_awq_gemm(WORDS)
    for r_ in range(2):
        for c in range(2):
            w = WORDS.view(np.uint32)[r_, c]
            for j in range(8):
                assert cols[r_, 8 * c + j] == _nib(w, j)
                assert rows[8 * r_ + j, c] == _nib(w, j)
                assert awq[r_, 8 * c + j] == _nib(w, AWQ_ORDER[j])
    assert cols.dtype == rows.dtype == np.uint8
    # round trips: the engine's own sequential pack, and the test writers
    assert np.array_equal(pack_u4_row(cols), WORDS)
    assert np.array_equal(r.pack_nibbles_last(cols), WORDS) and np.array_equal(r.pack_nibbles_rows(rows), WORDS)
    q = np.random.default_rng(0).integers(0, 16, (24, 16)).astype(np.uint8)
    assert np.array_equal(unpack_u4_cols(r.pack_nibbles_last(q)), q) and np.array_equal(unpack_u4_rows(r.pack_nibbles_rows(q)), q)
    assert not np.array_equal(unpack_awq_gemm(r.pack_nibbles_last(q)), q)         # the two orders are not interchangeable


def test_key_tables_against_transformers():
    """the GPTQ config keys are GPTQConfig's; compressed_tensors, when importable, knows the format and tensor names"""
    import inspect

    from transformers import GPTQConfig
    params = inspect.signature(GPTQConfig.__init__).parameters
    for key, default, _ in checkpoint.W4['gptq']['config']:
        assert key in params, key
        if key != 'bits':
            assert params[key].default == default, key
    assert any(k in params for k in checkpoint.W4['gptq']['v2_keys'])
    try:
        import compressed_tensors
    except ImportError:
        return
    from compressed_tensors import CompressionFormat
    assert CompressionFormat.pack_quantized.value == checkpoint.W4['compressed-tensors']['format']


class _T(dict):
    """a stand-in for checkpoint._Tensors over a dict of numpy arrays"""
    get = dict.__getitem__


def _np(tensors):
    import torch
    return _T({k: (v.float() if v.dtype == torch.bfloat16 else v).numpy() for k, v in tensors.items()})


def _qsz(K=128, N=16, group=128, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 16, (K, N)).astype(np.uint8)
    s = (rng.random((K // group, N)) * 0.01 + 0.001).astype(f16)
    z = rng.integers(1, 16, (K // group, N)).astype(np.uint8)
    return q, s, z


def test_gptq_zero_offsets():
    q, s, z = _qsz(256, 16)                         # two groups: a reversed g_idx differs from k // g
    z[0, :4] = (1, 15, 8, 2)
    for v2 in (False, True):
        t = _np(r.linear_tensors('p', q, s, z, 'gptq', gptq_v2=v2))
        stored = unpack_u4_cols(t['p.qzeros'])
        assert np.array_equal(stored, z - (0 if v2 else 1))
        t.w4 = dict(dialect='gptq', group=128, zero_offset=0 if v2 else 1)
        lin = checkpoint._linear(t, 'p', True)
        assert np.array_equal(lin['q'], q) and np.array_equal(lin['z'], z.astype(f16)) and lin['z'].dtype == f16
        assert np.array_equal(lin['s'].view(np.uint16), s.view(np.uint16))
    # a v2 checkpoint read with the v1 offset: stored 15 + 1 = 16
    t = _np(r.linear_tensors('model.layers.0.mlp.down_proj', q, s, z, 'gptq', gptq_v2=True))
    t.w4 = dict(dialect='gptq', group=128, zero_offset=1)
    with pytest.raises(ValueError, match='model.layers.0.mlp.down_proj.qzeros'):
        checkpoint._linear(t, 'model.layers.0.mlp.down_proj', True)
    # act-order
    t = _np(r.linear_tensors('p', q, s, z, 'gptq'))
    t['p.g_idx'] = t['p.g_idx'][::-1].copy()
    t.w4 = dict(dialect='gptq', group=128, zero_offset=1)
    with pytest.raises(NotImplementedError, match='p.g_idx'):
        checkpoint._linear(t, 'p', True)
    # shapes per dialect: a GPTQ tensor read as AWQ and the reverse are refused by name
    t = _np(r.linear_tensors('p', q, s, z, 'gptq'))
    t.w4 = dict(dialect='awq', group=128, zero_offset=1)
    with pytest.raises(ValueError, match='p.qweight'):
        checkpoint._linear(t, 'p', True)
    t = _np(r.linear_tensors('p', q, s, z, 'awq'))
    t.w4 = dict(dialect='gptq', group=128, zero_offset=1)
    with pytest.raises(ValueError, match='p.qweight'):
        checkpoint._linear(t, 'p', True)


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
@pytest.mark.parametrize('group', [128, 32])
def test_compressed_tensors_symmetric_zeros(dtype, group):
    q, s, z = _qsz(256, 16, group)
    if dtype == 'bfloat16':
        s = (s.view(np.uint16) & 0xFFE0).view(f16)            # scales a bf16 holds exactly (normal fp16 values fit its exponent)
    t = _np(r.linear_tensors('p', q, s, z, 'compressed-tensors', symmetric=True, scale_dtype=dtype))
    assert 'p.weight_zero_point' not in t and t['p.weight_packed'].shape == (16, 32)
    t.w4 = dict(dialect='compressed-tensors', group=group, zero_offset=1)
    lin = checkpoint._linear(t, 'p', True)
    assert lin['z'].shape == (256 // group, 16) and lin['z'].dtype == f16 and (lin['z'] == 8).all()
    assert np.array_equal(lin['q'], q) and lin['s'].dtype == f16 and np.array_equal(lin['s'].view(np.uint16), s.view(np.uint16))
    # asymmetric: the zero points come back; a wrong weight_shape is refused by name
    t = _np(r.linear_tensors('p', q, s, z, 'compressed-tensors'))
    t.w4 = dict(dialect='compressed-tensors', group=group, zero_offset=1)
    assert np.array_equal(checkpoint._linear(t, 'p', True)['z'], z.astype(f16))
    t['p.weight_shape'] = np.array([256, 16], np.int64)
    with pytest.raises(ValueError, match='p.weight_shape'):
        checkpoint._linear(t, 'p', True)


# ---- equivalence: three dialects, one set of slots ---------------------------------------------------------------------------------
_MODELS = {}


def _model(kind, group=128, D=128):
    key = (kind, group, D)
    if key not in _MODELS:
        _MODELS[key] = r.make_model(kind, group, D=D)
    return _MODELS[key]


def _slots(path, tp):
    cfg = checkpoint.read_config(path, tp)
    w = checkpoint.load_hf_weights(path, cfg)
    return cfg, [export_weights(cfg, w, tp, rank) for rank in range(tp)]


@pytest.mark.parametrize('tp', [1, 2])
@pytest.mark.parametrize('kind', ['llama', 'qwen2', 'qwen3', 'qwen3_moe'])
def test_three_dialects_one_set_of_slots(tmp_path, kind, tp):
    model = _model(kind)
    got = {}
    for d in r.DIALECTS:
        p = tmp_path / d
        p.mkdir()
        r.write_model(str(p), model, d)
        cfg, got[d] = _slots(str(p), tp)
        assert (cfg.weight_format, cfg.group, cfg.group_size, cfg.w4_dialect) == ('u4', 128, 128, d)
    for d in ('gptq', 'compressed-tensors'):
        for rank in range(tp):
            a, b = got['awq'][rank], got[d][rank]
            assert list(a) == list(b)
            for name in a:
                assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), (d, name)
    names = list(got['awq'][0])
    assert any(n.endswith('w_qkv.qweight') for n in names) and ('layers.0.attention.w_qkv.bias' in names) == (kind == 'qwen2')
    assert ('layers.0.attention.q_norm.weight' in names) == kind.startswith('qwen3')
    if kind == 'qwen3_moe':
        assert 'layers.0.moe_ffn.experts.3.w2.zeros' in names and got['awq'][0]['layers.0.moe_ffn.gate.weight'].dtype == f16


def test_gptq_v2_and_no_g_idx_give_the_same_slots(tmp_path):
    model = _model('llama')
    out = []
    for i, opts in enumerate((dict(), dict(gptq_v2=True), dict(g_idx=False))):
        p = tmp_path / str(i)
        p.mkdir()
        r.write_model(str(p), model, 'gptq', **opts)
        cfg, (s,) = _slots(str(p), 1)
        assert cfg.w4_zero_offset == (0 if opts.get('gptq_v2') else 1)
        out.append(s)
    for s in out[1:]:
        assert all(s[n].tobytes() == out[0][n].tobytes() for n in out[0])


@pytest.mark.parametrize('tp', [1, 2])
@pytest.mark.parametrize('D', [128, 64])
def test_group_32_slots(tmp_path, tp, D):
    """group 32: the slots are what a direct numpy construction gives, shard arithmetic included (host only: tp > 1 with group 32 has
    not run on a GPU)"""
    model = _model('llama', 32, D)
    r.write_model(str(tmp_path), model, 'compressed-tensors')
    cfg, slots = _slots(str(tmp_path), tp)
    assert cfg.group_size == 32 and cfg.group == 32 and cfg.weight_format == 'u4' and cfg.head_dim == D
    g = r.GEOMETRY
    H, Hq, Hkv, I = g['H'], g['Hq'], g['Hkv'], g['I']
    perm = lambda a, h: a.reshape(a.shape[0], h, 2, D // 2).swapaxes(-1, -2).reshape(a.shape[0], h * D)
    for rank in range(tp):
        s = slots[rank]
        p = 'model.layers.1'
        # wo: row-parallel, whole groups of 32
        q, sc, z = model['quant'][p + '.self_attn.o_proj']
        k0, k1 = rank * Hq * D // tp, (rank + 1) * Hq * D // tp
        assert np.array_equal(s['layers.1.attention.wo.qweight'], pack_u4_row(q[k0:k1]))
        assert s['layers.1.attention.wo.scales'].shape == ((k1 - k0) // 32, H)
        assert np.array_equal(s['layers.1.attention.wo.scales'], sc[k0 // 32:k1 // 32])
        assert np.array_equal(s['layers.1.attention.wo.zeros'], z[k0 // 32:k1 // 32].astype(f16))
        # w_qkv: column-parallel, q / k permuted for the interleaved RoPE
        parts = []
        for n, h in (('q_proj', Hq), ('k_proj', Hkv), ('v_proj', Hkv)):
            zz = model['quant'][f'{p}.self_attn.{n}'][2].astype(f16)
            zz = perm(zz, h) if n != 'v_proj' else zz
            hl = h // tp
            parts.append(zz[:, rank * hl * D:(rank + 1) * hl * D])
        assert np.array_equal(s['layers.1.attention.w_qkv.zeros'], np.concatenate(parts, 1))
        assert s['layers.1.attention.w_qkv.zeros'].shape == (H // 32, (Hq + 2 * Hkv) * D // tp)
        # w1w3: (gate_j, up_j) interleaved columns of this rank; w2 rows
        (qg, sg, _), (qu, su, _) = model['quant'][p + '.mlp.gate_proj'], model['quant'][p + '.mlp.up_proj']
        il = I // tp
        want = np.empty((H // 32, 2 * il), f16)
        want[:, 0::2], want[:, 1::2] = sg[:, rank * il:(rank + 1) * il], su[:, rank * il:(rank + 1) * il]
        assert np.array_equal(s['layers.1.feed_forward.w1w3.scales'], want)
        assert s['layers.1.feed_forward.w2.scales'].shape == (il // 32, H)
    from lmdeploy_amd.turbomind.engine import make_model_config
    assert make_model_config(cfg, 0).group_size == 32


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _edit_config(path, edit):
    with open(os.path.join(path, 'config.json')) as f:
        c = json.load(f)
    edit(c)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)


def _q(c):
    return c['quantization_config']


def _w(c):
    return _q(c)['config_groups']['group_0']['weights']


REFUSALS = [
    ('gptq bits', 'gptq', lambda c: _q(c).update(bits=8), 'bits'),
    ('gptq group_size', 'gptq', lambda c: _q(c).update(group_size=32), 'group_size'),
    ('gptq sym', 'gptq', lambda c: _q(c).update(sym=False), 'sym'),
    ('gptq desc_act', 'gptq', lambda c: _q(c).update(desc_act=True), 'desc_act'),
    ('ct group_size', 'compressed-tensors', lambda c: _w(c).update(group_size=64), 'weights.group_size'),
    ('ct channel', 'compressed-tensors', lambda c: _w(c).update(strategy='channel', group_size=None), 'weights.strategy'),
    ('ct tensor', 'compressed-tensors', lambda c: _w(c).update(strategy='tensor', group_size=None), 'weights.strategy'),
    ('ct dynamic', 'compressed-tensors', lambda c: _w(c).update(dynamic=True), 'weights.dynamic'),
    ('ct actorder', 'compressed-tensors', lambda c: _w(c).update(actorder='group'), 'weights.actorder'),
    ('ct two groups', 'compressed-tensors', lambda c: _q(c)['config_groups'].update(group_1=_q(c)['config_groups']['group_0']),
     'config_groups'),
    ('ct decoder linear ignored', 'compressed-tensors', lambda c: _q(c)['ignore'].append('model.layers.0.mlp.down_proj'), 'down_proj'),
    ('ct 8-bit pack-quantized', 'compressed-tensors', lambda c: _w(c).update(num_bits=8), 'format'),
    ('ct activations', 'compressed-tensors',
     lambda c: _q(c)['config_groups']['group_0'].update(input_activations={'num_bits': 8, 'type': 'int', 'strategy': 'token'}), 'format'),
]


@pytest.mark.parametrize('what,dialect,edit,needle', REFUSALS, ids=[x[0] for x in REFUSALS])
def test_refusals(tmp_path, what, dialect, edit, needle):
    r.write_model(str(tmp_path), _model('llama'), dialect)
    assert checkpoint.read_config(str(tmp_path)).weight_format == 'u4'
    _edit_config(str(tmp_path), edit)
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert needle in str(ei.value), str(ei.value)


def test_ignore_list_may_name_router_gates(tmp_path):
    r.write_model(str(tmp_path), _model('qwen3_moe'), 'compressed-tensors')
    _edit_config(str(tmp_path), lambda c: _q(c).update(ignore=['lm_head', 're:.*mlp.gate$']))
    assert checkpoint.read_config(str(tmp_path)).moe_experts == 4


def test_group_32_moe_is_refused(tmp_path):
    r.write_model(str(tmp_path), _model('qwen3_moe'), 'compressed-tensors')
    _edit_config(str(tmp_path), lambda c: _w(c).update(group_size=32))
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert 'Qwen3MoeForCausalLM' in str(ei.value) and 'group_size = 32' in str(ei.value) and 'dense models only' in str(ei.value)


def test_pinned_needles_on_their_original_configs(tmp_path):
    """the 8-bit compressed-tensors refusals older tests pin keep naming the same keys"""
    from tests import fp8_channel_reference as f8
    from tests import int8_reference as i8

    def group(c):
        return next(iter(_q(c)['config_groups'].values()))
    cases = [
        (lambda p: f8.write_checkpoint(p, dialect='compressed-tensors', strategy='channel', layers=1), [
            (lambda c: group(c)['weights'].update(num_bits=4), 'weights.num_bits'),
            (lambda c: group(c)['weights'].update(strategy='group', group_size=128), 'weights.strategy'),
            (lambda c: _q(c).update(format='pack-quantized'), 'format')]),
        (lambda p: i8.write_checkpoint(p, dialect='compressed-tensors', layers=1), [
            (lambda c: group(c)['weights'].update(num_bits=4), 'weights.num_bits'),
            (lambda c: group(c)['weights'].update(strategy='group', group_size=128), 'weights.strategy'),
            (lambda c: group(c).update(input_activations=None), 'input_activations')]),
    ]
    n = 0
    for write, edits in cases:
        for edit, needle in edits:
            p = tmp_path / str(n)
            p.mkdir()
            n += 1
            write(str(p))
            checkpoint.read_config(str(p))
            _edit_config(str(p), edit)
            with pytest.raises(NotImplementedError) as ei:
                checkpoint.read_config(str(p))
            assert needle in str(ei.value), str(ei.value)


# ---- public surface ----------------------------------------------------------------------------------------------------------------
def test_model_format_surface(tmp_path, monkeypatch):
    assert TurbomindEngineConfig(model_format='compressed-tensors').model_format == 'compressed-tensors'
    with pytest.raises(NotImplementedError):
        TurbomindEngineConfig(model_format='gptq')
    for needle in ('gptq', 'pack-quantized', 'group_size 128 or 32', 'gptq_v2'):
        assert needle in TurbomindEngineConfig.__doc__
    # the mismatch check runs before any GPU work: stop the constructor right behind it
    import importlib
    pl = importlib.import_module('lmdeploy_amd.pipeline')

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()
    monkeypatch.setattr(pl.checkpoint, 'check_kv_quant_policy', stop)
    dirs = {}
    for d in r.DIALECTS:
        dirs[d] = tmp_path / d
        dirs[d].mkdir()
        r.write_model(str(dirs[d]), _model('llama'), d)
    ok = [('awq', 'awq'), ('gptq', None), ('compressed-tensors', 'compressed-tensors'), ('compressed-tensors', None), ('awq', None)]
    for d, fmt in ok:
        with pytest.raises(Stop):
            pl.Pipeline(str(dirs[d]), TurbomindEngineConfig(model_format=fmt))
    bad = [('gptq', 'awq'), ('compressed-tensors', 'awq'), ('awq', 'compressed-tensors'), ('gptq', 'compressed-tensors'), ('gptq', 'fp8')]
    for d, fmt in bad:
        with pytest.raises(ValueError, match='model_format'):
            pl.Pipeline(str(dirs[d]), TurbomindEngineConfig(model_format=fmt))
    # the refusal of an unknown 4-bit method names what is served
    _edit_config(str(dirs['awq']), lambda c: _q(c).update(quant_method='hqq'))
    with pytest.raises(NotImplementedError, match='GPTQ 4-bit group 128.*pack-quantized'):
        checkpoint.read_config(str(dirs['awq']))
