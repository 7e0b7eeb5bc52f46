"""TurboQuant KV cache (quant_policy 42), host side: the config accepts it, the layer size, and the numpy reference of the contract
(tests/turboquant_reference.py) against the properties that define it -- Hadamard, Lloyd-Max codebooks, zero rows, reconstruction
error, byte packing."""
import math

import numpy as np
import pytest

from lmdeploy_amd import TurbomindEngineConfig
from lmdeploy_amd.messages import QuantPolicy
from lmdeploy_amd.turbomind import checkpoint
from oracle import tm_oracle as o
from tests import turboquant_reference as tq

f16, f32, f64 = np.float16, np.float32, np.float64


def test_config_accepts_turbo_quant():
    cfg = TurbomindEngineConfig(quant_policy=42)
    assert cfg.quant_policy is QuantPolicy.TURBO_QUANT
    assert int(cfg.quant_policy) == 42


def test_config_refuses_turbo_quant_with_tp():
    with pytest.raises(NotImplementedError, match='tp'):
        TurbomindEngineConfig(quant_policy=42, tp=2)


def test_model_checks_name_the_reason():
    base = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, inter=512, vocab=1024)
    ok = checkpoint.ModelConfig(head_dim=128, **base)
    checkpoint.check_kv_quant_policy(ok, 42)
    checkpoint.check_kv_quant_policy(checkpoint.ModelConfig(head_dim=64, **base), 8)       # every other policy passes
    with pytest.raises(NotImplementedError, match='head_dim 64'):
        checkpoint.check_kv_quant_policy(checkpoint.ModelConfig(head_dim=64, **base), 42)
    with pytest.raises(NotImplementedError, match='sliding window'):
        checkpoint.check_kv_quant_policy(checkpoint.ModelConfig(head_dim=128, window=40, **base), 42)
    with pytest.raises(NotImplementedError, match='sliding window'):
        checkpoint.check_kv_quant_policy(checkpoint.ModelConfig(head_dim=128, layer_windows=[0, 128], **base), 42)
    with pytest.raises(NotImplementedError, match='sinks'):
        checkpoint.check_kv_quant_policy(checkpoint.ModelConfig(head_dim=128, attn_sinks=1, **base), 42)
    with pytest.raises(NotImplementedError, match='tp'):
        checkpoint.check_kv_quant_policy(ok, 42, tp=2)


def test_layer_size(tm):
    assert tm.tm_kv_layer_size(2, 128, 64, 42) == 13312 == 2 * 64 * 104
    assert tq.TqBlockLayout(1, 2).layer_size == 13312
    for bits in (16, 8, 4):
        for heads, D in ((2, 128), (8, 128), (1, 64)):
            assert tm.tm_kv_layer_size(heads, D, 64, bits) == o.BlockLayout(1, heads, D, 64, bits).layer_size


def test_layout_regions_tile_the_layer():
    L = tq.TqBlockLayout(3, 2)
    seen = np.zeros(L.layer_size, np.int32)
    for hd in range(L.kv_heads):
        for ti in range(L.block_len):
            for off, size in ((L.k_data(hd, ti), 64), (L.v_data(hd, ti), 32), (L.k_param(hd, ti), 4), (L.v_param(hd, ti), 4)):
                seen[off:off + size] += 1
    assert (seen == 1).all()
    assert L.v_data(0, 0) == 64 * 64 and L.k_data(1, 0) == 64 * 96 and L.k_param(0, 0) == 2 * 64 * 96
    assert L.layer_offset(2) == 2 * 13312 and L.block_size == 3 * 13312


@pytest.mark.parametrize('D', [64, 128])
def test_hadamard(D):
    H = tq.hadamard(D)
    assert np.array_equal(H @ H, D * np.eye(D))
    assert np.array_equal(H, H.T)
    assert H[3, 5] == (-1) ** bin(3 & 5).count('1')


def _phi(x):
    return math.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _cdf(x):
    return 0.5 * (1 + math.erf(x / math.sqrt(2)))


@pytest.mark.parametrize('c,beta', [(tq.C2, tq.BETA2), (tq.C3, tq.BETA3)])
def test_codebooks_are_lloyd_max_of_the_normal(c, beta):
    c, beta = c.astype(f64), beta.astype(f64)
    assert np.abs(beta - (c[:-1] + c[1:]) / 2).max() <= 1e-6, 'boundaries are the midpoints of neighbouring centroids'
    edges = [-math.inf] + list(beta) + [math.inf]
    for i, ci in enumerate(c):
        a, b = edges[i], edges[i + 1]
        pa = 0.0 if math.isinf(a) else _phi(a)
        pb = 0.0 if math.isinf(b) else _phi(b)
        ca = 0.0 if math.isinf(a) else _cdf(a)
        cb = 1.0 if math.isinf(b) else _cdf(b)
        assert abs((pa - pb) / (cb - ca) - ci) <= 1e-3, 'each centroid is the N(0, 1) mean of its cell'


@pytest.mark.parametrize('D', [64, 128])
def test_zero_row(D):
    z = np.zeros((1, D), f16)
    for is_k in (True, False):
        q = tq.quantise(z, is_k)
        assert not q.params.view(np.uint16).any(), 'zero bytes of norms'
        for fn in (tq.dequant_rotated, tq.dequant_original):
            back = fn(q.codes, q.params, is_k)
            assert np.array_equal(back, np.zeros_like(back)) and not np.signbit(back).any(), 'a zero row back, +0, never NaN'


@pytest.mark.parametrize('D', [64, 128])
def test_reconstruction_nmse(D):
    x = np.random.default_rng(D).standard_normal((4096, D)).astype(f16)
    xf = x.astype(f64)
    for is_k, bound in ((True, 0.015), (False, 0.125)):
        q = tq.quantise(x, is_k)
        back = tq.dequant_original(q.codes, q.params, is_k)
        nmse = ((back - xf) ** 2).sum() / (xf ** 2).sum()
        print(f'D {D} {"K" if is_k else "V"} NMSE {nmse:.4f}')
        assert nmse <= bound
        # the rotated form is the same row: H is orthogonal up to sqrt(D)
        rot = tq.dequant_rotated(q.codes, q.params, is_k)
        assert np.allclose(rot @ tq.hadamard(D) / math.sqrt(D), back, rtol=0, atol=1e-12)


def test_pack_roundtrip_and_byte_order():
    rng = np.random.default_rng(0)
    k = rng.integers(0, 16, (5, 3, 128)).astype(np.uint8)
    v = rng.integers(0, 4, (5, 3, 128)).astype(np.uint8)
    kb, vb = tq.pack_k(k), tq.pack_v(v)
    assert kb.shape == (5, 3, 64) and vb.shape == (5, 3, 32) and kb.dtype == np.uint8
    assert np.array_equal(tq.unpack_k(kb), k) and np.array_equal(tq.unpack_v(vb), v)
    # the contract's shortcut: (raw >> 4p) & 0x000f000f is the pair (2p, 2p + 1); (raw >> 2p) & 0x00030003 likewise for V
    kw = kb.view('<u4').astype(np.uint32)       # [5, 3, 16]: dword w = dims 8w ..
    vw = vb.view('<u4').astype(np.uint32)       # [5, 3, 8]: dword w = dims 16w ..
    for p in range(4):
        pair = (kw >> (4 * p)) & 0x000f000f
        assert np.array_equal(pair & 0xffff, k.reshape(5, 3, 16, 8)[..., 2 * p])
        assert np.array_equal(pair >> 16, k.reshape(5, 3, 16, 8)[..., 2 * p + 1])
    for p in range(8):
        pair = (vw >> (2 * p)) & 0x00030003
        assert np.array_equal(pair & 0xffff, v.reshape(5, 3, 8, 16)[..., 2 * p])
        assert np.array_equal(pair >> 16, v.reshape(5, 3, 8, 16)[..., 2 * p + 1])


def test_cache_runs_under_the_oracle():
    """oracle.process_kv / flatten_kv on the substituted cache: bytes land where the layout says, other blocks and layers stay zero,
    and both dequantised forms come back"""
    rng = np.random.default_rng(1)
    L = tq.TqBlockLayout(2, 2)
    cache = tq.TqPagedKVCache(L, 4)
    table = np.array([2, 0])
    k = rng.standard_normal((70, 2, 128)).astype(f16)
    v = rng.standard_normal((70, 2, 128)).astype(f16)
    v[3, 1] = 0
    o.process_kv(cache, table, 1, k, v, None, None, 0)
    assert not cache.pool[[1, 3]].any() and not cache.pool[:, :L.layer_size].any()
    Kf, Vf = o.flatten_kv(cache, table, 1, 70)
    assert Kf.shape == (2, 70, 128) and Kf.dtype == f16
    assert not Vf[1, 3].view(np.uint16).any()
    kd, vd = cache.load_dequant(table, 1, 0, 0, 70, 'decode')
    assert np.array_equal(kd.astype(f16), Kf[0]) and np.array_equal(vd.astype(f16), Vf[0])
    nmse = ((Kf.astype(f64) - k.transpose(1, 0, 2)) ** 2).sum() / (k.astype(f64) ** 2).sum()
    assert nmse <= 0.015


def test_ambiguity_report():
    """an element placed on a boundary is reported; a plain Gaussian row reports (almost) nothing"""
    x = np.random.default_rng(2).standard_normal((256, 128)).astype(f16)
    q = tq.quantise(x, True)
    assert tq.ambiguous_exact(q).mean() < 1e-3
    q.y[0, 7] = q.bounds[0, 5]
    assert tq.ambiguous_exact(q)[0, 7]
    assert tq.ambiguous_abs(q, np.full(256, 1e-3))[0, 7]
