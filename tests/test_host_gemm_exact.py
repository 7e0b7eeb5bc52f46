"""The exactly summable GEMM operands of tests/gemm_exact_reference.py, proved on the CPU: their fp32 sums do not depend on the
order or chunking, the oracle's dequantisers / quantiser / fp8 linear reproduce them exactly, and the expected bits are sharp --
one code off by one, one k term dropped or the scales of two adjacent groups exchanged changes them."""
import numpy as np
import pytest

from oracle import tm_oracle as o
from tests import gemm_exact_reference as r

f16, f32, f64 = np.float16, np.float32, np.float64
CASES = [(K, N, False) for K, N in r.SHAPES] + [r.GATED_SHAPE + (True,)]
IDS = [f'{K}x{N}{"-gated" if g else ""}' for K, N, g in CASES]
DENSE_M = 64
SITES = 240


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.mark.parametrize('K,N,gated', CASES, ids=IDS)
def test_fp32_sums_do_not_depend_on_order_or_chunking(K, N, gated):
    """24 random orders of the products, each cut into 1 .. 16 split-K-like slabs at random places, every slab summed serially in
    fp32 and the slabs summed in slice order and in reverse: always the float64 sum, bit for bit.  Four rows of the dense x
    (the rows are independent) against up to 128 columns, for the u4 / fp16 operand and the e4m3 one."""
    W = r.weights(K, N, gated)
    rng = np.random.default_rng(K + N)
    x = r.dense_x(DENSE_M, K, r.X_SEED)[:4]
    cols = np.sort(rng.permutation(N)[:128])
    for w in (W.w(), W.w8(), W.w8(True) if gated else None):
        if w is None:
            continue
        r.check_budget(x, w, W.lsb, r.DENSE_BUDGET)
        prod = (x.astype(f64)[:, :, None] * w[None, :, cols]).astype(f32)           # [4][K][cols], each product exact
        assert np.array_equal(prod.astype(f64), x.astype(f64)[:, :, None] * w[None, :, cols])
        want = prod.astype(f64).sum(axis=1).astype(f32)
        assert np.array_equal(want.astype(f64), x.astype(f64) @ w[:, cols])
        for trial in range(24):
            order = rng.permutation(K) if trial else np.arange(K)
            slabs = int(rng.integers(1, 17))
            cuts = np.sort(rng.choice(np.arange(1, K), slabs - 1, replace=False)) if trial % 2 else np.arange(1, slabs) * (K // slabs)
            parts = [np.cumsum(c, axis=1, dtype=f32)[:, -1] for c in np.split(prod[:, order], cuts, axis=1)]
            for seq in (parts, parts[::-1]):
                acc = np.zeros_like(want)
                for part in seq:
                    acc = (acc + part).astype(f32)
                assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)), f'trial {trial}: {slabs} slabs'


@pytest.mark.parametrize('K,N,gated', CASES, ids=IDS)
def test_oracle_dequantisers_return_the_integers(K, N, gated):
    W = r.weights(K, N, gated)
    q, s, z = W.u4()
    assert np.array_equal(o.w4a16_dequant(q, s, z).astype(f64), W.w())
    assert np.array_equal(W.f16_weight().astype(f64), W.w())
    codes, sc = W.fp8()
    assert np.array_equal(o.fp8_dequant(codes, sc).astype(f64), W.w8())
    if gated:
        codes, sc = W.fp8(gated=True)
        assert np.array_equal(o.fp8_dequant(codes, sc, gated=True).astype(f64), W.w8(True))
    # a neighbour's scale is another scale: adjacent groups of a column never share one
    assert (np.diff(W.e, axis=0) != 0).all() and (np.diff(W.e8, axis=0) != 0).all()
    assert W.e.min() == W.e0 and W.e.max() == W.e0 + 3


@pytest.mark.parametrize('K', sorted({K for K, _ in r.SHAPES}))
def test_fp8_activation_quantiser_is_exact(K):
    """dense x and every launch of a few-hot sweep: scale 2^-6 wherever the group holds a +-7, codes e4m3(64 x)"""
    xs = [r.dense_x(130, K, r.X_SEED)] + [r.fewhot_x(K, 64, t) for t in range(r.fewhot_launches(K, 64))]
    for x in xs:
        codes, sx = o.fp8_quant_rows(x.astype(f16))
        live = np.abs(x.reshape(x.shape[0], -1, 128)).max(axis=2).T == 7
        assert np.array_equal(sx[live], np.full(int(live.sum()), 2.0**-6, f32))
        assert np.array_equal(codes, o.fp8_e4m3_from_f32((64 * x).astype(f32)))
        assert np.array_equal(o.fp8_e4m3_to_f32(codes).astype(np.int64), 64 * x)
        assert live.any()
    assert (np.abs(xs[0].reshape(130, -1, 128)).max(axis=2) == 7).all()


@pytest.mark.parametrize('K,N,gated', [c for c in CASES if c[1] % 32 == 0], ids=[i for c, i in zip(CASES, IDS) if c[1] % 32 == 0])
def test_oracle_fp8_linear_equals_the_exact_result(K, N, gated):
    W = r.weights(K, N, gated)
    x = r.dense_x(DENSE_M, K, r.X_SEED)
    codes, sc = W.fp8()
    assert np.array_equal(_bits(o.fp8_act_linear(x.astype(f16), codes, sc)), _bits(r.expected(x, W.w8(), W.lsb)))
    if gated:
        codes, sc = W.fp8(gated=True)
        got = o.fp8_act_linear(x.astype(f16), codes, sc, gated=True)
        assert np.array_equal(_bits(got), _bits(r.expected(x, W.w8(True), W.lsb, gated=True)))
    for t in (0, r.fewhot_launches(K, 64) - 1):
        xf, yf = r.fewhot_expected(K, 64, t, W.w8(), W.lsb)
        assert np.array_equal(_bits(o.fp8_act_linear(xf.astype(f16), *W.fp8())), _bits(yf))


def test_gated_accumulators_sit_where_silu_is_not_saturated():
    K, N = r.GATED_SHAPE
    W = r.weights(K, N, True)
    x = r.dense_x(DENSE_M, K, r.X_SEED)
    for w in (W.w(), W.w8(), W.w8(True)):
        sigma = float(r.exact_acc(x, w, W.lsb).std())
        assert 1.5 <= sigma <= 4.5, sigma
    y = r.expected(x, W.w(), W.lsb, gated=True)
    assert np.isfinite(y).all() and float(np.abs(y.astype(f32)).mean()) > 0.25


def test_budget_check_refuses_what_is_not_exactly_summable():
    W = r.weights(384, 64)
    x = r.dense_x(4, 384, 1)
    with pytest.raises(ValueError):
        r.exact_acc(x * 2**16, W.w(), W.lsb)                    # 2^16 x the terms: over 2^23 units
    with pytest.raises(ValueError):
        r.fewhot_check_budget(384, 64, W.wint * 16)             # two terms of up to 7 * 240 units
    with pytest.raises(AssertionError):
        r.check_budget(x, W.w() / 2, W.lsb, r.DENSE_BUDGET)     # lsb must divide every term


@pytest.mark.parametrize('M', [64, 256, 300])
@pytest.mark.parametrize('K', sorted({K for K, _ in r.SHAPES}))
def test_few_hot_sweep_hits_every_k(K, M):
    hit = r.fewhot_coverage(K, M)
    assert hit.min() >= 1, f'k = {int(np.argmin(hit))} is never hit'
    if (K, M) == (4096, 64):
        assert r.fewhot_launches(K, M) == 32 and hit.max() == 1
    for t in range(r.fewhot_launches(K, M)):
        k0, k1, x0, x1 = r.fewhot_rows(K, M, t)
        assert np.array_equal(k0 // 128, k1 // 128) and (k0 != k1).all()
        assert ((np.abs(x0) == 7) | (np.abs(x1) == 7)).all() and (x0 != 0).all() and (x1 != 0).all()


_SWEEP = {}


def _fewhot_column(K, wcol):
    """column of the whole M = 64 sweep's outputs from one weight column (float64, exact)"""
    if K not in _SWEEP:
        rows = [r.fewhot_rows(K, 64, t) for t in range(r.fewhot_launches(K, 64))]
        _SWEEP[K] = [np.concatenate(c) for c in zip(*rows)]
    k0, k1, x0, x1 = _SWEEP[K]
    return x0 * wcol[k0] + x1 * wcol[k1] + 0.0


@pytest.mark.parametrize('K,N,gated', CASES, ids=IDS)
def test_expected_bits_are_sharp(K, N, gated):
    """240 random (k, n) sites per shape, operand (u4 / fp16: per-column scales; e4m3: block scales) and fault.  A code off by
    +-1, a dropped k term and the scales of two adjacent groups exchanged change the expected bits of the few-hot sweep at EVERY
    site.  The same faults change the dense case's expected fp16 bits (M = 64; the gated case: the gated outputs) at 90 % of the sites at least."""
    W = r.weights(K, N, gated)
    rng = np.random.default_rng(K * 5 + N)
    x = r.dense_x(DENSE_M, K, r.X_SEED).astype(f64)
    r.fewhot_check_budget(K, 64, W.wint)
    for name, e_cols in (('u4', W.e), ('e4m3', W.e8_columns(gated))):
        for kind in ('code', 'drop', 'swap'):
            # a zero term (q = z, one weight in 16) cannot be dropped: that fault's sites are drawn among the others
            flat = rng.choice(np.flatnonzero(W.wint) if kind == 'drop' else K * N, SITES, replace=False)
            sites = list(zip((flat // N).tolist(), (flat % N).tolist()))
            dense_changed = 0
            for k, n in sites:
                base = r.column(W.wint[:, n], e_cols[:, n])
                mut = r.column(*r.mutate(W.wint, e_cols, W.q, kind, k, n, rng))
                few0, few1 = _fewhot_column(K, base), _fewhot_column(K, mut)
                assert np.array_equal(few0.astype(f16).astype(f64), few0)
                same = np.array_equal(_bits(few0.astype(f16)), _bits(few1.astype(f16)))
                assert not same, f'{name} {kind} at ({k}, {n}) leaves the few-hot bits unchanged'
                if gated:                                       # the partner column of the (gate, up) pair is untouched
                    n2 = n ^ 1
                    pair = r.column(W.wint[:, n2], e_cols[:, n2])
                    cols0 = np.stack([base, pair][::1 if n % 2 == 0 else -1], axis=1)
                    cols1 = np.stack([mut, pair][::1 if n % 2 == 0 else -1], axis=1)
                    d0 = o.gated_silu_epilogue((x @ cols0).astype(f32))
                    d1 = o.gated_silu_epilogue((x @ cols1).astype(f32))
                else:
                    d0, d1 = (x @ base).astype(f16), (x @ mut).astype(f16)
                dense_changed += not np.array_equal(_bits(d0), _bits(d1))
            assert dense_changed >= 0.9 * SITES, f'{name} {kind}: the dense bits change at {dense_changed} of {SITES} sites only'
