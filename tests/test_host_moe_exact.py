"""The exactly summable MoE blocks of tests/moe_exact_reference.py, proved on the CPU: the saturated gate and the tied router are
exact in float32, the budgets hold, float32 arithmetic in any order and row tiling returns the float64 expectation bit for bit,
the expectation is o.moe_ffn's on the same operands, and the expected bits are sharp -- every fault of the list in the reference
module changes at least one output bit at every block the device test runs."""
import numpy as np
import pytest

from oracle import tm_oracle as o
from tests import moe_exact_reference as r

f16, f32, f64 = np.float16, np.float32, np.float64
BLOCKS = [(H, I, E, k, s) for H, I in r.GEOMETRIES for E, k, s in r.CONFIGS]
IDS = [f'H{H}-I{I}-E{E}-k{k}' for H, I, E, k, s in BLOCKS]
SHARED_CONFIG = r.CONFIGS[0]


def test_saturated_gate_and_shared_sigmoid_are_exact_in_float32():
    """a / (1 + expf(-a)) == a for the gate values used (as a quotient and as a * (1 / (1 + expf(-a)))), so the epilogue's product
    is a * u, exact for a power of two; the shared gate's sigmoid is exactly 1 at logit 32 and exactly 0 at -128"""
    rng = np.random.default_rng(0)
    u = rng.standard_normal(4096).astype(f32)
    for a in (32.0, 64.0, 128.0, 256.0):
        a = f32(a)
        den = (f32(1) + np.exp(-a).astype(f32)).astype(f32)
        assert den == f32(1) and a / den == a and a * (f32(1) / den) == a
        assert np.array_equal(o.silu_f32(np.full(1, a)), np.full(1, a))
        acc = np.stack([np.full_like(u, a), u], axis=1).reshape(-1, 2)
        assert np.array_equal(o.gated_silu_epilogue(acc).view(np.uint16).ravel(), (u.astype(f64) * a).astype(f16).view(np.uint16))
    with np.errstate(over='ignore'):
        assert f32(1) / (f32(1) + np.exp(f32(-32.0))) == f32(1)
        assert np.isinf(np.exp(f32(128.0))) and f32(1) / (f32(1) + np.exp(f32(128.0))) == f32(0)
    for k, s in ((2, 1.0), (1, 2.0), (8, 1.0), (4, 0.5)):                  # p = expf(0) = 1, denom = k, w = 1 * (1 / k) * scale
        p = np.exp(f32(0))
        denom = f32(0)
        for _ in range(k):
            denom += p
        assert p * (f32(1) / denom) * f32(s) == f32(s / k)


@pytest.mark.parametrize('H,I,E,k,s', BLOCKS, ids=IDS)
def test_budgets_hold_and_the_builder_checks_itself(H, I, E, k, s):
    """forward() asserts every budget, lattice, the gate powers, the epilogue identity and the routing; here at the largest
    forward, at the edge routing and with an expert that takes every token, for both operand families"""
    B = r.Block(H, I, E, k, s)
    for fam in r.FAMILIES:
        for T, routing in ((300, 'random'), (64, 'edge'), (37, 'one'), (1, 'random')):
            x, ids = r.make_x(B, T, routing)
            res = r.forward(B, fam, x, ids)
            assert max(res.worst) <= r.BUDGET
            assert np.array_equal(res.ids, ids) and np.isfinite(res.out).all()
            if routing == 'edge':
                hist = np.diff(res.offsets)
                assert hist[1] == 2 * B.hint(T) and hist[2] == 2 * B.hint(T) + 1
            if routing == 'one':
                assert (np.diff(res.offsets) == 0).sum() >= E // 2 and np.diff(res.offsets)[3] == T
    x, ids = r.make_x(B, 37, 'random')
    assert set(x[:, H - 2].tolist()) == {1, 2} and set(x[:, H - 1].tolist()) == {1, -4}
    big = x.copy()
    big[:, E:H - 2] *= 2**7
    with pytest.raises(ValueError):
        r.forward(B, 'w', big, ids)                                        # 2^7 x the terms: over the budget, refused


def test_edge_routing_is_feasible_where_the_device_test_uses_it():
    for H, I, E, k, s in BLOCKS:
        B = r.Block(H, I, E, k, s)
        assert [T for T in r.TOKENS if not B.feasible(T, 'edge')] == [1]


@pytest.mark.parametrize('H,I', r.GEOMETRIES, ids=[f'H{H}-I{I}' for H, I in r.GEOMETRIES])
def test_float32_sums_do_not_depend_on_order_or_row_tiling(H, I):
    """(a) the segments cut into 16-, 32- and 64-row tiles, each tile a float32 matrix product (numpy's own blocking), the gated
    epilogue of the oracle, a float32 product with w2; (b) sixteen rows' products summed serially in float32 in 12 shuffled orders
    of k for both GEMMs; (c) the combine as a float32 fma chain over the picks in every rotation, shared term first: always the
    float64 expectation, bit for bit"""
    E, k, s = r.CONFIGS[2]
    B = r.Block(H, I, E, k, s)
    rng = np.random.default_rng(H)
    for fam in r.FAMILIES:
        x, ids = r.make_x(B, 64, 'edge')
        res = r.forward(B, fam, x, ids)
        for tile in (16, 32, 64):
            for e in np.flatnonzero(np.diff(res.offsets)):
                ex = B.expert(e)
                w13, w2 = ex.w13(fam).astype(f32), ex.w2(fam).astype(f32)
                for f0 in range(res.offsets[e], res.offsets[e + 1], tile):
                    rows = np.arange(f0, min(f0 + tile, res.offsets[e + 1]))
                    act = o.gated_silu_epilogue(x[res.f2n[rows]].astype(f32) @ w13)
                    assert np.array_equal(act.view(np.uint16), res.act[rows].view(np.uint16)), (fam, tile, e)
                    y2 = (act.astype(f32) @ w2).astype(f16)
                    assert np.array_equal(y2.view(np.uint16), res.y2[rows].view(np.uint16)), (fam, tile, e)
        e = int(np.argmax(np.diff(res.offsets)))
        rows = np.arange(res.offsets[e], res.offsets[e] + 16)
        ex = B.expert(e)
        for xin, w, want in ((x[res.f2n[rows]].astype(f64), ex.w13(fam), None), (res.act[rows].astype(f64), ex.w2(fam), res.y2[rows])):
            cols = np.sort(rng.permutation(w.shape[1])[:96])
            prod = (xin[:, :, None] * w[None, :, cols]).astype(f32)
            assert np.array_equal(prod.astype(f64), xin[:, :, None] * w[None, :, cols])
            exact = xin @ w[:, cols]
            for trial in range(12):
                order = rng.permutation(w.shape[0]) if trial else np.arange(w.shape[0])
                acc = np.cumsum(prod[:, order], axis=1, dtype=f32)[:, -1]
                assert np.array_equal(acc.astype(f64), exact), (fam, trial)
            if want is not None:
                assert np.array_equal(exact.astype(f16).view(np.uint16), want[:, cols].view(np.uint16))
    Es, ks, ss = SHARED_CONFIG
    B = r.Block(H, I, Es, ks, ss)
    x, ids = r.make_x(B, 37, 'random')
    shared = r.make_shared(B, 37)
    for sh in (None, shared):
        res = r.forward(B, 'w', x, ids, shared=sh)
        for rot in range(ks):
            acc = np.zeros((37, H), f32) if sh is None else (sh.astype(f32) * r.sigma_of(x).astype(f32)[:, None])
            for j in np.roll(np.arange(ks), rot):
                acc = (f32(B.w) * res.y2[res.en2f[j]].astype(f32) + acc).astype(f32)     # each fma is exact: so is its float32 restatement
            assert np.array_equal(r.bits(acc.astype(f16)), r.bits(res.out))


@pytest.mark.parametrize('fmt', ['u4', 'f16', 'fp8'])
def test_expectation_equals_the_oracle_moe_ffn(fmt):
    """o.moe_ffn on the dequantised operands (o.w4a16_dequant, the fp16 weights, o.fp8_dequant of the gated form), token by token,
    at the smallest geometry with both 8-expert configurations"""
    H, I = r.GEOMETRIES[1]
    for E, k, s in r.CONFIGS[:2]:
        B = r.Block(H, I, E, k, s)
        x, ids = r.make_x(B, 37, 'random')
        res = r.forward(B, r.family(fmt), x, ids)
        dense = [B.expert(e).dequantised(fmt) for e in range(E)]
        for e in range(E):
            assert np.array_equal(dense[e][0].astype(f64), B.expert(e).w13(r.family(fmt)))
            assert np.array_equal(dense[e][1].astype(f64), B.expert(e).w2(r.family(fmt)))
        out, oids, ow = o.moe_ffn(x.astype(f16), B.gate(), dense, k, True, s)
        assert np.array_equal(oids, ids) and np.array_equal(ow, res.w)
        assert np.array_equal(r.bits(out), r.bits(res.out))
    ex = B.expert(0)
    p13, s13, z13, p2, s2, z2 = ex.operands('u4')
    assert np.array_equal(o.unpack_u4_row(p13), ex.a.q) and np.array_equal(o.unpack_u4_row(p2), ex.b.q)
    assert not np.array_equal(B.expert(0).w13('w'), B.expert(1).w13('w'))


@pytest.mark.parametrize('H,I,E,k,s', BLOCKS, ids=IDS)
def test_every_fault_changes_an_output_bit(H, I, E, k, s):
    """T = 37 with the edge routing (above 8 experts: with the routing that leaves most experts empty, which keeps this test
    short); token 0 gets one more expert at the top logit, above its picks (the router must leave it out).
    routed_scale dropped is a fault only where routed_scale != 1; the shared expert's faults belong to the block that has one; w2
    has two groups' scales to swap only at I = 384"""
    B = r.Block(H, I, E, k, s)
    has_shared = (E, k, s) == SHARED_CONFIG
    x, ids = r.make_x(B, 37, 'edge' if E == 8 else 'one')
    extra = max(e for e in range(E) if e not in ids[0])
    assert extra > ids[0].max()
    x[0, extra] = r.LOGIT_TOP
    r.check_routing(B, x, ids)
    shared = r.make_shared(B, 37) if has_shared else None
    for fam in r.FAMILIES:
        base = r.forward(B, fam, x, ids, shared=shared)
        for mut in r.MUTATIONS:
            if (mut == 'no_scale' and s == 1.0) or (mut in ('no_shared', 'shared_sigma0') and not has_shared) \
                    or (mut == 'swap2' and I == 128):
                continue
            got = r.forward(B, fam, x, ids, shared=shared, mut=mut)
            assert not np.array_equal(r.bits(got.out), r.bits(base.out)), f'{fam} {mut}: the expected bits do not notice'
            if mut == 'tie_high':
                assert not np.array_equal(got.ids, ids)


@pytest.mark.parametrize('E', [8, 64, 65, 72, 128, 256])
def test_boundary_pattern(E):
    """the k-th and (k+1)-th logits tie in every token; o.moe_gate returns the intended ids (lower id first); above 64 experts the
    tie groups include one lane's experts in different 64-expert strides and pairs whose lower id sits in the higher lane"""
    for k in (1, 2, 4, 8):
        if k >= E:
            continue
        x, ids = r.boundary_x(E, k, 97, 384)
        lg = x[:, :E]
        kth = np.take_along_axis(lg, ids[:, -1:].astype(np.int64), axis=1)[:, 0]
        assert all((lg[t] == kth[t]).sum() >= 2 and (lg[t] > kth[t]).sum() < k < (lg[t] >= kth[t]).sum() for t in range(97))
        gate = np.zeros((384, E), f16)
        gate[:E] = np.eye(E, dtype=f16)
        olg, oids, _ = o.moe_gate(x.astype(f16), gate, k)
        assert np.array_equal(olg, lg.astype(f32)) and np.array_equal(oids, ids)
        if E > 64:
            tied = [np.flatnonzero(lg[t] == kth[t]) for t in range(97)]
            assert any(len(set(g % 64)) == 1 and len(g) > 1 for g in tied), 'no tie inside one lane'
            assert any(len(g) == 2 and g[0] % 64 > g[1] % 64 for g in tied), 'no tie with the lower id in the higher lane'
