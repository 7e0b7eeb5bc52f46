"""GPU parity tests of the small row kernels every forward passes through -- RMSNorm, greedy argmax, embedding lookup,
unfused SiLU * up, and flatten_kv feeding prefill attention -- at the sizes where they take another path: rows that are no
multiple of the vector / wave / workgroup width, a second trip of a strided loop, padded leading dimensions, the ends of the
fp16 range, and a scratch that still holds somebody else's bytes.

Expected values come from oracle.tm_oracle or from a few lines of numpy here, never from a second run of a kernel.
Bounds: integer / index / copied outputs bit exact; norms <= 1 fp16 ulp on < 0.1 % of the elements (reachable for these very
inputs: tests/test_host.py::test_rmsnorm_edge_inputs_meet_the_one_ulp_cap_in_kernel_order); attention
|a-b| <= 1e-2*|b| + 2e-3 (tests/test_gpu_ops.py); SiLU <= 1 fp16 ulp.
"""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import row_ops_reference as rr
from tests.gpu_helpers import DevCache, dev, host, st, ulp_diff_f16

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
NAN16 = 0x7e00          # fp16 quiet NaN


def _poisoned(shape):
    """device fp16 tensor with every element NaN"""
    return torch.full(shape, NAN16, dtype=torch.int16, device='cuda').view(torch.float16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ------------------------------------------------------------------------------------------------
# flatten_kv -> prefill attention through a scratch that is never cleared
# ------------------------------------------------------------------------------------------------
def _paged_cache(rng, L, klen, layer):
    """oracle cache with klen[b] random tokens per sequence in shuffled blocks + its device copy"""
    nblk = [(k + 63) // 64 for k in klen]
    total = sum(nblk) + 2
    perm = rng.permutation(total)
    tables = [perm[sum(nblk[:b]):sum(nblk[:b + 1])] for b in range(len(klen))]
    oc = o.PagedKVCache(L, total)
    for b, n in enumerate(klen):
        k = rng.standard_normal((n, L.kv_heads, 128)).astype(f16)
        v = rng.standard_normal((n, L.kv_heads, 128)).astype(f16)
        o.process_kv(oc, tables[b], layer, k, v, None, None, 0)
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    return oc, dc, tables


def _flatten_prefill(tm, kf, vf, koff, stride, dc, layer, q, qlens, klen, Hq, Hkv):
    """tm_flatten_kv(transpose_v=1) into (kf, vf), then tm_prefill_attention over that scratch -> out [T, Hq * 128]"""
    cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    koff_d, klen_d = dev(np.asarray(koff, np.int32)), dev(np.asarray(klen, np.int32))
    _ffi.check(tm.tm_flatten_kv(kf.data_ptr(), vf.data_ptr(), 1, koff_d.data_ptr(), klen_d.data_ptr(), len(klen), max(klen),
                                stride, dc.view(layer), st()))
    out = torch.zeros((len(q), Hq * 128), dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_prefill_attention(out.data_ptr(), dev(q).data_ptr(), Hq * 128, kf.data_ptr(), vf.data_ptr(), stride,
                                       dev(cu).data_ptr(), koff_d.data_ptr(), klen_d.data_ptr(), len(klen), max(qlens), Hq, Hkv,
                                       0.0, st()))
    return host(out)


@pytest.mark.parametrize('bits', [16, 8, 4])
def test_flatten_then_prefill_from_poisoned_scratch(tm, cuda, bits):
    """The engine's path: paged (quantised) cache -> flatten_kv -> prefill attention, with the scratch full of NaN before
    the flatten.  klen % 64 is 6, 0, 0: the first sequence's last 64-key stage is mostly tail.  The V^T tail must come out
    zero (0 * NaN = NaN in the P V product), the K tail may stay NaN (its scores are masked)."""
    Hq, Hkv, layer = 8, 2, 1
    qlens, hist = [70, 5, 64], [0, 59, 64]
    klen = [h + n for h, n in zip(hist, qlens)]
    rng = np.random.default_rng(500 + bits)
    L = o.BlockLayout(2, Hkv, 128, 64, bits)
    oc, dc, tables = _paged_cache(rng, L, klen, layer)
    koff = np.concatenate([[0], np.cumsum([(k + 63) // 64 * 64 for k in klen])]).astype(np.int32)
    stride = int(koff[-1])
    q = rng.standard_normal((sum(qlens), Hq * 128)).astype(f16)
    got = _flatten_prefill(tm, _poisoned((Hkv, stride, 128)), _poisoned((Hkv, 128, stride)), koff[:-1], stride, dc, layer, q,
                           qlens, klen, Hq, Hkv)
    assert np.isfinite(got).all(), f'{np.count_nonzero(~np.isfinite(got))} non-finite outputs: the scratch poison leaked'
    cu = np.concatenate([[0], np.cumsum(qlens)])
    for b, n in enumerate(qlens):
        K, V = o.flatten_kv(oc, tables[b], layer, klen[b])
        ref = o.prefill_attention(q[cu[b]:cu[b + 1]].reshape(n, Hq, 128), K, V, hist[b]).reshape(n, -1).astype(f32)
        err = np.abs(got[cu[b]:cu[b + 1]].astype(f32) - ref)
        print(f'bits {bits} seq {b}: max err {err.max():.3e}')
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'seq {b}: max err {err.max()}'


def test_flatten_prefill_scratch_reuse(tm, cuda):
    """A chunk with klen = [200, 130] goes through the scratch, then -- without clearing it -- a chunk with klen = [70, 5] at
    the same offsets: everything the second chunk's attention reads must have been rewritten by the second flatten.  Its
    output is bit-identical to the same two calls on a freshly poisoned scratch."""
    Hq, Hkv, layer, bits = 8, 2, 0, 8
    rng = np.random.default_rng(77)
    L = o.BlockLayout(1, Hkv, 128, 64, bits)
    koff, stride = [0, 256], 448
    first, second = [200, 130], [70, 5]
    _, dc1, _ = _paged_cache(rng, L, first, layer)
    _, dc2, _ = _paged_cache(rng, L, second, layer)
    q1 = rng.standard_normal((sum(first), Hq * 128)).astype(f16)
    q2 = rng.standard_normal((sum(second), Hq * 128)).astype(f16)
    kf, vf = _poisoned((Hkv, stride, 128)), _poisoned((Hkv, 128, stride))
    out1 = _flatten_prefill(tm, kf, vf, koff, stride, dc1, layer, q1, first, first, Hq, Hkv)
    reused = _flatten_prefill(tm, kf, vf, koff, stride, dc2, layer, q2, second, second, Hq, Hkv)
    fresh = _flatten_prefill(tm, _poisoned((Hkv, stride, 128)), _poisoned((Hkv, 128, stride)), koff, stride, dc2, layer, q2,
                             second, second, Hq, Hkv)
    assert np.isfinite(out1).all() and np.isfinite(fresh).all()
    assert np.array_equal(_bits(reused), _bits(fresh)), 'the second chunk read bytes the first one left in the scratch'


# ------------------------------------------------------------------------------------------------
# greedy argmax
# ------------------------------------------------------------------------------------------------
def _argmax_rows(rng, V):
    """8 rows [8, V] fp16.  tail0 = first index of the scalar tail loop (V % 8 entries); the vector loop covers [0, tail0)."""
    tail0 = V // 8 * 8
    ninf = f16(-np.inf)
    x = rng.standard_normal((8, V)).astype(f16)
    # row 0: random
    # row 1: tie between a vector-part index and a tail index (thread 0 owns both); without one of the two parts, two far ends
    a, b = (3, tail0) if 0 < tail0 < V else (1, V - 1)
    x[1, a] = x[1, b] = f16(30.0)
    # row 2: tie between two tail indices (without a tail: two entries of the last vector)
    a, b = (tail0, V - 1) if V - tail0 >= 2 else (V - 6, V - 2)
    x[2, a] = x[2, b] = f16(30.0)
    x[3, V - 1] = f16(30.0)                      # row 3: maximum at the last index
    x[4, 0] = f16(30.0)                          # row 4: maximum at index 0
    x[5] = ninf                                  # row 5: nothing above -inf
    x[6] = ninf                                  # row 6: NaN and -inf only, index 0 and the last index are -inf
    x[6, 1::3] = f16(np.nan)
    x[6, V - 1] = ninf
    nan_at = rng.random(V) < 0.3                 # row 7: NaN scattered among ordinary values, also at both ends and on
    top = V // 2                                 # either side of the maximum
    nan_at[[0, V - 1, top - 1, top + 1]] = True
    nan_at[top] = False
    x[7, nan_at] = f16(np.nan)
    x[7, top] = f16(25.0)
    return x


@pytest.mark.parametrize('V,ld', [(7, 8), (8, 8), (1003, 1008), (4099, 4104), (8200, 8200), (8207, 8208), (151936, 152064)])
def test_argmax_edges(tm, cuda, V, ld):
    """Contract of tm_argmax (argmax_kernel, misc.hip):
      * NaN never wins;
      * the result is the LOWEST index of the maximum over the remaining entries, wherever the tie partners sit (vector
        part, scalar tail V % 8, another thread, another trip of a thread: V = 8200 is 1025 vectors on 1024 threads);
      * a row with no entry above -inf (all -inf, or -inf and NaN) gives id 0 and value -inf;
      * columns [V, ld) are never read (they hold 100.0 here);
      * out_val is the winning logit, bit for bit.
    Expectation in numpy: NaN -> -inf, then argmax (first occurrence)."""
    rng = np.random.default_rng(V)
    x = _argmax_rows(rng, V)
    buf = np.full((8, ld), 100.0, f16)
    buf[:, :V] = x
    clean = np.where(np.isnan(x), f16(-np.inf), x)
    want_id = clean.astype(f32).argmax(-1).astype(np.int32)
    want_val = clean[np.arange(8), want_id]
    ids = torch.full((8,), -7, dtype=torch.int32, device='cuda')
    val = _poisoned((8,))
    _ffi.check(tm.tm_argmax(ids.data_ptr(), val.data_ptr(), dev(buf).data_ptr(), 8, V, ld, st()))
    got_id, got_val = host(ids), host(val)
    print(f'V {V}: ids {got_id.tolist()} want {want_id.tolist()} val bits {[hex(v) for v in _bits(got_val)]}')
    assert np.array_equal(got_id, want_id), f'ids {got_id.tolist()} != {want_id.tolist()}'
    assert np.array_equal(_bits(got_val), _bits(want_val)), f'values {got_val.tolist()} != {want_val.tolist()}'


# ------------------------------------------------------------------------------------------------
# RMSNorm / residual RMSNorm
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps', rr.NORM_EPS)
@pytest.mark.parametrize('H', rr.NORM_H)
def test_rmsnorm_edges(tm, cuda, H, eps):
    """H / 8 vectors on workgroups of whole waves: 8 -> 1 vector, 63 idle lanes; 896 -> 112 vectors, the second wave partly
    past the row; 1000 -> 125; 3584 -> 448 = 7 waves; 5120 -> 640 vectors on 512 threads, the second vector of a thread
    covers two of eight waves.  Rows scaled by 2**-12 .. 2**10 (eps dominates the small ones: 1e-5 and 1e-6 give different
    y) and one all-zero row, whose y is exactly zero."""
    x, w, zero_row = rr.rmsnorm_inputs(H)
    M = len(x)
    y = _poisoned((M + 1, H))                    # one canary row behind the output
    _ffi.check(tm.tm_rmsnorm(y.data_ptr(), dev(x).data_ptr(), dev(w).data_ptr(), eps, M, H, st()))
    got = host(y)
    assert (_bits(got[M]) == NAN16).all(), 'wrote past the last row'
    d = ulp_diff_f16(got[:M], o.rmsnorm(x, w, eps))
    print(f'H {H} eps {eps}: M {M} max ulp {d.max()} off {np.count_nonzero(d)} / {d.size}')
    assert np.isfinite(got[:M]).all()
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    assert not got[zero_row].any(), 'an all-zero row must give exactly zero'
    # the kernel's own summation order, restated on the host, is what the device computes: bit for bit
    assert np.array_equal(_bits(got[:M]), _bits(rr.rmsnorm_kernel_order(x, w, eps)))


@pytest.mark.parametrize('M,H,splits,bias', rr.RESIDUAL_CASES)
def test_residual_rmsnorm_edges(tm, cuda, M, H, splits, bias):
    """splits 1 and 2: the four unconditional slab loads clamp to the last slab; 5 and 8: the loop behind the first four;
    0: the fp16 hidden form.  Residual stream bit exact, y within the norm bound."""
    r, hcur, part, b, w = rr.residual_inputs(M, H, splits, bias)
    r_d = dev(np.concatenate([r, np.full((1, H), np.nan, f16)]))       # canary rows behind both outputs
    y = _poisoned((M + 1, H))
    _ffi.check(tm.tm_residual_rmsnorm(y.data_ptr(), r_d.data_ptr(), None if splits else dev(hcur).data_ptr(),
                                      dev(part).data_ptr() if splits else None, splits,
                                      dev(b).data_ptr() if bias else None, dev(w).data_ptr(), 1e-5, M, H, st()))
    r_ref, y_ref = o.residual_rmsnorm(r, rr.sum_partials(part) if splits else hcur, w, 1e-5, b)
    got_r, got_y = host(r_d), host(y)
    assert np.isnan(got_r[M]).all() and (_bits(got_y[M]) == NAN16).all(), 'wrote past the last row'
    assert np.array_equal(_bits(got_r[:M]), _bits(r_ref)), 'residual stream must be bit exact'
    d = ulp_diff_f16(got_y[:M], y_ref)
    print(f'M {M} H {H} splits {splits}: max ulp {d.max()} off {np.count_nonzero(d)} / {d.size}')
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    assert np.array_equal(_bits(got_y[:M]), _bits(rr.rmsnorm_kernel_order(r_ref, w, 1e-5)))


def test_residual_rmsnorm_zero_rows_is_a_noop(tm, cuda):
    """(M, H, splits) = (0, 4096, 0): returns 0 and launches nothing -- residual and y keep their canaries"""
    H = 4096
    canary = np.full((2, H), 1.5, f16)
    r_d, y_d, h_d = dev(canary), dev(canary), dev(np.full((2, H), 2.0, f16))
    rc = tm.tm_residual_rmsnorm(y_d.data_ptr(), r_d.data_ptr(), h_d.data_ptr(), None, 0, None, dev(np.ones(H, f16)).data_ptr(),
                                1e-5, 0, H, st())
    assert rc == 0
    assert np.array_equal(host(r_d), canary) and np.array_equal(host(y_d), canary)


# ------------------------------------------------------------------------------------------------
# embedding lookup, SiLU * up
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [8, 2048, 4104])
def test_embedding_edges(tm, cuda, H):
    """H / 8 vectors on 256 threads: 1 (255 idle threads), 256 (exactly one trip), 513 (a third trip of one thread).
    An id outside [0, vocab) is clamped to the nearest row -- this project's own contract (the reference indexes the table
    with whatever it is given); a wrong id must not read outside the table."""
    vocab = 50
    rng = np.random.default_rng(H)
    table = rng.standard_normal((vocab, H)).astype(f16)
    ids = np.concatenate([[-1, -2**31, vocab, 2**31 - 1, 0, vocab - 1], rng.integers(0, vocab, 7)]).astype(np.int32)
    T = len(ids)
    out = _poisoned((T + 1, H))
    _ffi.check(tm.tm_embedding(out.data_ptr(), dev(table).data_ptr(), dev(ids).data_ptr(), T, H, vocab, st()))
    got = host(out)
    assert (_bits(got[T]) == NAN16).all(), 'wrote past the last row'
    assert np.array_equal(_bits(got[:T]), _bits(table[np.clip(ids, 0, vocab - 1)]))


SILU_GATES = (65504.0, 20.0, 11.09, 2.0**-14, 6e-8, 0.0)      # each with both signs; 6e-8 -> the smallest fp16 subnormal


def _silu_inputs(rng, M, inter):
    """gate_up tensors [M, 2 * inter] ([gate | up]), as many as it takes for every special gate value to meet an up value of
    +65504, -65504 and two N(0, 1); the rest is gate ~ N(0, 3), up ~ N(0, 1) with a few +-65504"""
    g_sp = np.asarray([s * v for v in SILU_GATES for s in (1.0, -1.0)], f32).astype(f16)
    pairs_g = np.repeat(g_sp, 4)
    pairs_u = np.tile(np.asarray([65504.0, -65504.0, 0.0, 0.0], f32), len(g_sp)).astype(f16)
    rnd = np.tile(np.asarray([False, False, True, True]), len(g_sp))
    pairs_u[rnd] = rng.standard_normal(rnd.sum()).astype(f16)
    n = M * inter
    count = -(-(len(pairs_g) + 8) // n)          # at least 8 random pairs besides the special ones
    g = (rng.standard_normal(count * n) * 3).astype(f16)
    u = rng.standard_normal(count * n).astype(f16)
    u[len(pairs_g) + 3::17] = f16(65504.0)
    u[len(pairs_g) + 4::23] = f16(-65504.0)
    g[:len(pairs_g)], u[:len(pairs_u)] = pairs_g, pairs_u
    return [np.concatenate([g[i * n:(i + 1) * n].reshape(M, inter), u[i * n:(i + 1) * n].reshape(M, inter)], 1)
            for i in range(count)]


@pytest.mark.parametrize('M,inter', [(1, 8), (3, 2056)])
def test_silu_mul_edges(tm, cuda, M, inter):
    """out = h(silu_f32(g) * f32(u)) at the ends of the fp16 range: exp(-g) overflows to inf for g = -65504 (silu = -0) and
    underflows to 0 for g = 65504 (silu = g, times +-65504 -> +-inf); g = +-11.09 has exp(|g|) at the fp16 maximum; 2**-14 and
    6e-8 are the smallest normal / subnormal.  One vector in all (1 x 8), and 3 x 257 vectors = 771 on workgroups of 256.
    Finite expectations within 1 ulp; where the oracle gives inf or NaN the kernel gives the same."""
    rng = np.random.default_rng(inter)
    for gu in _silu_inputs(rng, M, inter):
        y = _poisoned((M + 1, inter))
        _ffi.check(tm.tm_silu_mul(y.data_ptr(), dev(gu).data_ptr(), M, inter, st()))
        got = host(y)
        assert (_bits(got[M]) == NAN16).all(), 'wrote past the last row'
        got = got[:M]
        with np.errstate(over='ignore', invalid='ignore'):
            ref = o.silu_and_mul_unfused(gu)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
        d = ulp_diff_f16(got[fin], ref[fin])
        print(f'({M}, {inter}): {fin.sum()} finite, {np.isinf(ref).sum()} inf, {np.isnan(ref).sum()} nan, max ulp {d.max()}')
        assert d.max() <= 1
