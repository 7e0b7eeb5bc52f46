"""TurboQuant KV cache (quant_policy 42) on the GPU: store, flatten and decode attention through the C-ABI against the numpy
restatement of the contract (tests/turboquant_reference.py), and the refusals by name.

Codes are integers: they must be IDENTICAL wherever the reference does not report the element as ambiguous (a value within fp32
summation noise of a decision boundary); the fp16 norms may differ by one ulp.  Flatten: |gpu - ref| <= 2^-10 * max|ref row| (one fp16
rounding + fp32 butterfly-order noise <= 7 * 2^-24 * sum|row|).  Attention: the project's bound (tests/test_gpu_ops.py:4-10).
"""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import turboquant_reference as tq
from tests.gpu_helpers import DevCache, dev, host, rope_table, st, ulp_diff_f16

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
TM_INVALID = 1


def _tables(rng, klen, spare=2):
    nblk = [(k + 63) // 64 for k in klen]
    total = sum(nblk) + spare
    perm = rng.permutation(total)
    tables, off = [], 0
    for nb in nblk:
        tables.append(perm[off:off + nb])
        off += nb
    return tables, total


def _param_mask(L, layer):
    """bool [block_size]: the bytes of `layer` that hold fp16 norms"""
    m = np.zeros(L.block_size, bool)
    base = L.layer_offset(layer)
    for hd in range(L.kv_heads):
        for ti in range(L.block_len):
            for off in (L.k_param(hd, ti), L.v_param(hd, ti)):
                m[base + off: base + off + 4] = True
    return m


def _assert_pool(got, ref, L, layer, what=''):
    pm = _param_mask(L, layer)
    bad = got[:, ~pm] != ref[:, ~pm]
    assert not bad.any(), f'{what}: {np.count_nonzero(bad)} code / foreign bytes differ'
    ulp = ulp_diff_f16(got[:, pm].copy().view(f16), ref[:, pm].copy().view(f16))
    assert ulp.max() <= 1, f'{what}: norms differ by up to {ulp.max()} fp16 ulps'


def _exact_rows(rng, shape, is_k):
    """fp16 rows whose H f and sum f^2 are exact in fp32 in any order; rows with an ambiguous element are redrawn until none is left"""
    def draw(n):
        return np.clip(np.round(64 * rng.standard_normal((n, shape[-1]))) / 64, -3.5, 3.5).astype(f16)
    x = draw(int(np.prod(shape[:-1])))
    redrawn = 0
    while True:
        bad = tq.ambiguous_exact(tq.quantise(x, is_k)).any(-1)
        if not bad.any():
            break
        redrawn += int(bad.sum())
        x[bad] = draw(int(bad.sum()))
    return x.reshape(shape), redrawn


# ------------------------------------------------------------------------------------------------
def test_store_exact(tm, cuda):
    """every byte of the cache: three sequences in one call -- (history 0, 1 new), (0, 65), (61, 6 across a block boundary)"""
    rng = np.random.default_rng(42)
    Hq, Hkv, layer = 4, 2, 1
    hist, new = [0, 0, 61], [1, 65, 6]
    klen = [h + n for h, n in zip(hist, new)]
    L = tq.TqBlockLayout(2, Hkv)
    tables, total = _tables(rng, klen, spare=3)
    T = sum(new)
    k, rk = _exact_rows(rng, (T, Hkv, 128), True)
    v, rv = _exact_rows(rng, (T, Hkv, 128), False)
    v[7, 1] = 0                                                      # one all-zero V row: n = 0, +0 back, never NaN
    print(f'redrawn rows: K {rk}, V {rv} of {T * Hkv}')
    q = np.clip(np.round(64 * rng.standard_normal((T, Hq, 128))) / 64, -3.5, 3.5).astype(f16)
    qkv = np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1)
    oc = tq.TqPagedKVCache(L, total)
    oc.pool[:] = 0xa5                                                # poison: other blocks, the other layer, the rows not stored
    kh = rng.standard_normal((61, Hkv, 128)).astype(f16)
    vh = rng.standard_normal((61, Hkv, 128)).astype(f16)
    o.process_kv(oc, tables[2], layer, kh, vh, None, None, 0)        # the 61 earlier tokens: their bytes must stay
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    cu = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    for b in range(3):
        sl = slice(cu[b], cu[b + 1])
        o.process_kv(oc, tables[b], layer, k[sl], v[sl], None, None, hist[b])
    qkv_d = dev(qkv)
    _ffi.check(tm.tm_kv_rope_store(qkv_d.data_ptr(), Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), 3, T, None, 0,
                                   dc.view(layer), st()))
    _assert_pool(dc.download(), oc.pool, L, layer, 'store')
    # the zero row: zero norms on the device too
    blk = dc.download()[tables[1][0]]
    assert not blk[L.layer_offset(layer) + L.v_param(1, 7 - 1): L.layer_offset(layer) + L.v_param(1, 7 - 1) + 4].any()
    # q (and the rest of qkv) as the bits-16 call leaves it
    L16 = o.BlockLayout(2, Hkv, 128, 64, 16)
    dc16 = DevCache(L16, total, tables)
    qkv16 = dev(qkv)
    _ffi.check(tm.tm_kv_rope_store(qkv16.data_ptr(), Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), 3, T, None, 0,
                                   dc16.view(layer), st()))
    assert np.array_equal(host(qkv_d).view(np.uint16), host(qkv16).view(np.uint16))


def test_store_with_rope(tm, cuda):
    """K after RoPE: the GPU's own rotated K (from a bits-16 store of the same qkv) quantised by the reference"""
    rng = np.random.default_rng(7)
    Hq, Hkv, layer = 4, 2, 1
    hist, new = [0, 200], [70, 3]
    klen = [h + n for h, n in zip(hist, new)]
    tables, total = _tables(rng, klen)
    T = sum(new)
    qkv = (rng.standard_normal((T, (Hq + 2 * Hkv) * 128)) * 1.5).astype(f16)
    p = o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192)
    max_pos = max(klen) + 1
    tab_d = dev(rope_table(tm, max_pos, p))
    cu = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    args = (Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), 2, T, tab_d.data_ptr(), max_pos)
    L16 = o.BlockLayout(2, Hkv, 128, 64, 16)
    dc16 = DevCache(L16, total, tables)
    qkv16 = dev(qkv)
    _ffi.check(tm.tm_kv_rope_store(qkv16.data_ptr(), *args, dc16.view(layer), st()))
    oc16 = o.PagedKVCache(L16, total)
    oc16.pool[:] = dc16.download()
    L = tq.TqBlockLayout(2, Hkv)
    dc = DevCache(L, total, tables)
    qkv42 = dev(qkv)
    _ffi.check(tm.tm_kv_rope_store(qkv42.data_ptr(), *args, dc.view(layer), st()))
    assert np.array_equal(host(qkv42).view(np.uint16), host(qkv16).view(np.uint16)), 'q is rotated in place as the bits-16 call does'
    got = tq.TqPagedKVCache(L, total)
    got.pool[:] = dc.download()
    skipped = compared = 0
    for b in range(2):
        for hd in range(Hkv):
            k16, v16, _, _ = oc16.load_raw(tables[b], layer, hd, hist[b], klen[b])
            kc, vc, kp, vp = got.load_raw(tables[b], layer, hd, hist[b], klen[b])
            for x, codes, params, is_k in ((k16, kc, kp, True), (v16, vc, vp, False)):
                ref = tq.quantise(x, is_k)
                skip = tq.ambiguous_abs(ref, 2.0 ** -17 * np.abs(x.astype(f64)).sum(-1))
                skipped += int(skip.sum())
                compared += skip.size
                assert np.array_equal(codes[~skip], ref.codes[~skip]), f'seq {b} head {hd} {"K" if is_k else "V"}: codes differ'
                assert ulp_diff_f16(params, ref.params).max() <= 1
    print(f'skipped {skipped} of {compared} elements ({100 * skipped / compared:.3f} %)')
    assert skipped <= 0.005 * compared


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('transpose_v', [0, 1])
def test_flatten(tm, cuda, transpose_v):
    rng = np.random.default_rng(transpose_v)
    Hkv, layer = 2, 1
    klen = [1, 64, 65, 130]
    L = tq.TqBlockLayout(2, Hkv)
    tables, total = _tables(rng, klen)
    oc = tq.TqPagedKVCache(L, total)
    for b, n in enumerate(klen):
        k = rng.standard_normal((n, Hkv, 128)).astype(f16)
        v = rng.standard_normal((n, Hkv, 128)).astype(f16)
        o.process_kv(oc, tables[b], layer, k, v, None, None, 0)
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    pad = [((n + 63) // 64) * 64 for n in klen]
    koff = np.asarray([0, pad[0], pad[0] + pad[1] + 64, pad[0] + pad[1] + 64 + pad[2]], np.int32)   # one foreign region in between
    stride = int(koff[-1]) + pad[3] + 64                                                              # and one behind
    kl_d, koff_d = dev(np.asarray(klen, np.int32)), dev(koff)

    def scratch():
        kf = torch.full((Hkv, stride, 128), 0x7e00, dtype=torch.int16, device='cuda').view(torch.float16)
        vf = torch.full((Hkv, 128, stride) if transpose_v else (Hkv, stride, 128), 0x7e00, dtype=torch.int16,
                        device='cuda').view(torch.float16)
        return kf, vf
    kf, vf = scratch()
    _ffi.check(tm.tm_flatten_kv(kf.data_ptr(), vf.data_ptr(), transpose_v, koff_d.data_ptr(), kl_d.data_ptr(), len(klen), max(klen),
                                stride, dc.view(layer), st()))
    K, V = host(kf), host(vf)
    Vt = V.transpose(0, 2, 1) if transpose_v else V
    k_written = np.zeros(stride, bool)
    v_written = np.zeros(stride, bool)
    for b, n in enumerate(klen):
        for hd in range(Hkv):
            kc, vc, kp, vp = oc.load_raw(tables[b], layer, hd, 0, n)
            for got, ref in ((K[hd, koff[b]:koff[b] + n], tq.dequant_original(kc, kp, True)),
                             (Vt[hd, koff[b]:koff[b] + n], tq.dequant_original(vc, vp, False))):
                err = np.abs(got.astype(f64) - ref)
                bound = 2.0 ** -10 * np.abs(ref).max(-1, keepdims=True)
                assert (err <= bound).all(), f'seq {b} head {hd}: worst err / bound {np.max(err / bound):.3f}'
        if transpose_v:   # the tail up to the 64-token tile is zero-filled
            assert not Vt[:, koff[b] + n:koff[b] + pad[b]].view(np.uint16).any()
        k_written[koff[b]:koff[b] + n] = True
        v_written[koff[b]:koff[b] + (pad[b] if transpose_v else n)] = True
    assert (K[:, ~k_written].view(np.uint16) == 0x7e00).all(), 'K rows outside [0, klen) of a flattened sequence were written'
    assert (Vt[:, ~v_written].view(np.uint16) == 0x7e00).all(), 'V outside the flattened sequences\' regions was written'
    # tm_flatten_kv_window: window 0 is the same call, a window is refused by name
    kf2, vf2 = scratch()
    _ffi.check(tm.tm_flatten_kv_window(kf2.data_ptr(), vf2.data_ptr(), transpose_v, koff_d.data_ptr(), kl_d.data_ptr(), len(klen), max(klen),
                                       stride, dc.view(layer), None, 0, st()))
    assert np.array_equal(host(kf2).view(np.uint16), K.view(np.uint16)) and np.array_equal(host(vf2).view(np.uint16), V.view(np.uint16))
    cu_q = dev(np.arange(len(klen) + 1, dtype=np.int32))
    rc = tm.tm_flatten_kv_window(kf2.data_ptr(), vf2.data_ptr(), transpose_v, koff_d.data_ptr(), kl_d.data_ptr(), len(klen), max(klen),
                                 stride, dc.view(layer), cu_q.data_ptr(), 64, st())
    assert rc == TM_INVALID and 'window' in _ffi.last_error()


# ------------------------------------------------------------------------------------------------
def _fill(rng, L, klen, layer):
    tables, total = _tables(rng, klen)
    oc = tq.TqPagedKVCache(L, total)
    for b, n in enumerate(klen):
        k = rng.standard_normal((n, L.kv_heads, 128)).astype(f16)
        v = rng.standard_normal((n, L.kv_heads, 128)).astype(f16)
        if n > 40:
            k[n // 3] *= f16(6.0)     # forces the online-softmax rescale branch at a chosen tile (as _fill_cache(spike=True))
        o.process_kv(oc, tables[b], layer, k, v, None, None, 0)
    return oc, tables, total


def _decode(tm, dc, q_d, klen, Hq, splits, layer):
    B = len(klen)
    # poisoned, not zeroed: an output row or a split-K partial that is never written must not read as a plausible value
    out = torch.full((B, Hq * 128), 0x7e00, dtype=torch.int16, device='cuda').view(torch.float16)
    ws = torch.full((max(1, tm.tm_decode_attention_workspace(B, Hq, splits)),), 0xFF, dtype=torch.uint8, device='cuda')
    _ffi.check(tm.tm_decode_attention(out.data_ptr(), q_d.data_ptr(), Hq * 128, dev(np.asarray(klen, np.int32)).data_ptr(), B, Hq, 0.0,
                                      splits, ws.data_ptr(), dc.view(layer), st()))
    return host(out)


@pytest.mark.parametrize('Hq,Hkv,klen,splits', [(8, 2, [1, 64, 65, 300], 1), (8, 2, [1, 64, 65, 300], 3), (6, 1, [129, 5], 1),
                                                (32, 8, [257, 37], 2), (2, 2, [31], 1)])
def test_decode_attention(tm, cuda, Hq, Hkv, klen, splits):
    """the cache is written by the reference (no code can flip); against the unfused fp64 attention over the reference's
    original-domain rows"""
    rng = np.random.default_rng(Hq + sum(klen) + splits)
    layer = 1
    L = tq.TqBlockLayout(2, Hkv)
    oc, tables, total = _fill(rng, L, klen, layer)
    B = len(klen)
    q = rng.standard_normal((B, Hq * 128)).astype(f16)
    q_d = dev(q)
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    got = _decode(tm, dc, q_d, klen, Hq, splits, layer)
    worst = 0.0
    for b, n in enumerate(klen):
        Ks, Vs = zip(*[oc.load_dequant(tables[b], layer, hd, 0, n, 'decode') for hd in range(Hkv)])
        ref = o.attention_reference_unfused(q[b].reshape(Hq, 128), np.stack(Ks), np.stack(Vs))
        err = np.abs(got[b].reshape(Hq, 128).astype(f64) - ref)
        worst = max(worst, err.max())
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'seq {b}: max err {err.max()}'
        assert err.max() < 5e-3
    print(f'worst abs err {worst:.2e}')
    # rows of the last block past k_len hold 0xff bytes (NaN norms): finite and unchanged
    pool = oc.pool.copy()
    base = L.layer_offset(layer)
    for b, n in enumerate(klen):
        blk = pool[tables[b][-1]]
        for ti in range(n % 64 or 64, 64):
            for hd in range(Hkv):
                blk[base + L.k_data(hd, ti): base + L.k_data(hd, ti) + 64] = 0xff
                blk[base + L.v_data(hd, ti): base + L.v_data(hd, ti) + 32] = 0xff
                blk[base + L.k_param(hd, ti): base + L.k_param(hd, ti) + 4] = 0xff
                blk[base + L.v_param(hd, ti): base + L.v_param(hd, ti) + 4] = 0xff
    dc.pool.copy_(torch.from_numpy(pool).cuda())
    got2 = _decode(tm, dc, q_d, klen, Hq, splits, layer)
    assert np.isfinite(got2.astype(f32)).all()
    assert np.array_equal(got2.view(np.uint16), got.view(np.uint16)), 'bytes past k_len reached the output'
    # a permuted block table gives identical bytes
    perm = rng.permutation(total)
    pool3 = np.zeros_like(oc.pool)
    pool3[perm] = oc.pool
    dc3 = DevCache(L, total, [perm[t] for t in tables])
    dc3.pool.copy_(torch.from_numpy(pool3).cuda())
    got3 = _decode(tm, dc3, q_d, klen, Hq, splits, layer)
    assert np.array_equal(got3.view(np.uint16), got.view(np.uint16))


# ------------------------------------------------------------------------------------------------
def test_refusals(tm, cuda):
    """head_dim 64, the fused entry points, a window and sinks return TM_INVALID with bits 42, and the message names the limit"""
    Hq, Hkv = 4, 2
    buf = torch.zeros(1 << 16, dtype=torch.float16, device='cuda')
    pool = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    ptrs = torch.tensor([pool.data_ptr()], dtype=torch.int64, device='cuda')
    cu = dev(np.array([0, 1], np.int32))
    one = dev(np.array([1], np.int32))

    def view(D):
        return _ffi.KvCache(ptrs.data_ptr(), cu.data_ptr(), 0, Hkv, D, 64, 42)

    def refused(rc, *words):
        msg = _ffi.last_error()
        assert rc == TM_INVALID, (rc, msg)
        for w in words:
            assert w in msg, msg
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    # head_dim 64
    refused(tm.tm_kv_rope_store(buf.data_ptr(), Hq, cu.data_ptr(), one.data_ptr(), 1, 1, None, 0, view(64), st()), 'head_dim', '42')
    refused(tm.tm_flatten_kv(buf.data_ptr(), buf.data_ptr(), 0, cu.data_ptr(), one.data_ptr(), 1, 1, 64, view(64), st()), 'head_dim', '42')
    refused(tm.tm_decode_attention(buf.data_ptr(), buf.data_ptr(), Hq * 64, one.data_ptr(), 1, Hq, 0.0, 1, ws.data_ptr(), view(64), st()),
            'head_dim', '42')
    # the fused prologue
    qkv_n = (Hq + 2 * Hkv) * 128
    refused(tm.tm_decode_attention_fused(buf.data_ptr(), buf.data_ptr(), 0, qkv_n, None, 0, one.data_ptr(), 1, Hq, 0.0, 1, ws.data_ptr(),
                                         view(128), st()), 'fused', '42')
    refused(tm.tm_decode_attention_fused_qk(buf.data_ptr(), buf.data_ptr(), 0, qkv_n, None, 0, None, None, None, 0.0, one.data_ptr(), 1, Hq,
                                            0.0, 1, ws.data_ptr(), view(128), st()), 'fused', '42')
    # a window, sinks
    refused(tm.tm_decode_attention_window(buf.data_ptr(), buf.data_ptr(), Hq * 128, one.data_ptr(), 1, Hq, 0.0, 1, ws.data_ptr(), view(128),
                                          8, None, st()), 'window', '42')
    refused(tm.tm_decode_attention_window(buf.data_ptr(), buf.data_ptr(), Hq * 128, one.data_ptr(), 1, Hq, 0.0, 1, ws.data_ptr(), view(128),
                                          0, buf.data_ptr(), st()), 'sinks', '42')
    refused(tm.tm_flatten_kv_window(buf.data_ptr(), buf.data_ptr(), 0, cu.data_ptr(), one.data_ptr(), 1, 1, 64, view(128), cu.data_ptr(), 8,
                                    st()), 'window', '42')
