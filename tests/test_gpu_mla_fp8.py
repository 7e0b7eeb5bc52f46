"""GPU tests of MLA on the FP8 latent cache (csrc/attention_mla_fp8.hip; the store arm of csrc/attention_mla.hip): 640-byte rows of 512
e4m3fn codes + 64 fp16 k_pe.  Store and flatten are compared byte for byte with tests/fp8_kv_reference.py; attention with the float64
softmax over the dequantised codes under the project's attention bound |a - b| <= 1e-2 |b| + 2e-3 (the quantisation error is on both
sides); end to end the HIP path may take twice the error of a torch-only fp16 path that quantises the latent identically."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi, mla
from oracle import tm_oracle as o
from tests.fp8_kv_reference import dequantise, quantise, view
from tests.gpu_helpers import DevCache, dev, host, rope_table, st
from tests.test_gpu_mla_attention import CASES, _cu, _err_units, _idx, _norm, _rope64, _tables

pytestmark = pytest.mark.gpu
f16, f64 = np.float16, np.float64
RANK, ROPE, ROW, ROWB = 512, 64, 576, 640
LAYERS, LAYER = 2, 1
SCALE = 192 ** -0.5


def _layout(bits):
    rb = mla.row_bytes(bits)
    return SimpleNamespace(kv_heads=1, head_dim=ROW, block_len=64, bits=bits, layer_size=64 * rb, block_size=LAYERS * 64 * rb)


F8, F16 = _layout(_ffi.KV_BITS_FP8), _layout(16)


def _lay(pool, rb=ROWB):
    """view [blocks, 64, row bytes] uint8 of LAYER in a host pool [blocks, block_size] uint8"""
    return pool.reshape(len(pool), LAYERS, 64, rb)[:, LAYER]


def test_store(tm, cuda):
    """the existing store test's rows on both views; k_scale 0.0071 saturates the codes of |c| > 3.18"""
    rng = np.random.default_rng(7)
    H, qlen, hist, eps, max_pos, kvs, ks = 3, [3, 70], [0, 61], 1e-6, 128, ROW + 8, 0.0071
    klen = [h + n for h, n in zip(hist, qlen)]
    T, cu = sum(qlen), _cu(qlen)
    tables, nblk = _tables(rng, klen)
    kv_a = (rng.standard_normal((T, kvs)) * rng.choice([0.05, 1.0, 30.0], (T, 1))).astype(f16)
    w = (1.0 + 0.2 * rng.standard_normal(RANK)).astype(f16)
    q = rng.standard_normal((T, H, ROW)).astype(f16)
    cs = rope_table(tm, max_pos, o.RopeParam(ROPE, 10000.0))
    pools, qs = [], []
    for L in (F8, F16):
        dc = DevCache(L, nblk, tables)
        dc.pool.fill_(0xff)
        q_d = dev(q)
        _ffi.check(tm.tm_mla_kv_store(dev(kv_a).data_ptr(), kvs, dev(w).data_ptr(), eps, q_d.data_ptr(), H * ROW, H, dev(cu).data_ptr(),
                                      dev(np.asarray(klen, np.int32)).data_ptr(), 2, T, dev(cs).data_ptr(), max_pos,
                                      view(dc, LAYER, ks, 0.0), st()))
        pools.append(dc.download()), qs.append(host(q_d))
    want, saturated = np.full_like(pools[0], 0xff), 0
    for b in range(2):
        ix = _idx(tables[b], hist[b], klen[b])
        r16 = _lay(pools[1], ROW * 2)[ix]
        codes = quantise(r16[:, :RANK * 2].view(f16), ks)
        saturated += np.count_nonzero((codes & 0x7f) == 0x7e)
        _lay(want)[ix] = np.concatenate([codes, r16[:, RANK * 2:]], 1)
    assert saturated > 0, 'k_scale must exercise the clamp'
    assert np.array_equal(pools[0], want), f'{np.count_nonzero(pools[0] != want)} pool bytes differ'
    assert np.array_equal(qs[0].view(np.uint16), qs[1].view(np.uint16))


@functools.lru_cache(maxsize=None)
def _attention_case(H, case, ks=0.011):
    """(q, pool, tables, blocks, reference [rows, H * 512] float64); every cache byte the kernel must not read is 0xff"""
    qlen, hist = CASES[case]
    rng = np.random.default_rng(2000 * H + len(qlen))
    klen = [h + n for h, n in zip(hist, qlen)]
    tables, nblk = _tables(rng, klen)
    pool = np.full((nblk, F8.block_size), 0xff, np.uint8)
    q = (0.6 * rng.standard_normal((sum(qlen), H, ROW))).astype(f16)
    cu, ref = _cu(qlen), []
    for b, n in enumerate(klen):
        codes, pe = quantise(rng.standard_normal((n, RANK)).astype(f16), ks), rng.standard_normal((n, ROPE)).astype(f16)
        _lay(pool)[_idx(tables[b], 0, n)] = np.concatenate([codes, pe.view(np.uint8)], 1)
        c = dequantise(codes, ks, f64)
        s = np.einsum('jhd,td->jht', q[cu[b]:cu[b + 1]].astype(f64), np.concatenate([c, pe.astype(f64)], 1)) * SCALE
        seen = np.arange(n)[None, :] < hist[b] + np.arange(qlen[b])[:, None] + 1
        s = np.where(seen[:, None, :], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref.append(np.einsum('jht,td->jhd', p / p.sum(-1, keepdims=True), c).reshape(qlen[b], -1))
    return q, pool, tables, nblk, np.concatenate(ref), ks


@pytest.mark.parametrize('splits', [1, 2, 4])
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('H', [1, 16, 24])
def test_attention(tm, cuda, H, case, splits):
    """the fp16 test's cases (the tile is 64 tokens here too): decode at contexts 1 / 64 / 65, verify rows over five blocks, a 70-row
    chunk; ragged and rectangular tables; canary row behind the output"""
    qlen, hist = CASES[case]
    q, pool, tables, nblk, ref, ks = _attention_case(H, case)
    klen = np.asarray([h + n for h, n in zip(hist, qlen)], np.int32)
    rows = sum(qlen)
    dc = DevCache(F8, nblk, tables)
    dc.pool.copy_(torch.from_numpy(pool).cuda())
    ws = torch.empty(max(1, tm.tm_mla_attention_workspace(rows, H, splits)), dtype=torch.uint8, device='cuda')
    q_d, cu_d, kl_d = dev(q), dev(_cu(qlen)), dev(klen)
    stride = max(len(t) for t in tables) + 1
    try:
        for mode in (0, stride):
            dc.set_tables(tables, mode)
            _ffi.check(tm.tm_debug_set_block_stride(mode))
            out = torch.full((rows + 1, H * RANK), 7.0, dtype=torch.float16, device='cuda')
            _ffi.check(tm.tm_mla_attention(out.data_ptr(), q_d.data_ptr(), H * ROW, cu_d.data_ptr(), kl_d.data_ptr(), len(qlen), H, SCALE,
                                           splits, ws.data_ptr(), view(dc, LAYER, ks, 0.0), st()))
            got = host(out).astype(f64)
            assert (got[rows] == 7.0).all(), 'wrote past the last row'
            err = np.abs(got[:rows] - ref)
            print(f'H {H} {case} splits {splits} stride {mode}: max err {np.nanmax(err):.2e} max |ref| {np.abs(ref).max():.2f}')
            assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'stride {mode}: max err {np.nanmax(err)}, {np.isnan(got).sum()} NaN'
    finally:
        tm.tm_debug_set_block_stride(0)


def test_flatten(tm, cuda):
    rng = np.random.default_rng(11)
    klen, ks = [70, 5], 0.013
    tables, nblk = _tables(rng, klen)
    pool = np.full((nblk, F8.block_size), 0xff, np.uint8)
    for b, n in enumerate(klen):   # codes up to the clamp; the fp16 tail is copied as bytes
        _lay(pool)[_idx(tables[b], 0, n)] = np.concatenate([quantise((2 * rng.standard_normal((n, RANK))).astype(f16), ks),
                                                            rng.integers(0, 256, (n, ROPE * 2), dtype=np.uint8)], 1)
    dc = DevCache(F8, nblk, tables)
    dc.pool.copy_(torch.from_numpy(pool).cuda())
    off = np.asarray([3, 80], np.int32)
    out = torch.full((90, ROW), 7.0, dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_mla_flatten(out.data_ptr(), dev(off).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), 2, 70,
                                 view(dc, LAYER, ks, 0.0), st()))
    got, want = host(out).view(np.uint16), np.full((90, ROW), 7.0, f16)
    for b, n in enumerate(klen):
        rows = _lay(pool)[_idx(tables[b], 0, n)]
        want[off[b]:off[b] + n, :RANK] = dequantise(rows[:, :RANK], ks, f16)
        want[off[b]:off[b] + n, RANK:] = rows[:, RANK:].view(f16)
    assert np.array_equal(got, want.view(np.uint16))


@pytest.mark.parametrize('form,H', [('absorbed', 16), ('expanded', 2)])
def test_forward_end_to_end(tm, cuda, form, H):
    """mla.mla_forward on the FP8 view against the NON-absorbed float64 MLA (no quantisation in the reference), q_len (3, 66).
    Measured on one MI355X, in units of the attention bound: see DESIGN.md 7.19."""
    rng = np.random.default_rng(3)
    nope, vd, qlen, eps, max_pos, ks = 128, 128, [3, 66], 1e-6, 128, 0.0123
    T, cu = sum(qlen), _cu(qlen)
    wkvb = (rng.standard_normal((H * (nope + vd), RANK)) / np.sqrt(RANK)).astype(f16)
    q_nope = (0.6 * rng.standard_normal((T, H, nope))).astype(f16)
    q_pe = (0.6 * rng.standard_normal((T, H, ROPE))).astype(f16)
    kv_a = rng.standard_normal((T, ROW)).astype(f16)
    w = (1.0 + 0.1 * rng.standard_normal(RANK)).astype(f16)
    cs = rope_table(tm, max_pos, o.RopeParam(ROPE, 10000.0))

    def rot(x, pos):            # float64, no rounding
        c, s = cs[pos, :, 0].astype(f64)[:, None], cs[pos, :, 1].astype(f64)[:, None]
        y = np.empty(x.shape, f64)
        y[..., 0::2], y[..., 1::2] = c * x[..., 0::2] - s * x[..., 1::2], c * x[..., 1::2] + s * x[..., 0::2]
        return y

    tables, nblk = _tables(rng, qlen)
    dc = DevCache(F8, nblk, tables)
    W_UK, W_UV = mla.absorb(dev(wkvb), H, nope, vd)
    got = host(mla.mla_forward(dev(q_nope), dev(q_pe), dev(kv_a), dev(w), W_UK, W_UV, view(dc, LAYER, ks, 0.0), dev(cu),
                               dev(np.asarray(qlen, np.int32)), SCALE, dev(cs), eps, splits=2, form=form))
    ref, t16 = np.empty((T, H, vd), f64), torch.empty((T, H, vd), dtype=torch.float16, device='cuda')
    q_lat = torch.einsum('thd,hdr->thr', dev(q_nope), W_UK)
    for b, n in enumerate(qlen):
        r, pos = slice(cu[b], cu[b + 1]), np.arange(n)
        tril = np.tril(np.ones((n, n), bool))[:, None, :]
        kv = (_norm(kv_a[r, :RANK], w, eps, rounded=False) @ wkvb.astype(f64).T).reshape(n, H, nope + vd)
        k = np.concatenate([kv[..., :nope], np.broadcast_to(rot(kv_a[r, None, RANK:].astype(f64), pos), (n, H, ROPE))], -1)
        qq = np.concatenate([q_nope[r].astype(f64), rot(q_pe[r].astype(f64), pos)], -1)
        s = np.where(tril, np.einsum('jhd,thd->jht', qq, k) * SCALE, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref[r] = np.einsum('jht,thd->jhd', p / p.sum(-1, keepdims=True), kv[..., nope:])
        # the absorbed path with torch alone, every intermediate fp16, the latent through the same codes
        c = dev(dequantise(quantise(_norm(kv_a[r, :RANK], w, eps), ks), ks, f16))
        rows = torch.cat([c, dev(_rope64(kv_a[r, RANK:], cs, pos))], 1)
        qf = torch.cat([q_lat[r], dev(_rope64(q_pe[r], cs, pos))], 2)
        s = (torch.einsum('jhd,td->jht', qf, rows) * SCALE).masked_fill(~torch.from_numpy(tril).cuda(), float('-inf'))
        t16[r] = torch.einsum('jhr,hrv->jhv', torch.einsum('jht,tr->jhr', torch.softmax(s, -1), c), W_UV)
    e_t, e_h = _err_units(host(t16), ref), _err_units(got, ref)
    print(f'{form} H {H}, units of the attention bound: fp16 torch on dequantised codes {e_t:.3f}, HIP {e_h:.3f}')
    assert e_h <= 2 * e_t


def test_refusals(tm, cuda):
    buf = torch.zeros(4096, dtype=torch.float16, device='cuda')
    two, cu = dev(np.asarray([2], np.int32)), dev(np.asarray([0, 2], np.int32))
    dc = DevCache(F8, 1, [[0]])
    calls = (lambda c: tm.tm_mla_attention(buf.data_ptr(), buf.data_ptr(), ROW, cu.data_ptr(), two.data_ptr(), 1, 1, SCALE, 1, None, c, st()),
             lambda c: tm.tm_mla_kv_store(buf.data_ptr(), ROW, buf.data_ptr(), 1e-6, buf.data_ptr(), ROW, 1, cu.data_ptr(), two.data_ptr(), 1,
                                          2, None, 0, c, st()),
             lambda c: tm.tm_mla_flatten(buf.data_ptr(), cu.data_ptr(), two.data_ptr(), 1, 2, c, st()))
    for call in calls:
        c8 = dc.view(0)
        c8.bits = 8
        assert call(c8) == 1 and 'bits 16' in _ffi.last_error(), _ffi.last_error()
        for bad in (-1.0, float('nan'), float('inf')):
            assert call(view(dc, 0, bad, 0.0)) == 1 and 'k_scale' in _ffi.last_error(), (bad, _ffi.last_error())
        assert call(view(dc, 0, 0.0, 0.0)) == 0      # 0 means 1.0
    assert tm.tm_mla_layer_size_fp8(64, 512, 64) == 40960 == F8.layer_size
    assert [tm.tm_mla_layer_size_fp8(*bad) for bad in ((64, 256, 64), (64, 512, 32), (32, 512, 64))] == [-1] * 3
