"""GPU tests of Multi-head Latent Attention on the paged latent cache (csrc/attention_mla.hip) against float64 numpy in this file.
Store: the norm bound of tests/test_gpu_row_ops.py, <= 1 fp16 ulp on < 0.1 % of the elements, against the float64 norm and rotation
rounded to fp16 where the contract rounds; every other pool byte keeps its fill.  Attention: |a - b| <= 1e-2 |b| + 2e-3
(tests/test_gpu_ops.py).  End to end: the HIP path may take twice the error of the fp16-torch-only absorbed path, in units of that bound."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi, mla
from oracle import tm_oracle as o
from tests.gpu_helpers import DevCache, dev, host, rope_table, st, ulp_diff_f16

pytestmark = pytest.mark.gpu
f16, f64 = np.float16, np.float64
RANK, ROPE, ROW = 512, 64, 576
LAYERS, LAYER = 2, 1
LAYOUT = SimpleNamespace(kv_heads=1, head_dim=ROW, block_len=64, bits=16, layer_size=64 * ROW * 2, block_size=LAYERS * 64 * ROW * 2)
SCALE = 192 ** -0.5                 # DeepSeek: 1 / sqrt(qk_nope 128 + qk_rope 64)
NAN16 = 0x7e00


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _tables(rng, klen, spare=2):
    """permuted block tables for contexts klen + `spare` blocks nobody owns"""
    nblk = [(k + 63) // 64 for k in klen]
    perm = rng.permutation(sum(nblk) + spare)
    return [perm[sum(nblk[:b]):sum(nblk[:b + 1])] for b in range(len(klen))], sum(nblk) + spare


def _lay(pool):
    """view [blocks, 64, 576] fp16 of LAYER in a host pool [blocks, block_size] uint8"""
    return pool.reshape(len(pool), LAYERS, 64, ROW * 2)[:, LAYER].view(f16)


def _idx(table, lo, hi):
    """(block, row) index arrays of a sequence's cache rows lo .. hi - 1"""
    return np.asarray(table)[np.arange(lo, hi) // 64], np.arange(lo, hi) % 64


def _rope64(x, cs, pos):
    """float64 rotation of pairs (2i, 2i + 1) by table row pos, each product and sum rounded to fp16 as the contract states"""
    c, s = cs[pos, :, 0].astype(f64), cs[pos, :, 1].astype(f64)
    while c.ndim < x.ndim:
        c, s = c[:, None], s[:, None]
    x0, x1 = x[..., 0::2].astype(f64), x[..., 1::2].astype(f64)
    h = lambda v: v.astype(f16).astype(f64)
    out = np.empty(x.shape, f16)
    out[..., 0::2] = h(c * x0) - h(s * x1)
    out[..., 1::2] = h(c * x1) + h(s * x0)
    return out


def _norm(x, w, eps, rounded=True):
    x = x.astype(f64)
    n = x / np.sqrt((x * x).mean(-1, keepdims=True) + eps)
    return (n.astype(f16).astype(f64) * w.astype(f64)).astype(f16) if rounded else n * w.astype(f64)


def test_mla_kv_store(tm, cuda):
    """rows of two sequences, q_len (3, 70) behind hist (0, 61): the second crosses two block boundaries; positions 128 .. 130 clamp
    to the table's last row; padded kv_a rows; a permuted table; layer 1 of 2"""
    rng = np.random.default_rng(7)
    H, qlen, hist, eps, max_pos, kvs = 3, [3, 70], [0, 61], 1e-6, 128, ROW + 8
    klen = [h + n for h, n in zip(hist, qlen)]
    T, cu = sum(qlen), _cu(qlen)
    tables, nblk = _tables(rng, klen)
    dc = DevCache(LAYOUT, nblk, tables)
    dc.pool.fill_(0xff)
    kv_a = (rng.standard_normal((T, kvs)) * rng.choice([0.05, 1.0, 30.0], (T, 1))).astype(f16)
    w = (1.0 + 0.2 * rng.standard_normal(RANK)).astype(f16)
    q = rng.standard_normal((T, H, ROW)).astype(f16)
    cs = rope_table(tm, max_pos, o.RopeParam(ROPE, 10000.0))
    q_d = dev(q)
    _ffi.check(tm.tm_mla_kv_store(dev(kv_a).data_ptr(), kvs, dev(w).data_ptr(), eps, q_d.data_ptr(), H * ROW, H, dev(cu).data_ptr(),
                                  dev(np.asarray(klen, np.int32)).data_ptr(), 2, T, dev(cs).data_ptr(), max_pos, dc.view(LAYER), st()))
    pool, got_q = dc.download(), host(q_d)
    want = np.full_like(pool, 0xff)
    for b in range(2):
        pos = np.minimum(hist[b] + np.arange(qlen[b]), max_pos - 1)
        rows = slice(cu[b], cu[b + 1])
        ref = np.concatenate([_norm(kv_a[rows, :RANK], w, eps), _rope64(kv_a[rows, RANK:ROW], cs, pos)], 1)
        got = _lay(pool)[_idx(tables[b], hist[b], klen[b])]
        d = ulp_diff_f16(got, ref)
        print(f'seq {b}: cache rows max ulp {d.max()} off {np.count_nonzero(d)} / {d.size}')
        assert np.isfinite(got).all() and d.max() <= 1 and (d > 0).mean() < 1e-3
        _lay(want)[_idx(tables[b], hist[b], klen[b])] = got
        dq = ulp_diff_f16(got_q[rows, :, RANK:], _rope64(q[rows, :, RANK:], cs, pos))
        assert dq.max() <= 1 and (dq > 0).mean() < 1e-3, f'seq {b}: q_pe max ulp {dq.max()}'
    assert np.array_equal(got_q[:, :, :RANK], q[:, :, :RANK]), 'q_lat must not be touched'
    assert np.array_equal(pool, want), f'{np.count_nonzero(pool != want)} pool bytes outside the written rows changed'


CASES = {'decode': ([1, 1, 1], [0, 63, 64]), 'verify': ([4, 8, 2], [129, 57, 300]), 'chunk': ([70], [5])}


@functools.lru_cache(maxsize=None)
def _attention_case(H, case):
    """(q, pool, tables, blocks, reference [rows, H * 512] float64); every cache row the kernel must not read is NaN"""
    qlen, hist = CASES[case]
    rng = np.random.default_rng(1000 * H + len(qlen))
    klen = [h + n for h, n in zip(hist, qlen)]
    tables, nblk = _tables(rng, klen)
    pool = np.full((nblk, LAYOUT.block_size // 2), NAN16, np.uint16).view(np.uint8)
    q = (0.6 * rng.standard_normal((sum(qlen), H, ROW))).astype(f16)
    cu, ref = _cu(qlen), []
    for b, n in enumerate(klen):
        rows = rng.standard_normal((n, ROW)).astype(f16)
        _lay(pool)[_idx(tables[b], 0, n)] = rows
        s = np.einsum('jhd,td->jht', q[cu[b]:cu[b + 1]].astype(f64), rows.astype(f64)) * SCALE
        seen = np.arange(n)[None, :] < hist[b] + np.arange(qlen[b])[:, None] + 1
        s = np.where(seen[:, None, :], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref.append(np.einsum('jht,td->jhd', p / p.sum(-1, keepdims=True), rows[:, :RANK].astype(f64)).reshape(qlen[b], -1))
    return q, pool, tables, nblk, np.concatenate(ref)


@pytest.mark.parametrize('splits', [1, 2, 4])
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('H', [1, 16, 24])
def test_mla_attention(tm, cuda, H, case, splits):
    """H 1 / 16 / 24: padding columns, exactly one chunk per row, a partial second chunk.  decode: contexts 1, 64, 65 (with splits 2
    and 4 some split owns no tile); verify: rows straddle a block boundary, five blocks; chunk: 70 prefill rows that cross a block.
    Ragged and rectangular block tables; the output is pre-filled with 7 and carries a canary row."""
    qlen, hist = CASES[case]
    q, pool, tables, nblk, ref = _attention_case(H, case)
    klen = np.asarray([h + n for h, n in zip(hist, qlen)], np.int32)
    rows = sum(qlen)
    dc = DevCache(LAYOUT, nblk, tables)
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
                                           splits, ws.data_ptr(), dc.view(LAYER), st()))
            got = host(out).astype(f64)
            assert (got[rows] == 7.0).all(), 'wrote past the last row'
            err = np.abs(got[:rows] - ref)
            print(f'H {H} {case} splits {splits} stride {mode}: max err {np.nanmax(err):.2e} max |ref| {np.abs(ref).max():.2f}')
            assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'stride {mode}: max err {np.nanmax(err)}, {np.isnan(got).sum()} NaN'
    finally:
        tm.tm_debug_set_block_stride(0)


def _err_units(x, ref):
    """largest error in units of the attention bound 1e-2 |ref| + 2e-3"""
    return float((np.abs(x.astype(f64) - ref) / (1e-2 * np.abs(ref) + 2e-3)).max())


def test_mla_forward_end_to_end(tm, cuda):
    """mla.mla_forward (einsum -> store -> attention -> einsum) against the NON-absorbed float64 MLA: k_nope and v expanded from the
    latent with kv_b_proj, per-head attention at 192 / 128.  H 16, nope 128, v 128; prefill rows (3, 66), the second crosses a block.
    Measured on one MI355X, in units of the attention bound: the fp16-torch-only absorbed path 0.448, the HIP path 0.390."""
    rng = np.random.default_rng(3)
    H, nope, vd, qlen, eps, max_pos = 16, 128, 128, [3, 66], 1e-6, 128
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
    ref = np.empty((T, H, vd), f64)
    for b, n in enumerate(qlen):
        r, pos = slice(cu[b], cu[b + 1]), np.arange(n)
        kv = (_norm(kv_a[r, :RANK], w, eps, rounded=False) @ wkvb.astype(f64).T).reshape(n, H, nope + vd)
        k = np.concatenate([kv[..., :nope], np.broadcast_to(rot(kv_a[r, None, RANK:].astype(f64), pos), (n, H, ROPE))], -1)
        qq = np.concatenate([q_nope[r].astype(f64), rot(q_pe[r].astype(f64), pos)], -1)
        s = np.where(np.tril(np.ones((n, n), bool))[:, None, :], np.einsum('jhd,thd->jht', qq, k) * SCALE, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref[r] = np.einsum('jht,thd->jhd', p / p.sum(-1, keepdims=True), kv[..., nope:])

    tables, nblk = _tables(rng, qlen)
    dc = DevCache(LAYOUT, nblk, tables)
    W_UK, W_UV = mla.absorb(dev(wkvb), H, nope, vd)
    got = host(mla.mla_forward(dev(q_nope), dev(q_pe), dev(kv_a), dev(w), W_UK, W_UV, dc.view(LAYER), dev(cu),
                               dev(np.asarray(qlen, np.int32)), SCALE, dev(cs), eps, splits=2))

    # the same absorbed path with torch alone, every intermediate fp16
    t16 = torch.empty((T, H, vd), dtype=torch.float16, device='cuda')
    q_lat = torch.einsum('thd,hdr->thr', dev(q_nope), W_UK)
    for b, n in enumerate(qlen):
        r, pos = slice(cu[b], cu[b + 1]), np.arange(n)
        c = dev(_norm(kv_a[r, :RANK], w, eps))
        rows = torch.cat([c, dev(_rope64(kv_a[r, RANK:], cs, pos))], 1)
        qf = torch.cat([q_lat[r], dev(_rope64(q_pe[r], cs, pos))], 2)
        s = (torch.einsum('jhd,td->jht', qf, rows) * SCALE).masked_fill(~torch.ones(n, n, dtype=torch.bool, device='cuda').tril()[:, None, :],
                                                                         float('-inf'))
        t16[r] = torch.einsum('jhr,hrv->jhv', torch.einsum('jht,tr->jhr', torch.softmax(s, -1), c), W_UV)
    e_t, e_h = _err_units(host(t16), ref), _err_units(got, ref)
    print(f'units of the attention bound: fp16 torch {e_t:.3f}, HIP {e_h:.3f}; max |ref| {np.abs(ref).max():.2f}')
    assert e_h <= 2 * e_t


def test_mla_refusals(tm, cuda):
    buf = torch.zeros(4096, dtype=torch.float16, device='cuda')
    one, two, cu = dev(np.asarray([1], np.int32)), dev(np.asarray([2], np.int32)), dev(np.asarray([0, 2], np.int32))
    dc = DevCache(LAYOUT, 1, [[0]])

    def view(**kw):
        c = dc.view(0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def attn(cache=None, klen=two, H=1, scale=SCALE, splits=1, ws=None):
        return tm.tm_mla_attention(buf.data_ptr(), buf.data_ptr(), H * ROW, cu.data_ptr(), klen.data_ptr(), 1, H, scale, splits, ws,
                                   cache or view(), st())

    def store(cache=None, klen=two, H=1):
        return tm.tm_mla_kv_store(buf.data_ptr(), ROW, buf.data_ptr(), 1e-6, buf.data_ptr(), H * ROW, H, cu.data_ptr(), klen.data_ptr(), 1, 2,
                                  None, 0, cache or view(), st())

    def refused(rc, *words):
        assert rc == 1 and all(w in _ffi.last_error() for w in words), (rc, _ffi.last_error())

    assert tm.tm_mla_layer_size(64, 512, 64) == 64 * ROW * 2
    assert [tm.tm_mla_layer_size(*bad) for bad in ((64, 256, 64), (64, 512, 32), (32, 512, 64))] == [-1] * 3
    for call in (attn, store):
        refused(call(cache=view(head_dim=128)), 'head_dim 576')
        refused(call(cache=view(head_dim=ROW + 64)), 'kv_lora_rank 512')
        refused(call(cache=view(bits=8)), 'bits 16')
        refused(call(cache=view(kv_heads=2)), 'kv_heads 1')
        refused(call(klen=one), 'k_len[b] >= q_len[b]')
        refused(call(H=0), 'H <= 128'), refused(call(H=129), 'H <= 128')
    refused(attn(splits=0), 'splits <= 128'), refused(attn(splits=129), 'splits <= 128')
    refused(attn(splits=2), 'workspace')
    refused(attn(scale=0.0), 'softmax_scale')
    # the launchers that existed before still refuse the latent view by name
    refused(tm.tm_kv_rope_store(buf.data_ptr(), 1, cu.data_ptr(), two.data_ptr(), 1, 2, None, 0, view(), st()), 'head_dim')
    assert attn() == 0 and store() == 0
