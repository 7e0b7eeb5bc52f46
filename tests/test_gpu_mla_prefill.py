"""GPU tests of MLA prefill in the expanded form (csrc/attention_mla_prefill.hip) against float64 numpy in this file.  Attention:
|a - b| <= 1e-2 |b| + 2e-3 (tests/test_gpu_ops.py, tests/test_gpu_mla_attention.py).  Flatten: bit equality.  End to end: the HIP path may
take twice the error of the fp16-torch-only absorbed path, in units of that bound, and leaves the cache bytes of form='absorbed'."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi, mla
from oracle import tm_oracle as o
from tests.gpu_helpers import DevCache, dev, host, rope_table, st

pytestmark = pytest.mark.gpu
f16, f64 = np.float16, np.float64
RANK, ROPE, ROW, NOPE, VD = 512, 64, 576, 128, 128
LAYERS, LAYER = 2, 1
LAYOUT = SimpleNamespace(kv_heads=1, head_dim=ROW, block_len=64, bits=16, layer_size=64 * ROW * 2, block_size=LAYERS * 64 * ROW * 2)
SCALE = 192 ** -0.5
GAP, PAD = 3, 8
CASES = {'one_tile': ([64], [0]), 'ragged': ([70, 5, 129], [5, 200, 0]), 'tail_row': ([1], [130]), 'empty': ([0, 17], [0, 0])}


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _k_off(klen):
    """sequence starts with a gap of GAP rows behind every sequence"""
    return (_cu(klen)[:-1] + GAP * np.arange(len(klen))).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(H, case):
    """(q, kv, lat, reference [rows, H * 128] float64): padded strides, k_pe inside a 576-wide buffer, NaN in every gap row"""
    qlen, hist = CASES[case]
    rng = np.random.default_rng(100 * H + len(qlen))
    klen = [h + n for h, n in zip(hist, qlen)]
    cu, off, tokens = _cu(qlen), _k_off(klen), sum(klen) + GAP * len(klen)
    q = (0.6 * rng.standard_normal((sum(qlen), H * 192 + PAD))).astype(f16)
    kv = np.full((tokens, H * 256 + PAD), np.nan, f16)
    lat = np.full((tokens, ROW), np.nan, f16)
    ref = []
    for b, n in enumerate(klen):
        rows = slice(off[b], off[b] + n)
        kv[rows] = rng.standard_normal((n, kv.shape[1])).astype(f16)
        lat[rows] = rng.standard_normal((n, ROW)).astype(f16)
        kvh = kv[rows, :H * 256].astype(f64).reshape(n, H, 256)
        k = np.concatenate([kvh[..., :NOPE], np.broadcast_to(lat[rows, None, RANK:].astype(f64), (n, H, ROPE))], -1)
        s = np.einsum('jhd,thd->jht', q[cu[b]:cu[b + 1], :H * 192].astype(f64).reshape(-1, H, 192), k) * SCALE
        seen = np.arange(n)[None, :] < hist[b] + np.arange(qlen[b])[:, None] + 1
        s = np.where(seen[:, None, :], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True)) if n else s
        ref.append(np.einsum('jht,thd->jhd', p / p.sum(-1, keepdims=True), kvh[..., NOPE:]).reshape(qlen[b], H * VD))
    return q, kv, lat, np.concatenate(ref)


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('H', [1, 3])
def test_mla_prefill_attention(tm, cuda, H, case):
    qlen, hist = CASES[case]
    q, kv, lat, ref = _case(H, case)
    klen = np.asarray([h + n for h, n in zip(hist, qlen)], np.int32)
    rows = sum(qlen)
    out = torch.full((rows + 1, H * VD), 7.0, dtype=torch.float16, device='cuda')
    lat_d = dev(lat)
    _ffi.check(tm.tm_mla_prefill_attention(out.data_ptr(), dev(q).data_ptr(), q.shape[1], dev(kv).data_ptr(), kv.shape[1],
                                           lat_d.data_ptr() + RANK * 2, ROW, dev(_cu(qlen)).data_ptr(), dev(_k_off(klen)).data_ptr(),
                                           dev(klen).data_ptr(), len(qlen), max(qlen), H, SCALE, st()))
    got = host(out).astype(f64)
    assert (got[rows] == 7.0).all(), 'wrote past the last row'
    err = np.abs(got[:rows] - ref)
    print(f'H {H} {case}: max err {np.nanmax(err):.2e} max |ref| {np.abs(ref).max():.2f}')
    assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'max err {np.nanmax(err)}, {np.isnan(got).sum()} NaN'


def _tables(rng, klen, spare=2):
    nblk = [(k + 63) // 64 for k in klen]
    perm = rng.permutation(sum(nblk) + spare)
    return [perm[sum(nblk[:b]):sum(nblk[:b + 1])] for b in range(len(klen))], sum(nblk) + spare


def _lay(pool):
    return pool.reshape(len(pool), LAYERS, 64, ROW * 2)[:, LAYER].view(f16)


def test_mla_flatten(tm, cuda):
    rng = np.random.default_rng(11)
    klen = [1, 64, 65, 130]
    tables, nblk = _tables(rng, klen)
    dc = DevCache(LAYOUT, nblk, tables)
    pool = rng.integers(0, 256, (nblk, LAYOUT.block_size), dtype=np.uint8)
    dc.pool.copy_(torch.from_numpy(pool).cuda())
    off = _k_off(klen)
    total = int(off[-1]) + klen[-1] + GAP
    out = torch.full((total, ROW), 7.0, dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_mla_flatten(out.data_ptr(), dev(off).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), len(klen), max(klen),
                                 dc.view(LAYER), st()))
    want = np.full((total, ROW), 7.0, f16)
    for b, n in enumerate(klen):
        t = np.arange(n)
        want[off[b]:off[b] + n] = _lay(pool)[np.asarray(tables[b])[t // 64], t % 64]
    assert np.array_equal(host(out).view(np.uint16), want.view(np.uint16))


def _err_units(x, ref):
    return float((np.abs(x.astype(f64) - ref) / (1e-2 * np.abs(ref) + 2e-3)).max())


def test_mla_forward_expanded_end_to_end(tm, cuda):
    """mla_forward(form='expanded') against the NON-absorbed float64 MLA (the construction of test_gpu_mla_attention.py).  H 2; two
    sequences, the second behind 70 rows that an earlier mla_forward call wrote; the same inputs through form='absorbed' on a second
    pool must leave the same cache bytes."""
    rng = np.random.default_rng(5)
    H, eps, max_pos = 2, 1e-6, 256
    hist, qlen = [0, 70], [66, 37]
    klen = [h + n for h, n in zip(hist, qlen)]
    wkvb = (rng.standard_normal((H * (NOPE + VD), RANK)) / np.sqrt(RANK)).astype(f16)
    w = (1.0 + 0.1 * rng.standard_normal(RANK)).astype(f16)
    cs = rope_table(tm, max_pos, o.RopeParam(ROPE, 10000.0))
    kv_a = [rng.standard_normal((n, ROW)).astype(f16) for n in klen]                       # every token of each sequence
    q_nope = [(0.6 * rng.standard_normal((n, H, NOPE))).astype(f16) for n in qlen]
    q_pe = [(0.6 * rng.standard_normal((n, H, ROPE))).astype(f16) for n in qlen]

    def rot(x, pos):            # float64, no rounding
        c, s = cs[pos, :, 0].astype(f64)[:, None], cs[pos, :, 1].astype(f64)[:, None]
        y = np.empty(x.shape, f64)
        y[..., 0::2], y[..., 1::2] = c * x[..., 0::2] - s * x[..., 1::2], c * x[..., 1::2] + s * x[..., 0::2]
        return y

    def norm(x, rounded):
        x = x.astype(f64)
        n = x / np.sqrt((x * x).mean(-1, keepdims=True) + eps)
        return (n.astype(f16).astype(f64) * w.astype(f64)).astype(f16) if rounded else n * w.astype(f64)

    def rope16(x, pos):         # the store's rotation: each product rounded to fp16
        c, s = cs[pos, :, 0].astype(f64), cs[pos, :, 1].astype(f64)
        while c.ndim < x.ndim:
            c, s = c[:, None], s[:, None]
        x0, x1, h = x[..., 0::2].astype(f64), x[..., 1::2].astype(f64), lambda v: v.astype(f16).astype(f64)
        out = np.empty(x.shape, f16)
        out[..., 0::2], out[..., 1::2] = h(c * x0) - h(s * x1), h(c * x1) + h(s * x0)
        return out

    W_UK, W_UV = mla.absorb(dev(wkvb), H, NOPE, VD)
    ref, t16 = [], []
    for b, n in enumerate(klen):
        pos, qpos = np.arange(n), hist[b] + np.arange(qlen[b])
        kv = (norm(kv_a[b][:, :RANK], False) @ wkvb.astype(f64).T).reshape(n, H, NOPE + VD)
        k = np.concatenate([kv[..., :NOPE], np.broadcast_to(rot(kv_a[b][:, None, RANK:].astype(f64), pos), (n, H, ROPE))], -1)
        qq = np.concatenate([q_nope[b].astype(f64), rot(q_pe[b].astype(f64), qpos)], -1)
        seen = pos[None, :] <= qpos[:, None]
        s = np.where(seen[:, None, :], np.einsum('jhd,thd->jht', qq, k) * SCALE, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref.append(np.einsum('jht,thd->jhd', p / p.sum(-1, keepdims=True), kv[..., NOPE:]))
        # the absorbed path with torch alone, every intermediate fp16
        c = dev(norm(kv_a[b][:, :RANK], True))
        rows = torch.cat([c, dev(rope16(kv_a[b][:, RANK:], pos))], 1)
        qf = torch.cat([torch.einsum('thd,hdr->thr', dev(q_nope[b]), W_UK), dev(rope16(q_pe[b], qpos))], 2)
        sc = (torch.einsum('jhd,td->jht', qf, rows) * SCALE).masked_fill(~dev(seen)[:, None, :], float('-inf'))
        t16.append(host(torch.einsum('jhr,hrv->jhv', torch.einsum('jht,tr->jhr', torch.softmax(sc, -1), c), W_UV)))
    ref, t16 = np.concatenate(ref), np.concatenate(t16)

    tables, nblk = _tables(rng, klen)
    pools, got = [], None
    for form in ('expanded', 'absorbed'):
        dc = DevCache(LAYOUT, nblk, tables)
        args = lambda qn, qp, ka, cu, kl: (dev(qn), dev(qp), dev(ka), dev(w), W_UK, W_UV, dc.view(LAYER), dev(_cu(cu)),
                                           dev(np.asarray(kl, np.int32)), SCALE, dev(cs), eps)
        # the second sequence's history, written by an earlier forward of its own (sequence 0 takes no part: q_len 0, k_len 0)
        mla.mla_forward(*args(np.zeros((70, H, NOPE), f16), np.zeros((70, H, ROPE), f16), kv_a[1][:70], [0, 70], [0, 70]), form=form)
        y = mla.mla_forward(*args(np.concatenate(q_nope), np.concatenate(q_pe), np.concatenate([kv_a[0], kv_a[1][70:]]), qlen, klen),
                            form=form)
        pools.append(dc.download())
        got = host(y) if form == 'expanded' else got
    e_t, e_h = _err_units(t16, ref), _err_units(got, ref)
    print(f'units of the attention bound: fp16 torch {e_t:.3f}, expanded HIP {e_h:.3f}; max |ref| {np.abs(ref).max():.2f}')
    assert got.shape == (sum(qlen), H, VD) and e_h <= 2 * e_t
    assert np.array_equal(pools[0], pools[1]), 'form=expanded must leave the cache bytes of form=absorbed'


def test_mla_prefill_refusals(tm, cuda):
    buf = torch.zeros(8192, dtype=torch.float16, device='cuda')
    cu, one = dev(np.asarray([0, 1], np.int32)), dev(np.asarray([1], np.int32))
    dc = DevCache(LAYOUT, 1, [[0]])
    ptr = buf.data_ptr()

    def attn(H=1, scale=SCALE, qs=None, kvs=None, pes=64, q=ptr):
        return tm.tm_mla_prefill_attention(ptr, q, H * 192 if qs is None else qs, ptr, H * 256 if kvs is None else kvs, ptr, pes,
                                           cu.data_ptr(), cu.data_ptr(), one.data_ptr(), 1, 1, H, scale, st())

    def flat(**kw):
        c = dc.view(0)
        for k, v in kw.items():
            setattr(c, k, v)
        return tm.tm_mla_flatten(ptr, cu.data_ptr(), one.data_ptr(), 1, 1, c, st())

    for rc, word in ((lambda: attn(H=0), 'H <= 128'), (lambda: attn(H=129), 'H <= 128'), (lambda: attn(scale=0.0), 'softmax_scale'),
                     (lambda: attn(H=2, qs=376), 'q_stride'), (lambda: attn(H=2, kvs=504), 'kv_stride'), (lambda: attn(pes=56), 'pe_stride'),
                     (lambda: attn(qs=196), '16-byte aligned'), (lambda: attn(q=ptr + 2), '16-byte aligned'),
                     (lambda: flat(head_dim=128), 'head_dim 576'), (lambda: flat(bits=8), 'bits 16'), (lambda: flat(kv_heads=2), 'kv_heads 1'),
                     (lambda: flat(block_len=32), 'block_len 64')):
        assert rc() == 1 and word in _ffi.last_error(), (word, _ffi.last_error())
    assert attn() == 0 and flat() == 0
