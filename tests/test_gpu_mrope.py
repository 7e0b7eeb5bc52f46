"""M-RoPE and image-embedding operators, bit for bit against the numpy contract of tests/qwen_vl_reference.py:
tm_kv_rope_store_mrope (sections, coordinates, position delta, clamp), tm_decode_attention_fused_delta (the fused prologue's
pos_delta) and tm_embedding_mixed."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import qwen_vl_reference as Q
from tests.gpu_helpers import DevCache, dev, host, rope_table, st
from tests.qwen_reference import prologue
from tests.test_gpu_rope_scaling import _kv_case

pytestmark = pytest.mark.gpu
f16 = np.float16
Hq, Hkv, LAYER, MAX_POS = 4, 2, 1, 256
LENS_NEW, HIST = [70, 5, 1], [0, 130, 63]        # crosses a block boundary; a later chunk; the last row of a block
DELTAS = np.array([0, -11, -37], np.int32)
ROPE = o.RopeParam(128, 10000.0)


def _coords(sections_case: bool):
    """[T, 3] coordinates of the three sequences' new rows.  Sequence 0: text, then a 6 x 9 image grid (three distinct axes) whose last
    row carries a w coordinate at and one above max_pos (the clamp), then text.  Sequence 1: rows 130 .. 134 of a sequence whose history
    held an image (delta -11): two more image rows, then text at p + delta.  Sequence 2: no coordinates, delta -37 (26 on all axes)."""
    c0 = np.zeros((70, 3), np.int32)
    c0[:8] = np.arange(8)[:, None]
    t, r, c = np.meshgrid([0], np.arange(6), np.arange(9), indexing='ij')
    c0[8:62] = 8 + np.stack([t.reshape(-1), r.reshape(-1), c.reshape(-1)], 1)
    c0[60, 2], c0[61, 2] = MAX_POS - 1, MAX_POS + 1
    c0[62:] = (17 + np.arange(8))[:, None]
    c1 = np.array([[100, 118, 107], [100, 118, 108], [119, 119, 119], [120, 120, 120], [121, 121, 121]], np.int32)
    c2 = np.full((1, 3), 63 - 37, np.int32)
    if not sections_case:      # all axes = the linear position
        return np.concatenate([np.broadcast_to(np.arange(h, h + n)[:, None], (n, 3)) for h, n in zip(HIST, LENS_NEW)]).astype(np.int32)
    return np.concatenate([c0, c1, c2])


def _reference(L, tables, total, qkv, coords, Lw, sections):
    oc = o.PagedKVCache(L, total)
    cu = np.concatenate([[0], np.cumsum(LENS_NEW)]).astype(np.int32)
    q_ref = np.zeros((len(qkv), Hq, 128), f16)
    for b, n in enumerate(LENS_NEW):
        sl = slice(cu[b], cu[b + 1])
        cos, sin = Q.mrope_cos_sin(ROPE, coords[sl].T, sections, MAX_POS)
        q, k, v = prologue(qkv[sl, :Hq * 128].reshape(n, Hq, 128), qkv[sl, Hq * 128:(Hq + Hkv) * 128].reshape(n, Hkv, 128),
                           qkv[sl, (Hq + Hkv) * 128:].reshape(n, Hkv, 128), Lw, 0.0)
        q_ref[sl] = o.rope_apply(q, cos, sin)
        o.process_kv(oc, tables[b], LAYER, k, v, cos, sin, HIST[b])
    return oc.pool, q_ref, cu


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('sections', [(16, 24, 24), (10, 27, 27)])      # boundaries at multiples of 4 / inside a lane's four pairs
@pytest.mark.parametrize('bits', [16, 8, 4])
def test_kv_rope_store_mrope_bit_exact(tm, cuda, bits, sections, bias):
    L, tables, total, klen, qkv = _kv_case(bits, LENS_NEW, HIST, Hq, Hkv, seed=bits + 1)
    rng = np.random.default_rng(bits)
    Lw = dict(qkv_bias=(0.5 * rng.standard_normal((Hq + 2 * Hkv) * 128)).astype(f16)) if bias else {}
    bias_d = dev(Lw['qkv_bias']) if bias else None
    tab_d = dev(rope_table(tm, MAX_POS, ROPE))
    coords = _coords(True)
    pool, q_ref, cu = _reference(L, tables, total, qkv, coords, Lw, sections)
    cu_d, kl_d = dev(cu), dev(np.asarray(klen, np.int32))

    def run(mrope_pos, delta, entry='mrope', secs=sections):
        dc, q = DevCache(L, total, tables), dev(qkv.copy())
        head = (q.data_ptr(), Hq, cu_d.data_ptr(), kl_d.data_ptr(), len(LENS_NEW), len(qkv), tab_d.data_ptr(), MAX_POS)
        tail = (bias_d.data_ptr() if bias else None, None, None, 0.0, dc.view(LAYER), st())
        if entry == 'mrope':
            _ffi.check(tm.tm_kv_rope_store_mrope(*head, mrope_pos.data_ptr() if mrope_pos is not None else None,
                                                 delta.data_ptr() if delta is not None else None, *secs, *tail))
        else:
            _ffi.check(tm.tm_kv_rope_store_qk(*head, *tail))
        return dc.download(), host(q)[:, :Hq * 128].reshape(-1, Hq, 128)

    got, q_got = run(dev(coords), None)
    assert np.array_equal(got, pool), f'cache bytes differ in {np.count_nonzero(got != pool)} positions'
    assert np.array_equal(q_got.view(np.uint16), q_ref.view(np.uint16)), 'RoPE(q) must be bit exact'
    # all three axes = the linear position, delta 0 (array of zeros, or none): tm_kv_rope_store_qk's bytes and q
    plain, q_plain = run(None, None, 'qk')
    assert not np.array_equal(plain, pool), 'the coordinates must change the K bytes'
    for mp, dl in ((dev(_coords(False)), None), (None, dev(np.zeros(3, np.int32))), (None, None)):
        g, q = run(mp, dl)
        assert np.array_equal(g, plain) and np.array_equal(q.view(np.uint16), q_plain.view(np.uint16))
    # no coordinates: every row at linear position + delta[b] on all axes, clamped at 0 (sequence 2: 63 - 37; a delta of -200: row 0)
    for deltas in (DELTAS, np.array([-200, 3, 200], np.int32)):
        lin = np.concatenate([np.broadcast_to(np.arange(h, h + n)[:, None] + d, (n, 3)) for h, n, d in zip(HIST, LENS_NEW, deltas)])
        pool_d, q_d, _ = _reference(L, tables, total, qkv, lin, Lw, sections)
        g, q = run(None, dev(deltas))
        assert np.array_equal(g, pool_d) and np.array_equal(q.view(np.uint16), q_d.view(np.uint16))


def test_kv_rope_store_mrope_refusals(tm, cuda):
    buf = torch.zeros(8 * 6 * 128, dtype=torch.float16, device='cuda')
    cu, one = dev(np.array([0, 1], np.int32)), dev(np.array([1], np.int32))
    tab = dev(np.zeros((4, 64, 2), f16))

    def call(bits=8, D=128, secs=(16, 24, 24), table=True):
        L = o.BlockLayout(1, 1, D, 64, 4 if bits == 42 else bits)
        dc = DevCache(L, 2, [np.array([0])])
        view = dc.view(0)
        view.bits = bits
        return tm.tm_kv_rope_store_mrope(buf.data_ptr(), 1, cu.data_ptr(), one.data_ptr(), 1, 1, tab.data_ptr() if table else None, 4, None,
                                         None, *secs, None, None, None, 0.0, view, st())

    def refused(rc, *words):
        assert rc != 0
        msg = _ffi.last_error()
        assert all(w in msg for w in words), msg
    refused(call(bits=42), 'M-RoPE', '42')
    refused(call(D=64, secs=(8, 12, 12)), 'M-RoPE', 'head_dim 64')
    refused(call(secs=(16, 24, 20)), 'sections')
    refused(call(table=False), 'table')
    assert call() == 0
    # (per-sequence tables: neither the entry nor its launcher takes row offsets; the engine refuses rope_type 4 with sections --
    # tests/test_gpu_qwen_vl_engine.py::test_engine_refusals)


# ---- fused decode prologue with pos_delta --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('klen,splits,qkv_splits', [([64, 65, 300], 1, 0), ([64, 65, 300], 3, 2)])
@pytest.mark.parametrize('bits', [8, 4])
def test_decode_attention_fused_delta(tm, cuda, bits, klen, splits, qkv_splits, bias):
    """geometry of test_gpu_ops.test_decode_attention_fused_prologue (8 q / 2 kv heads); deltas (0, -37, +5): 299 + 5 passes
    max_pos - 1 = 301 and clamps"""
    q_heads, kv_heads, layer = 8, 2, 1
    rng = np.random.default_rng(sum(klen) + splits + qkv_splits + bits)
    L = o.BlockLayout(2, kv_heads, 128, 64, bits)
    B, hist = len(klen), [k - 1 for k in klen]
    nblk = [(k + 63) // 64 for k in klen]
    total = sum(nblk) + 2
    perm = rng.permutation(total)
    tables = [perm[sum(nblk[:b]):sum(nblk[:b + 1])] for b in range(B)]
    oc = o.PagedKVCache(L, total)
    for b, n in enumerate(hist):
        o.process_kv(oc, tables[b], layer, rng.standard_normal((n, kv_heads, 128)).astype(f16),
                     rng.standard_normal((n, kv_heads, 128)).astype(f16), None, None, 0)
    qkv_n = (q_heads + 2 * kv_heads) * 128
    if qkv_splits:
        slabs = (rng.standard_normal((qkv_splits, B, qkv_n)) / np.sqrt(qkv_splits)).astype(np.float32)
        acc = np.zeros((B, qkv_n), np.float32)
        for s_ in slabs:
            acc = acc + s_
        qkv, qkv_in = acc.astype(f16), dev(slabs)
    else:
        qkv = rng.standard_normal((B, qkv_n)).astype(f16)
        qkv_in = dev(qkv.copy())
    Lw = dict(qkv_bias=(0.5 * rng.standard_normal(qkv_n)).astype(f16)) if bias else {}
    bias_d = dev(Lw['qkv_bias']) if bias else None
    max_pos = 302
    deltas = np.array([0, -37, 5], np.int32)
    tab = rope_table(tm, max_pos, ROPE)
    rows = np.clip(np.asarray(hist) + deltas, 0, max_pos - 1)
    assert rows.tolist() == [63, 27, 301] and hist[2] + 5 > max_pos - 1
    klen_d = dev(np.asarray(klen, np.int32))
    ws_n = max(1, tm.tm_decode_attention_workspace(B, q_heads, splits))

    def run(table, delta):
        dc = DevCache(L, total, tables)
        dc.upload(oc)
        out = torch.zeros((B, q_heads * 128), dtype=torch.float16, device='cuda')
        ws = torch.zeros(ws_n, dtype=torch.uint8, device='cuda')
        _ffi.check(tm.tm_decode_attention_fused_delta(out.data_ptr(), qkv_in.data_ptr(), qkv_splits, qkv_n, dev(table).data_ptr(), max_pos,
                                                      dev(delta).data_ptr() if delta is not None else None,
                                                      bias_d.data_ptr() if bias else None, None, None, 0.0, klen_d.data_ptr(), B, q_heads,
                                                      0.0, splits, ws.data_ptr(), dc.view(layer), st()))
        return host(out), dc.download()

    out, pool = run(tab, deltas)
    # the new token's KV bytes: the contract (row clamp(k_len - 1 + delta)) through process_kv at the linear position
    for b in range(B):
        cos, sin = o.rope_cos_sin(ROPE, rows[b:b + 1])
        _, k, v = prologue(qkv[b:b + 1, :q_heads * 128].reshape(1, q_heads, 128),
                           qkv[b:b + 1, q_heads * 128:(q_heads + kv_heads) * 128].reshape(1, kv_heads, 128),
                           qkv[b:b + 1, (q_heads + kv_heads) * 128:].reshape(1, kv_heads, 128), Lw, 0.0)
        o.process_kv(oc, tables[b], layer, k, v, cos, sin, hist[b])
    assert np.array_equal(pool, oc.pool), f'cache bytes differ in {np.count_nonzero(pool != oc.pool)} positions'
    # the same entry, delta 0, on a table whose rows are pre-shifted by the deltas (the three linear positions are distinct rows)
    shifted = tab.copy()
    shifted[hist] = tab[rows]
    out_s, pool_s = run(shifted, np.zeros(B, np.int32))
    assert np.array_equal(out_s.view(np.uint16), out.view(np.uint16)) and np.array_equal(pool_s, pool)
    # a zero delta array = no delta array, bit for bit; and the deltas do change the result
    out_z, pool_z = run(tab, np.zeros(B, np.int32))
    out_n, pool_n = run(tab, None)
    assert np.array_equal(out_z.view(np.uint16), out_n.view(np.uint16)) and np.array_equal(pool_z, pool_n)
    assert np.array_equal(out[0].view(np.uint16), out_n[0].view(np.uint16)) and not np.array_equal(pool, pool_n)


# ---- embeddings -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden', [256, 384])
def test_embedding_mixed(tm, cuda, hidden):
    rng = np.random.default_rng(hidden)
    vocab, T = 50, 7
    table = rng.standard_normal((vocab, hidden)).astype(f16)
    rows = rng.standard_normal((3, hidden)).astype(f16)
    rows[1, :4] = np.array([np.inf, -0.0, 6e-8, np.nan]).astype(f16)        # copied bit for bit
    ids = np.array([3, 999, -5, 49, 0, 7, 7], np.int32)                      # ids under an embedding row are not read
    index = np.array([-1, 0, 1, -1, 2, -1, -1], np.int32)
    want = np.where(index[:, None] >= 0, rows[np.maximum(index, 0)], table[np.clip(ids, 0, vocab - 1)])
    out = torch.full((T + 1, hidden), 7.0, dtype=torch.float16, device='cuda')
    args = (dev(table).data_ptr(), dev(ids).data_ptr())
    _ffi.check(tm.tm_embedding_mixed(out.data_ptr(), *args, dev(rows).data_ptr(), dev(index).data_ptr(), T, hidden, vocab, st()))
    got = host(out)
    assert np.array_equal(got[:T].view(np.uint16), want.view(np.uint16)) and np.all(got[T] == f16(7.0))
    # all -1 = tm_embedding
    a, b = torch.zeros((T, hidden), dtype=torch.float16, device='cuda'), torch.zeros((T, hidden), dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_embedding_mixed(a.data_ptr(), *args, dev(rows).data_ptr(), dev(np.full(T, -1, np.int32)).data_ptr(), T, hidden, vocab, st()))
    _ffi.check(tm.tm_embedding(b.data_ptr(), *args, T, hidden, vocab, st()))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
