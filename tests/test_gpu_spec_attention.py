"""The verify attention kernel (csrc/attention_verify_mfma.hip: 1 .. 8 query rows per sequence over the paged int8 / int4 cache, a
score column per (row, head) pair) held to

(a) the bits of tests/attention_exact_reference.py's prefill cases quantised into the paged cache: every correct order of computation
    returns fp16(exact rational), so a mismatch is a wrong per-column limit, a foreign or dropped token, a wrong (scale, zero), a lost
    split or a column written to the wrong (row, head) -- never accumulation order.  Rows per sequence 1 .. 8, histories that end on,
    before and behind a block boundary (rows straddling it: a column that sees nothing of the newest tile), GQA groups 1 .. 8 (group 7:
    columns of one row in two chunks), split counts 1, 2, 4, a permuted block table, 0xFF in every byte the kernel must not read;
(b) the oracle's float64 attention over the dequantised cache on random operands, the project's attention bound
    |a - b| <= 1e-2 |b| + 2e-3 (tests/test_gpu_ops.py), at Llama-3-8B's group 4 with 4 rows (16 columns: one chunk) and group 8 with
    3 rows (two chunks);
(c) the existing decode kernel: row j against tm_decode_attention at k_len = hist + j + 1, the same bound (the tiles are cut at the
    same 64-token blocks, the splits differ)."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import attention_exact_reference as r
from tests.gpu_helpers import DevCache, dev, host, st

pytestmark = pytest.mark.gpu
f16 = np.float16
LAYER = 1
D = 128
SHAPES = (((4, 4, 2, 8, 1, 3), (0, 63, 64, 300, 129, 1086)), ((8, 8, 5), (57, 120, 250)))
SPLITS = (1, 2, 4)


def _tables(rng, klen, spare=2):
    nblk = [(k + 63) // 64 for k in klen]
    perm = rng.permutation(sum(nblk) + spare)
    tables, off = [], 0
    for nb in nblk:
        tables.append(perm[off:off + nb])
        off += nb
    return tables, len(perm)


def _verify(tm, out, q_d, cu_d, klen_d, B, Hq, scale, splits, ws, dc):
    _ffi.check(tm.tm_verify_attention(out.data_ptr(), q_d.data_ptr(), Hq * D, cu_d.data_ptr(), klen_d.data_ptr(), B, Hq, scale, splits,
                                      ws.data_ptr(), dc.view(LAYER), st()))


# ---- (a) bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', [1, 2, 4, 7, 8])
@pytest.mark.parametrize('bits', [8, 4])
def test_verify_attention_exact(tm, cuda, bits, group):
    n_cmp = 0
    for shape in SHAPES:
        for tier in 'AB':
            case = r.build('prefill', bits, D, 2 * group, 2, tier, shape)
            qlens, Hq, B, klen = shape[0], case.Hq, len(case.seqs), case.klen
            assert klen == [h + n for n, h in zip(*shape)]
            L = o.BlockLayout(2, case.Hkv, D, 64, bits)
            tables, total = _tables(np.random.default_rng(bits + group + len(qlens)), klen)
            pool = np.full((total, L.block_size), 0xFF, np.uint8)          # the other layer, spare blocks, rows behind the context
            for s, tab in zip(case.seqs, tables):
                r.fill_cache(pool, L, tab, LAYER, s.K, s.V)
            dc = DevCache(L, total, tables)
            dc.pool.copy_(torch.from_numpy(pool).cuda())
            cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
            T = int(cu[-1])
            q_d = dev(np.concatenate([s.q.reshape(len(s.q), -1) for s in case.seqs]))
            cu_d, klen_d = dev(cu), dev(np.asarray(klen, np.int32))
            ws = torch.full((max(1, tm.tm_verify_attention_workspace(T, Hq, max(SPLITS))),), 0xFF, dtype=torch.uint8, device='cuda')
            stride = max((k + 63) // 64 for k in klen) + 2
            for mode in (0, stride):                                       # ragged and rectangular block tables
                dc.set_tables(tables, stride=mode)
                for splits in SPLITS:
                    out = torch.full((T, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
                    _verify(tm, out, q_d, cu_d, klen_d, B, Hq, r.softmax_scale(tier, D), splits, ws, dc)
                    got = host(out).view(np.uint16).copy()
                    got[got == 0x8000] = 0
                    for b, s in enumerate(case.seqs):
                        g = got[cu[b]:cu[b + 1]].reshape(s.bits.shape)
                        bad = (g != s.bits) & ~s.loose
                        what = (f'bits {bits} group {group} tier {tier} q_lens {qlens} splits {splits} '
                                f'{"rectangular" if mode else "ragged"} table, sequence {b} (hist {s.hist}, rows {len(s.q)})')
                        assert not bad.any(), (f'{what}: {int(bad.sum())} outputs differ, first (row, head, channel) '
                                               f'{tuple(np.argwhere(bad)[0])}: got {g[bad][0]:#06x}, expected {s.bits[bad][0]:#06x}')
                        assert r.ulp16(g, s.bits)[s.loose].max(initial=0) <= 1, what
                    n_cmp += 1
    print(f'[verify attention exact] bits {bits} group {group}: {n_cmp} launches, all bits equal')


# ---- random operands: one cache and one set of references per (bits, group, rows), shared by (b) and (c) ----------------------------
HISTS = (0, 1, 65, 1089)       # row 0 sees 1 token; rows that straddle the first block boundary; context 1089 + rows
_RANDOM = {}


def _hists(rows):
    """the histories above and the ones that make the whole forward end at context 65 and 1089"""
    return sorted(set(HISTS) | {65 - rows, 1089 - rows})


def _random_case(bits, group, rows):
    key = (bits, group, rows)
    if key not in _RANDOM:
        rng = np.random.default_rng(1000 * bits + 10 * group + rows)
        Hkv, Hq = 2, 2 * group
        L = o.BlockLayout(2, Hkv, D, 64, bits)
        hists = _hists(rows)
        klen = [h + rows for h in hists]
        tables, total = _tables(rng, klen)
        oc = o.PagedKVCache(L, total)
        for b, n in enumerate(klen):
            k = rng.standard_normal((n, Hkv, D)).astype(f16)
            v = rng.standard_normal((n, Hkv, D)).astype(f16)
            if n > 40:
                k[n // 3] *= f16(6.0)                                    # the online-softmax rescale at a chosen tile
            o.process_kv(oc, tables[b], LAYER, k, v, None, None, 0)
        q = rng.standard_normal((len(klen), rows, Hq, D)).astype(f16)
        ref = np.zeros((len(klen), rows, Hq, D), np.float64)
        for b, n in enumerate(klen):
            kd, vd = zip(*[oc.load_dequant(tables[b], LAYER, hd, 0, n, 'decode') for hd in range(Hkv)])
            kd, vd = np.stack(kd), np.stack(vd)
            for j in range(rows):
                ctx = hists[b] + j + 1
                ref[b, j] = o.attention_reference_unfused(q[b, j], kd[:, :ctx], vd[:, :ctx])
        _RANDOM[key] = dict(L=L, hists=hists, klen=klen, tables=tables, total=total, oc=oc, q=q, ref=ref, Hq=Hq)
    return _RANDOM[key]


def _launch_random(tm, c, rows, splits):
    B, Hq = len(c['klen']), c['Hq']
    dc = DevCache(c['L'], c['total'], c['tables'])
    dc.upload(c['oc'])
    cu = (np.arange(B + 1) * rows).astype(np.int32)
    out = torch.full((B * rows, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
    ws = torch.full((max(1, tm.tm_verify_attention_workspace(B * rows, Hq, splits)),), 0xFF, dtype=torch.uint8, device='cuda')
    _verify(tm, out, dev(c['q'].reshape(B * rows, -1)), dev(cu), dev(np.asarray(c['klen'], np.int32)), B, Hq, 0.0, splits, ws, dc)
    return host(out).view(f16).reshape(B, rows, Hq, D), dc


# ---- (b) against the oracle's float64 attention --------------------------------------------------------------------------------------
@pytest.mark.parametrize('group,rows', [(4, 4), (8, 3)])
@pytest.mark.parametrize('bits', [8, 4])
def test_verify_attention_random(tm, cuda, bits, group, rows):
    c = _random_case(bits, group, rows)
    for splits in (1, 3):
        got, _ = _launch_random(tm, c, rows, splits)
        for b, h in enumerate(c['hists']):
            err = np.abs(got[b].astype(np.float64) - c['ref'][b])
            tol = 1e-2 * np.abs(c['ref'][b]) + 2e-3
            print(f'[verify attention random] bits {bits} group {group} rows {rows} splits {splits} hist {h}: max err {err.max():.2e}')
            assert np.all(err <= tol), f'hist {h} splits {splits}: max err {err.max()}, worst excess {(err - tol).max()}'


# ---- (c) against the existing decode kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group,rows', [(4, 4), (8, 3)])
@pytest.mark.parametrize('bits', [8, 4])
def test_verify_attention_matches_decode_kernel(tm, cuda, bits, group, rows):
    c = _random_case(bits, group, rows)
    B, Hq = len(c['klen']), c['Hq']
    got, dc = _launch_random(tm, c, rows, 2)
    ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, 2)), dtype=torch.uint8, device='cuda')
    for j in range(rows):
        out = torch.full((B, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
        klen_j = np.asarray([h + j + 1 for h in c['hists']], np.int32)
        _ffi.check(tm.tm_decode_attention(out.data_ptr(), dev(c['q'][:, j].reshape(B, -1)).data_ptr(), Hq * D, dev(klen_j).data_ptr(), B, Hq,
                                          0.0, 2, ws.data_ptr(), dc.view(LAYER), st()))
        ref = host(out).view(f16).reshape(B, Hq, D).astype(np.float32)
        err = np.abs(got[:, j].astype(np.float32) - ref)
        print(f'[verify vs decode] bits {bits} group {group} row {j}: max err {err.max():.2e}')
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'row {j}: max err {err.max()}'


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_verify_attention_refusals(tm, cuda):
    L = o.BlockLayout(2, 2, D, 64, 8)
    dc = DevCache(L, 4, [np.arange(2)])
    q = dev(np.zeros((9, 4 * D), f16))
    out = torch.zeros((9, 4 * D), dtype=torch.float16, device='cuda')

    def call(cu, klen, cache=None):
        return tm.tm_verify_attention(out.data_ptr(), q.data_ptr(), 4 * D, dev(np.asarray(cu, np.int32)).data_ptr(),
                                      dev(np.asarray(klen, np.int32)).data_ptr(), 1, 4, 0.0, 1, None, cache or dc.view(LAYER), st())
    assert call([0, 9], [20]) == 1 and '1 <= q_len' in _ffi.last_error()          # more than 8 rows
    assert call([0, 0], [20]) == 1 and '1 <= q_len' in _ffi.last_error()
    assert call([0, 4], [3]) == 1 and 'k_len' in _ffi.last_error()                # k_len counts every row
    L16 = o.BlockLayout(2, 2, D, 64, 16)
    assert call([0, 4], [20], DevCache(L16, 4, [np.arange(2)]).view(LAYER)) == 1 and 'int8 / int4' in _ffi.last_error()
    L64 = o.BlockLayout(2, 2, 64, 64, 8)
    assert call([0, 4], [20], DevCache(L64, 4, [np.arange(2)]).view(LAYER)) == 1 and 'head_dim 128' in _ffi.last_error()
    assert call([0, 8], [20]) == 0
