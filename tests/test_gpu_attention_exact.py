"""The attention kernels against operands whose softmax weights are exact powers of two and whose weighted sums are exact in fp32
(tests/attention_exact_reference.py; proved on the CPU by tests/test_host_attention_exact.py): every correct order of computation
-- tile size, wave interleave, split count, merge order, rescale schedule -- returns the same bits, fp16(exact rational), and the
kernels are held to those bits.  A mismatch is a dropped, doubled or foreign token, a wrong (scale, zero), a mask or diagonal off by
one, a rescale with the wrong alpha or a lost split, never an accumulation-order effect.

Tier A (default scale, weights 0 or 1) rests on 0 * x = 0, exp2(0) = 1 and exp2(<= -150) = 0 alone; tier B (softmax_scale =
float32(ln 2 / 32), weights 2^0 .. 2^-8) also needs v_exp_f32 to be exact at integer arguments in [-24, 0].

All comparisons are equalities of uint16 views with -0 mapped to +0.  Outputs are pre-filled with fp16 NaN, the cache pool outside
the sequences' own rows and the split-KV workspace with 0xFF; the workspace is allocated once per case and never cleared.  The slots
of a partial newest block behind the context hold rows that look live to every head.

Comparisons (case x kernel launch): decode 576 (6 (KV width, head_dim) x 6 GQA groups x 2 tiers x 2 block-table forms x 4 split
counts), fused prologue 16 (2 KV widths x 2 tiers x fp16 / fp32-slab input x 2 split counts), prefill 60 (2 head_dims x 5 GQA groups x 3 batches x 2 tiers).  All equal on an MI355X, tier B included: v_exp_f32 returned
the exact power of two at every integer argument these cases reach (0 .. -8 for weights and rescales, <= -150 -> 0)."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import attention_exact_reference as r
from tests.gpu_helpers import DevCache, dev, host, st

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
LAYER = 1
SPLITS = (1, 2, 3, 16)                       # 16: more splits than tiles for all but the longest sequence -- they contribute nothing


def _tables(rng, klen, spare=2):
    nblk = [(k + 63) // 64 for k in klen]
    perm = rng.permutation(sum(nblk) + spare)                # shuffled block tables
    tables, off = [], 0
    for nb in nblk:
        tables.append(perm[off:off + nb])
        off += nb
    return tables, len(perm)


def _pool(case, L, tables, total):
    """0xFF everywhere (fp16 / (scale, zero) NaN: the other layer, the spare blocks), the sequences' rows and the look-alive rows
    behind them in LAYER"""
    pool = np.full((total, L.block_size), 0xFF, np.uint8)
    for s, tab in zip(case.seqs, tables):
        r.fill_cache(pool, L, tab, LAYER, s.K, s.V)
    return pool


def _assert_bits(got, case, what):
    got = got.view(np.uint16).reshape(len(case.seqs), -1).copy()
    got[got == 0x8000] = 0
    for b, s in enumerate(case.seqs):
        g, e = got[b].reshape(s.bits.shape[1:]), s.bits[0]
        bad = (g != e) & ~s.loose[0]
        assert not bad.any(), (f'{what}, sequence {b} (k_len {s.n}): {int(bad.sum())} outputs differ, first (head, channel) '
                               f'{tuple(np.argwhere(bad)[0])}: got {g[bad][0]:#06x}, expected {e[bad][0]:#06x}')
        assert r.ulp16(g, e)[s.loose[0]].max(initial=0) <= 1, what


# ---- decode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,bits', [(128, 8), (128, 4), (128, 16), (64, 8), (64, 4), (64, 16)])
def test_decode_attention_exact(tm, cuda, D, bits):
    """D = 128 at 8 / 4 bits: the MFMA kernel; everything else: the VALU kernel.  GQA groups 1 .. 20 (20 = two chunks of 10 heads),
    ragged and rectangular block tables, 1 .. 16 splits"""
    n_cmp = 0
    try:
        for group in r.GROUPS_DECODE:
            for tier in 'AB':
                case = r.decode_case(bits, D, group, tier)
                klen, B, Hq = case.klen, len(case.seqs), case.Hq
                L = o.BlockLayout(2, case.Hkv, D, 64, bits)
                tables, total = _tables(np.random.default_rng(bits + D + group), klen)
                dc = DevCache(L, total, tables)
                dc.pool.copy_(torch.from_numpy(_pool(case, L, tables, total)).cuda())
                q_d = dev(np.stack([s.q[0].reshape(-1) for s in case.seqs]))
                klen_d = dev(np.asarray(klen, np.int32))
                ws = torch.full((max(1, tm.tm_decode_attention_workspace(B, Hq, max(SPLITS))),), 0xFF, dtype=torch.uint8, device='cuda')
                stride = max((k + 63) // 64 for k in klen) + 2
                for mode in (0, stride):
                    dc.set_tables(tables, stride=mode)
                    _ffi.check(tm.tm_debug_set_block_stride(mode))
                    for splits in SPLITS:
                        out = torch.full((B, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
                        _ffi.check(tm.tm_decode_attention(out.data_ptr(), q_d.data_ptr(), Hq * D, klen_d.data_ptr(), B, Hq,
                                                          r.softmax_scale(tier, D), splits, ws.data_ptr(), dc.view(LAYER), st()))
                        _assert_bits(host(out), case, f'bits {bits} head_dim {D} group {group} tier {tier} '
                                                      f'{"rectangular" if mode else "ragged"} table splits {splits}')
                        n_cmp += 1
    finally:
        tm.tm_debug_set_block_stride(0)
    print(f'[attention exact] decode bits {bits} head_dim {D}: {n_cmp} launches, all bits equal')


# ---- fused prologue -------------------------------------------------------------------------------------------------------------
KLEN_FUSED = (1, 63, 64, 65, 129, 257, 1089)


@pytest.mark.parametrize('bits', [8, 4])
def test_decode_attention_fused_exact(tm, cuda, bits):
    """the newest token arrives in the qkv input (fp16, or two fp32 slabs of integers and quarter-integers that sum exactly); with the
    eight live-set patterns over eight heads it is live alone in one head, live with older tokens in another and dead in the others.
    Its cache slot holds 0xFF before the launch; afterwards the pool equals o.process_kv's and the outputs the expected bits."""
    D, group = 128, 8
    n_cmp = 0
    for tier in 'AB':
        case = r.decode_case(bits, D, group, tier, KLEN_FUSED)
        klen, B, Hq, Hkv = case.klen, len(case.seqs), case.Hq, case.Hkv
        L = o.BlockLayout(2, Hkv, D, 64, bits)
        tables, total = _tables(np.random.default_rng(bits), klen)
        full = _pool(case, L, tables, total)
        oc = o.PagedKVCache(L, total)
        oc.pool[:] = full
        for s, tab in zip(case.seqs, tables):                # the new token's slot: 0xFF (codes, scale and zero)
            blk, ti = oc.pool[tab[(s.n - 1) // 64]], (s.n - 1) % 64
            for hd in range(Hkv):
                for doff, poff in ((L.k_data(hd, ti), L.k_param(hd, ti)), (L.v_data(hd, ti), L.v_param(hd, ti))):
                    blk[L.layer_offset(LAYER) + doff:L.layer_offset(LAYER) + doff + L.token_data_size] = 0xFF
                    blk[L.layer_offset(LAYER) + poff:L.layer_offset(LAYER) + poff + 4] = 0xFF
        before = oc.pool.copy()
        assert not np.array_equal(before, full)
        for s, tab in zip(case.seqs, tables):
            o.process_kv(oc, tab, LAYER, s.K[:, s.n - 1][None], s.V[:, s.n - 1][None], None, None, s.n - 1)
        assert np.array_equal(oc.pool, full)                  # the oracle's store of the new token is the vectorised fill's
        qkv = np.stack([np.concatenate([s.q[0].reshape(-1), s.K[:, s.n - 1].reshape(-1), s.V[:, s.n - 1].reshape(-1)]) for s in case.seqs])
        qkv_n = (Hq + 2 * Hkv) * D
        assert qkv.shape == (B, qkv_n)
        slab0 = np.random.default_rng(1).integers(-300, 300, qkv.shape).astype(f32)
        slabs = np.stack([slab0, qkv.astype(f32) - slab0])
        assert np.array_equal((slabs[0] + slabs[1]).astype(f16).view(np.uint16), qkv.view(np.uint16))
        klen_d = dev(np.asarray(klen, np.int32))
        dc = DevCache(L, total, tables)
        ws = torch.full((max(1, tm.tm_decode_attention_workspace(B, Hq, 3)),), 0xFF, dtype=torch.uint8, device='cuda')
        for qkv_splits, qkv_in in ((0, dev(qkv)), (2, dev(slabs))):
            for splits in (1, 3):
                dc.pool.copy_(torch.from_numpy(before).cuda())
                out = torch.full((B, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
                _ffi.check(tm.tm_decode_attention_fused(out.data_ptr(), qkv_in.data_ptr(), qkv_splits, qkv_n, None, 0, klen_d.data_ptr(), B,
                                                        Hq, r.softmax_scale(tier, D), splits, ws.data_ptr(), dc.view(LAYER), st()))
                what = f'fused bits {bits} tier {tier} qkv_splits {qkv_splits} splits {splits}'
                got_pool = dc.download()
                assert np.array_equal(got_pool, full), f'{what}: cache bytes differ in {np.count_nonzero(got_pool != full)} positions'
                _assert_bits(host(out), case, what)
                n_cmp += 1
    print(f'[attention exact] fused prologue bits {bits}: {n_cmp} launches, all bits equal')


# ---- prefill --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', r.GROUPS_PREFILL)
@pytest.mark.parametrize('D', [128, 64])
def test_prefill_attention_exact(tm, cuda, D, group):
    """GQA groups 1, 2, 4, 6, 7 (G = 1, 2, 4, 2, 1 query heads per wave); K rows past k_len hold NaN, the V^T tail is zero"""
    n_cmp = 0
    for shape in r.PREFILL_SHAPES:
        for tier in 'AB':
            case = r.prefill_case(D, group, tier, shape)
            qlens, Hq, Hkv = shape[0], case.Hq, case.Hkv
            klen, B = case.klen, len(case.seqs)
            koff = np.concatenate([[0], np.cumsum([((k + 63) // 64) * 64 for k in klen])]).astype(np.int32)
            stride = int(koff[-1])
            cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
            T = int(cu[-1])
            q = np.concatenate([s.q.reshape(len(s.q), -1) for s in case.seqs])
            K = np.full((Hkv, stride, D), np.nan, f16)    # garbage past the context must be masked, not multiplied
            Vt = np.zeros((Hkv, D, stride), f16)
            for b, s in enumerate(case.seqs):
                K[:, koff[b]:koff[b] + s.n] = s.K
                Vt[:, :, koff[b]:koff[b] + s.n] = s.V.transpose(0, 2, 1)
            out = torch.full((T, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
            _ffi.check(tm.tm_prefill_attention_hd(out.data_ptr(), dev(q).data_ptr(), Hq * D, dev(K).data_ptr(), dev(Vt).data_ptr(), stride,
                                                  dev(cu).data_ptr(), dev(koff).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), B,
                                                  max(qlens), Hq, Hkv, D, r.softmax_scale(tier, D), st()))
            got = host(out).view(np.uint16).copy()
            got[got == 0x8000] = 0
            for b, s in enumerate(case.seqs):
                g = got[cu[b]:cu[b + 1]].reshape(s.bits.shape)
                bad = (g != s.bits) & ~s.loose
                what = f'prefill head_dim {D} group {group} tier {tier} q_lens {qlens} sequence {b}'
                assert not bad.any(), (f'{what}: {int(bad.sum())} outputs differ, first (row, head, channel) {tuple(np.argwhere(bad)[0])}: '
                                       f'got {g[bad][0]:#06x}, expected {s.bits[bad][0]:#06x}')
                assert r.ulp16(g, s.bits)[s.loose].max(initial=0) <= 1, what
            n_cmp += 1
    print(f'[attention exact] prefill head_dim {D} group {group}: {n_cmp} launches, all bits equal')
