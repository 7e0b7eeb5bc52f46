"""tests/turboquant_select_reference.py on the host: its conditions hold for every case the GPU module launches, a float32 numpy model
of the kernel's rotated-domain attention returns the expected rows within half the bound, and the same model with one deliberate fault
(a context off by one, the neighbour's params, exchanged heads, the other kv head's cache, a dropped split, a dropped wave, a
never-written split slot read as zeros) misses the bound by more than a factor 4 -- the proof that tests/test_gpu_turboquant_select.py
would fail if attention_decode_tq.hip were subtly wrong.

The model follows the kernel's structure, not its lanes: q' = fp16(fp32(H q) / sqrt(128)); k^ = fp16(fma(+-1, g, c3h[idx])) from the
kernel's fp16 centroid tables; S = fp32(k^ . q') * n; online softmax over 32-token tiles, newest to oldest, the tiles of a split dealt
to four waves from its newest tile on, p rounded to fp16 for the value side; a merge of the four waves, a merge of the split slots,
o / l, the rotation back.  It returns fp32: the fp16 rounding of the output is the other half of the bound."""
import re

import numpy as np
import pytest

from tests import turboquant_reference as tq
from tests import turboquant_select_reference as r

f16, f32, f64 = np.float16, np.float32, np.float64
C3H = np.array([0xb216, 0xaf9a, 0xac47, 0xa58c, 0x258c, 0x2c47, 0x2f9a, 0x3216], np.uint16).view(f16)   # attention_decode_tq.hip
C2H = np.array([0xbe0b, 0xb73f, 0x373f, 0x3e0b], np.uint16).view(f16)
FAULTS = ('ctx_plus_1', 'ctx_minus_1', 'k_params_of_neighbour', 'v_norm_of_neighbour', 'heads_exchanged', 'kv_head_0_for_1',
          'last_split_dropped', 'wave_3_dropped', 'unwritten_slot_reads_zero')
CASE_IDS = [f'group{g}' for g in r.GROUPS] + ['sweep']


def _case(cid):
    return r.build(r.SWEEP_GROUP, True) if cid == 'sweep' else r.build(int(cid[5:]))


def _exp2(x):
    with np.errstate(under='ignore', invalid='ignore'):
        return np.exp2(x.astype(f32)).astype(f32)


def _merge(ms_all, l_all, o_all):
    """slots [n, G], [n, G], [n, G, D] -> (m, l, o): the kernel's merge of waves and of splits (fmaxf ignores a NaN, -inf weighs 0)"""
    with np.errstate(invalid='ignore'):
        ms = np.fmax.reduce(np.concatenate([np.full_like(ms_all[:1], -np.inf), ms_all]), 0)
        wt = np.where(ms_all == -np.inf, f32(0), _exp2((ms_all - ms) * r.SC))
        return ms, (wt * l_all).sum(0, dtype=f32), (wt[..., None] * o_all).sum(0, dtype=f32)


def model(case, splits, fault=None):
    """-> per sequence float32 [Hq, D]"""
    G = case.group
    hpw, _ = r.hpw_chunks(G)
    outs = []
    for s in case.seqs:
        ctx = {'ctx_plus_1': min(s.ctx + 1, s.nalloc), 'ctx_minus_1': s.ctx - 1}.get(fault, s.ctx)
        tiles = (ctx + r.TILE - 1) // r.TILE
        per = (tiles + splits - 1) // splits if tiles else 0
        out = np.empty((case.Hq, r.D), f32)
        for kv in range(r.HKV):
            src = 0 if fault == 'kv_head_0_for_1' else kv
            kpar, vpar = s.kpar[src], s.vpar[src]
            if fault == 'k_params_of_neighbour':
                kpar = np.roll(kpar, -1, 0)
            if fault == 'v_norm_of_neighbour':
                vpar = np.roll(vpar, -1, 0)
            kc = s.kcodes[src]
            kh = (C3H[kc & 7].astype(f64) + np.where(kc & 8, 1.0, -1.0) * kpar[:, 1:2].astype(f64)).astype(f16)   # one fp16 fma
            qr = r.rotate_q(s.q[kv * G:(kv + 1) * G])
            # every product is an fp32 number and so is every partial sum of a live row in the kernel's order: the float64 sum is it
            S = (kh.astype(f64) @ qr.astype(f64).T).astype(f32) * kpar[:, :1].astype(f32)                          # [nalloc, G]
            vn = vpar[:, 0].astype(f32) * r.RSQRT_D
            vc = C2H[s.vcodes[src]].astype(f32)
            slot_m = np.full((splits, G), np.nan, f32)                 # the workspace as the tests leave it: never zeroed
            slot_l = np.full((splits, G), np.nan, f32)
            slot_o = np.full((splits, G, r.D), np.nan, f32)
            nonempty = [sp for sp in range(splits) if sp * per < min((sp + 1) * per, tiles)]
            for sp in range(splits):
                t0, t1 = sp * per, min((sp + 1) * per, tiles)
                if t0 >= t1 and fault == 'unwritten_slot_reads_zero':
                    slot_m[sp], slot_l[sp], slot_o[sp] = 0, 0, 0
                    continue
                if fault == 'last_split_dropped' and splits > 1 and nonempty and sp == nonempty[-1]:
                    slot_m[sp], slot_l[sp], slot_o[sp] = -np.inf, 0, 0
                    continue
                wm = np.full((4, G), -np.inf, f32)
                wl = np.zeros((4, G), f32)
                wo = np.zeros((4, G, r.D), f32)
                for tile in range(t1 - 1, t0 - 1, -1):
                    w = (t1 - 1 - tile) % 4
                    if fault == 'wave_3_dropped' and w == 3:
                        continue
                    tok = slice(tile * r.TILE, min((tile + 1) * r.TILE, ctx))
                    St = S[tok]
                    with np.errstate(invalid='ignore'):
                        mnew = np.maximum(wm[w], St.max(0))
                        alpha = np.where(wm[w] == -np.inf, f32(0), _exp2((wm[w] - mnew) * r.SC))
                    wl[w] *= alpha
                    wo[w] *= alpha[:, None]
                    wm[w] = mnew
                    p = _exp2(St * r.SC - mnew * r.SC)                                                            # [nt, G]
                    wl[w] += p.sum(0, dtype=f32)
                    wo[w] += (p.astype(f16).astype(f32) * vn[tok, None]).T @ vc[tok]
                slot_m[sp], slot_l[sp], slot_o[sp] = _merge(wm, wl, wo)
            if splits == 1:
                l, o = slot_l[0], slot_o[0]
            else:
                _, l, o = _merge(slot_m, slot_l, slot_o)
            with np.errstate(divide='ignore', invalid='ignore'):
                rows = ((o / l[:, None]).astype(f64) @ r.H).astype(f32) * r.RSQRT_D
            if fault == 'heads_exchanged':
                for h0 in range(0, G, hpw):
                    for h in range(h0, h0 + hpw - 1, 2):
                        rows[[h, h + 1]] = rows[[h + 1, h]]
            out[kv * G:(kv + 1) * G] = rows
        outs.append(out)
    return outs


def _worst(case, outs):
    return max(r.ratios(case, b, o).max() for b, o in enumerate(outs))


# ------------------------------------------------------------------------------------------------------------------------------------
def test_centroid_tables():
    """the fp16 bit patterns the kernel's v_perm tables hold are the rounded centroids of the contract"""
    assert np.array_equal(C3H.view(np.uint16), (tq.C3.astype(f64) / np.sqrt(128.0)).astype(f16).view(np.uint16))
    assert np.array_equal(C2H.view(np.uint16), tq.C2.astype(f16).view(np.uint16))
    assert float(r.rotate_q(np.eye(1, r.D, 5, dtype=f16) * r.QMAG)[0, 0]) == 181.0
    assert abs(float(r.SC) - np.log2(np.e) / np.sqrt(128)) < 1e-8 and r.DEAD_GAP < 128 * 181 * float(C3H[7])


@pytest.mark.parametrize('cid', CASE_IDS)
def test_conditions(cid):
    """build() asserts the conditions of the construction; here what the issue's table of cases promises on top of them"""
    case = _case(cid)
    hpw, chunks = r.hpw_chunks(case.group)
    assert hpw * chunks == case.group and (hpw, chunks) == {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (4, 1), 5: (1, 5), 6: (3, 2), 7: (1, 7),
                                                            8: (4, 2), 10: (2, 5)}[case.group]
    assert case.klen == (list(r.CONTEXTS) if cid != 'sweep' else [r.SWEEP_CTX] * len(r.SWEEP_SHIFTS))
    assert case.redraws < 0.01 * case.rows
    zero_live = 0
    for s in case.seqs:
        assert s.nalloc == -(-s.ctx // 64) * 64
        for kv in range(r.HKV):
            vn = s.vpar[kv, :s.ctx, 0]
            assert len(set(vn.tolist())) == s.ctx and vn.max() <= 4 and np.sort(vn)[1 if (vn == 0).any() else 0] >= 0.25
            assert (s.vpar[kv, s.ctx:, 0] == r.LOOK_N).all() and (s.kpar[kv, s.ctx:, 0] == r.LOOK_N).all()
            assert set(np.unique(s.vcodes[kv])) == {0, 1, 2, 3}
            zero_live += sum(int((s.vpar[kv, s.live[kv * case.group + h], 0] == 0).any()) for h in range(case.group))
        S = r.scores(s, case.group)
        for h in range(case.Hq):
            live = s.live[h]
            assert len(set(S[h, live].tolist())) == 1 and 1 <= len(live) <= r.MAX_LIVE
            if h % case.group < s.nalloc - s.ctx:      # its row behind the context would dominate: 64 / n x the live score
                assert S[h, s.ctx:].max() >= abs(S[h, live[0]]) * 16
    assert zero_live >= 1, 'no live token with V norm 0'
    # 16 splits: every sequence but the longest has splits without a tile, the longest has per_split = 3 and splits 12 .. 15 empty
    if cid != 'sweep':
        assert [r.where(1089, t, 16)[2] for t in (0, 1088)] == [0, 11] and r.where(1089, 1088, 1)[:2] == (34, 0)


def test_sweep_covers_context_300():
    covered = r.coverage_300()
    assert covered.all(), f'positions of context 300 never live for one head and dead for another: {np.flatnonzero(~covered).tolist()}'


@pytest.mark.parametrize('cid', CASE_IDS)
def test_model_meets_expected(cid):
    case = _case(cid)
    for splits in r.SPLITS:
        worst = _worst(case, model(case, splits))
        print(f'{case.name} splits {splits}: model worst err / bound {worst:.3f}')
        assert worst <= 0.5, f'{case.name} splits {splits}: the float32 model is {worst:.3f} x the bound from the expected rows'


@pytest.mark.parametrize('fault,kind,wave', [('wave_3_dropped', 'removing live', 3), ('ctx_plus_1', 'adding the row behind the context', 0)])
def test_failure_message_names_the_token(fault, kind, wave):
    """explain() on the rows of a faulted model: the token it names is one the fault lost or let in, with its tile, wave and split"""
    case, splits = r.build(4), 2
    outs = model(case, splits, fault)
    named = 0
    for b, s in enumerate(case.seqs):
        ratio = r.ratios(case, b, outs[b])
        for h in np.flatnonzero((ratio > 4) & np.isfinite(ratio)):
            if fault == 'wave_3_dropped' and len(s.live[h]) == 1:
                continue                               # its only token lost: the row is the mean of the dead ones, no single-token change
            msg = r.explain(case, b, h, outs[b][h], splits)
            assert f'live set {s.live[h].tolist()}' in msg and 'got' in msg and 'expected' in msg
            tok = int(re.search(r'token (\d+) \(tile', msg).group(1))
            assert kind in msg and f'wave {wave}, ' in msg, msg
            assert (tok in s.live[h]) == (kind == 'removing live') and tok == (s.ctx if fault == 'ctx_plus_1' else tok)
            named += 1
    assert named >= 3


@pytest.mark.parametrize('fault', FAULTS)
def test_model_with_fault_misses(fault):
    """every fault is seen, and seen at every GQA group whose launch can have it"""
    for cid in CASE_IDS:
        case = _case(cid)
        hpw, _ = r.hpw_chunks(case.group)
        if fault == 'heads_exchanged' and hpw == 1:
            continue
        splits = {'unwritten_slot_reads_zero': 16, 'last_split_dropped': 3}.get(fault, 2)
        if cid == 'sweep' and fault == 'unwritten_slot_reads_zero':
            continue                                   # context 300 only: every maximum is positive, a slot of zeros weighs 0
        ratio = np.concatenate([r.ratios(case, b, o) for b, o in enumerate(model(case, splits, fault))])
        finite = ratio[np.isfinite(ratio)].max()
        print(f'{fault}, {case.name} splits {splits}: {int((ratio > 4).sum())} of {ratio.size} (sequence, head) rows miss 4 x the bound, '
              f'{int(np.isinf(ratio).sum())} are not finite, worst finite err / bound {finite:.1f}')
        assert ratio.max() > 4, f'{fault} at {case.name}: the faulted model stays within {ratio.max():.2f} x the bound'
        if fault != 'unwritten_slot_reads_zero':       # (that one shows as 0 / 0 only); every other fault also as a wrong finite row
            assert finite > 4, f'{fault} at {case.name}: seen only as rows that are not finite'
