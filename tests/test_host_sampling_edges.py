"""CPU proof of tests/sampling_edges_reference.py: the bin model over all 65536 fp16 patterns, that every constructed cut lands in the
bin, thread and wave it claims, every margin, and that each boundary case tells the right rule from its neighbours.  What the GPU
module (tests/test_gpu_sampling_edges.py) compares with the oracle is exactly what is proved here."""
import numpy as np
import pytest

from tests import sampling_edges_reference as R

f16, f32 = np.float16, np.float32
ALL = np.arange(65536, dtype=np.int64)


def _sampler_calls():
    """every tm_sample call the GPU module makes, by section"""
    return {'2 boundary rows': [R.boundary_call(n) for n in R.BOUNDARY_SETS],
            '3A small vocabularies': [R.small_vocab_call(*s) for s in R.SMALL_VOCABS],
            '3B large vocabularies': [R.big_vocab_call(*s) for s in R.BIG_VOCABS],
            '4 logprobs boundaries': [R.logprobs_call(C) for C in R.LP_CAPS],
            '5 degenerate rows': [R.degenerate_call()[1]],
            '6 workspace reuse': list(R.reuse_calls()[:3])}


# ------------------------------------------------------------------------------------------------
# bin model
# ------------------------------------------------------------------------------------------------
def test_bin_model_over_all_patterns():
    val = R.value_of_bits(ALL.astype(np.uint16)).astype(np.float64)
    nan = np.isnan(val)
    key, j = R.key_of(ALL), R.desc_bin(ALL)
    assert key.min() == 0 and key.max() == key[0x7c00] == 0xfc00 and np.array_equal(j, 65535 - key)     # +inf is highest
    assert (key[nan] == 0).all() and (key[~nan] > 0).all() and (j[nan] == 65535).all()          # NaN is lowest, alone in its bin
    order = np.argsort(key[~nan], kind='stable')
    v, k = val[~nan][order], key[~nan][order]
    assert (np.diff(v) >= 0).all()                                                             # order preserving ...
    assert np.array_equal(np.diff(v) > 0, np.diff(k) > 0)                                      # ... strictly: equal key <=> equal value
    assert key[0x0000] == key[0x8000] == 0x8000 and j[0x8000] == j[0x0000] == 32767            # +-0 merge
    assert 32768 not in set(j.tolist()), 'bin 32768 (the slot of -0.0) is never populated'
    pos, neg = ALL[(ALL < 0x8000) & ~nan], ALL[(ALL > 0x8000) & ~nan]
    assert np.array_equal(j[pos], 0x7fff - pos) and np.array_equal(j[neg], 0x8000 + (neg & 0x7fff))
    back = R.value_of_bits(R.bits_of_bin(j)).astype(np.float64)                                # the inverse returns the value
    assert np.array_equal(back[~nan], val[~nan]) and np.isnan(back[nan]).all()
    t, q, w = R.owner(ALL)
    assert np.array_equal(t, j // 64) and np.array_equal(q, j % 64) and np.array_equal(w, j // 4096) and t.max() == 1023
    assert j[0x7c00] == 1023 and j[0x7bff] == 1024 and j[0xfbff] == 64511 and j[0xfc00] == 64512


@pytest.mark.parametrize('name', list(R.BOUNDARY_SETS))
def test_boundary_sets_sit_where_the_table_says(name):
    firsts = [s if isinstance(s, int) else s[0] for s in R.BOUNDARY_SETS[name]]
    vals = R.value_of_bits(np.asarray(firsts, np.uint16))
    for a, b in zip(vals[:-1], vals[1:]):                                  # four ADJACENT values, descending
        with np.errstate(over='ignore'):
            assert np.nextafter(a, f16(-np.inf)) == b or (a == 0 and b == -f16(2.0**-24))
    for g, j, t, q, w in R.BOUNDARY_OWNERS[name]:
        assert int(R.desc_bin(firsts[g])) == j and tuple(int(x) for x in R.owner(firsts[g])) == (t, q, w)
        assert (t, q, w) == (j // 64, j % 64, j // 4096)
    if name == 'sign':
        assert R.BOUNDARY_SETS[name][2] == (0x0000, 0x8000) and int(R.desc_bin(0x8000)) == 32767
    T = R.boundary_temperature(name)
    assert np.log2(T) == np.round(np.log2(T)) and f32(T) == T
    w = R._group_weights(name, T)
    live = w[w > 0]
    ratio = (live[1:] / live[:-1]).astype(np.float64)
    assert ((ratio >= 0.9) & (ratio <= 0.99)).all(), ratio
    row, grp = R.boundary_row(name)
    assert row.shape == (64,) and np.bincount(grp).tolist() == [16] * 4
    assert (np.diff(np.flatnonzero(grp == 0)) > 1).any(), 'ids are scrambled'
    bits = row.view(np.uint16)
    for g, s in enumerate(R.BOUNDARY_SETS[name]):
        assert set(bits[grp == g].tolist()) == ({s} if isinstance(s, int) else set(s))
    call = R.boundary_call(name)
    assert call.V == call.ld == 64 and (call.logits.view(np.uint16) == bits).all() and (call.temperature == f32(T)).all()


@pytest.mark.parametrize('name', list(R.BOUNDARY_SETS))
def test_boundary_cuts_land_in_the_bin_they_claim(name):
    call = R.boundary_call(name)
    row, grp = R.boundary_row(name)
    firsts = [s if isinstance(s, int) else s[0] for s in R.BOUNDARY_SETS[name]]
    kinds = [c[0] for c in call.claims]
    assert [int(k) for k, c in zip(call.top_k, kinds) if c == 'top_k'] == list(R.BOUNDARY_TOP_KS)
    assert kinds.count('top_p') + kinds.count('off') == 4 and kinds.count('min_p') == 4 and kinds.count('combined') == 1
    assert kinds.count('u') == (10 if name != 'bottom' else 8)             # bottom: the -inf group is never drawn
    assert (call.min_p[[k == 'min_p' for k in kinds]] == 1.0).sum() == 1
    for b, ((ids, p, tok), (kind, g, n)) in enumerate(zip(call.expected(), call.claims)):
        if kind == 'u':                                                    # member n of group g, in id order
            assert len(ids) == 64 and grp[tok] == g and np.flatnonzero(grp == g)[n] == tok, (b, call.tags[b])
            continue
        assert len(ids) == n, (b, call.tags[b], len(ids), n)
        cut = ids[-1]                                                      # the last survivor sits in the claimed group ...
        assert grp[cut] == g, (b, call.tags[b])
        want = tuple(int(x) for x in R.owner(firsts[g]))                   # ... hence in its bin, thread and wave
        assert tuple(int(x) for x in R.owner(row.view(np.uint16)[cut])) == want
        assert tok == ids[p > 0][-1], 'u = 1 - 2^-24 draws the last survivor with a non-zero weight'
    if name == 'bottom':                                                   # zero weight, still counted by top-k
        k63 = list(R.BOUNDARY_TOP_KS).index(63)
        ids, p, tok = call.expected()[k63]
        assert len(ids) == 63 and p[-1] == 0 and grp[ids[-1]] == 3 and grp[tok] == 2


@pytest.mark.parametrize('name', list(R.BOUNDARY_SETS))
def test_boundary_cases_tell_the_rule_from_its_neighbours(name):
    """ties by descending id, and a cut (or a draw) one candidate earlier or later, each give another (kept, token)"""
    call = R.boundary_call(name)
    for b, (ids, p, tok) in enumerate(call.expected()):
        rivals = R.rival_outcomes(call, b)
        assert 'ties by descending id' in rivals and len(rivals) >= 2, (b, call.tags[b])
        for what, outcome in rivals.items():
            assert outcome != (len(ids), tok), f'{call.tags[b]}: "{what}" gives the same (kept, token) {outcome}'


# ------------------------------------------------------------------------------------------------
# margins
# ------------------------------------------------------------------------------------------------
def test_margins_longdouble_restates_the_oracle():
    """margins() must walk the same pipeline as o.sample_filter: same survivors at every row it is used on"""
    for calls in _sampler_calls().values():
        for c in calls[:2]:
            for b in range(c.B):
                cand, z, p, cum = R._profile(c.logits[b, :c.V], c.temperature[b], c.top_k[b])
                ids = c.expected()[b][0]
                assert np.array_equal(cand[:len(ids)], ids), (c.name, b)
    row = np.asarray([2.0, 1.0, 1.0, 0.0], f16)                            # p = .5761, .2119, .2119, .0780
    d_p, d_m, d_u = R.margins(row, 1.0, 0, 0.6, 0.3, 0.5)
    p = np.exp(np.asarray([0, -1, -1, -2.0]))
    p /= p.sum()
    assert abs(d_p - min(abs(np.cumsum(p) - f32(0.6)))) < 1e-12
    assert abs(d_m - abs(p[1] / p[0] - f32(0.3))) < 1e-12                  # top_p keeps two, the maximum itself is left out
    assert abs(d_u - abs(p[0] / (p[0] + p[1]) - 0.5)) < 1e-12              # the survivors' total decides nothing


def test_every_margin_holds():
    """all margins >= 64 V 2^-53; min_p and the all-defaults rows' u >= 2^-20 too; a moved parameter moved <= 16 float32 steps"""
    for section, calls in _sampler_calls().items():
        for c in calls:
            assert c.margins.shape == (c.B, 3)
            for b in range(c.B):
                for what, m, need in zip(('top_p', 'min_p', 'u'), c.margins[b], c.floors(b)):
                    assert need >= R.floor_of(c.V)
                    assert m >= need, f'{c.name} row {b} ({c.tags[b]}): {what} margin {m:.3e} < {need:.3e}'
                assert 0.0 <= c.u[b] < 1.0
        rows, ratio, m, need = R.margin_report(calls)
        print(f'section {section}: {rows} rows, {sum(c.nudges for c in calls)} parameters moved, smallest margin {m:.3e} against {need:.3e}')


def test_margin_rule_moves_a_parameter_that_sits_on_a_boundary():
    row = np.zeros((2, 8), f16)                                            # eight equal candidates: cumulative sums k / 8
    c = R._make('probe', 8, 8, row, [dict(top_p=0.5, u=0.9), dict(top_k=8, u=0.25)])
    assert c.nudges == 2 and c.top_p[0] == np.nextafter(f32(0.5), f32(1)) and c.u[1] == np.nextafter(f32(0.25), f32(1))
    assert (c.margins >= np.asarray([c.floors(0), c.floors(1)])).all()
    c = R._make('probe', 8, 8, row[:1], [dict(u=0.25)])                    # an all-defaults row needs 2^-20: out of reach in 16 steps,
    assert c.nudges == 0 and c.u[0] == 0.25 and c.margins[0, 2] == 0       # the nominal value stays and the margin test reports it


# ------------------------------------------------------------------------------------------------
# the other inputs
# ------------------------------------------------------------------------------------------------
def test_no_compared_row_mixes_nan_and_minus_inf():
    for calls in _sampler_calls().values():
        for c in calls:
            x = c.logits[:, :c.V]
            assert not np.isnan(x).any(), c.name
    gpu, ref, proper = R.degenerate_call()
    for b in proper:
        x = gpu.logits[b]
        assert not (np.isnan(x).any() and np.isneginf(x).any()), b


def test_vocabulary_cases():
    assert R.SMALL_VOCABS == ((1, 8), (5, 8), (7, 8), (8, 8), (9, 16), (1023, 1024), (1024, 1024), (1025, 1032), (2049, 2056))
    for V, ld in R.SMALL_VOCABS:
        c = R.small_vocab_call(V, ld)
        assert c.B == 8 and c.u[0] == 0 and c.u[7] == R.U_LAST and (c.logits[:, V:] == 100).all()
        assert (c.logits[2, :V] == 1.5).all() and (V < 3 or np.isneginf(c.logits[0, 1])) and (V < 4 or c.logits[0, 0] == c.logits[0, V - 1])
        assert c.temperature[6] == 0 and c.temperature[7] == -1 and c.top_p[4] == 0 and c.top_k[1] == 1 and c.top_k[2] == 3
    assert R.BIG_VOCABS == ((151936, 152064), (137221, 137224)) and 137221 == R.SECOND_TRIP + 3 * 2048 + 5
    for V, ld in R.BIG_VOCABS:
        c = R.big_vocab_call(V, ld)
        e = c.expected()
        assert c.B == 15 and (c.logits[:, V:] == 100).all()
        flat = len(e[R.BIG_FLAT_ROW][0])
        assert flat == int(np.floor(np.float64(f32(0.3)) * V)) + 1         # one bin of V members
        ids, p, tok = e[R.BIG_HIGH_ROW]
        assert (ids[:11] >= R.SECOND_TRIP).all() and ids[0] == R.SECOND_TRIP and ids[1] == V - 1 and tok >= R.SECOND_TRIP
        ids, p, tok = e[R.BIG_TAIL_ROW]
        assert int(np.flatnonzero(ids == tok)[0]) >= 1024                  # tail_draws > 0 at both caps
        assert sum(x[2] >= R.SECOND_TRIP for x in e) >= 1


@pytest.mark.parametrize('C', R.LP_CAPS)
def test_logprobs_rows_hit_the_positions_they_claim(C):
    c = R.logprobs_call(C)
    assert (c.V, c.ld) == (1100, 1104)
    seen = set()
    for b, ((ids, p, tok), (kept, nA, pos)) in enumerate(zip(c.expected(), c.claims)):
        assert len(ids) == kept, (b, len(ids), kept)
        L = min(kept, C)
        bins = R.desc_bin(c.logits[b, :c.V].view(np.uint16)[ids[:L]])
        got_nA = int((bins < bins[-1]).sum())
        assert got_nA == nA, (b, got_nA, nA)
        n_cut = int((R.desc_bin(c.logits[b, :c.V].view(np.uint16)) == bins[-1]).sum())
        seen.add(('kept', kept - C) if kept <= C + 1 else ('nA', 'none' if nA == 0 else nA - C, 'bin ends at the cap' if nA + n_cut == L else 'bin goes on'))
        if pos is not None:
            assert int(np.flatnonzero(ids == tok)[0]) == pos
            seen.add(('draw', pos))
    want = {('kept', 0), ('kept', 1), ('nA', 'none', 'bin ends at the cap'), ('nA', 'none', 'bin goes on')}
    if C > 1:
        want |= {('kept', -1), ('nA', -1, 'bin goes on')}
        assert any(s[0] == 'nA' and s[1] not in ('none', -1) and s[2] == 'bin ends at the cap' for s in seen)   # two groups sum to C
    if C == 1024:
        want |= {('draw', 1023), ('draw', 1024)}
    if C == 5:
        want |= {('draw', 700)}
    assert want <= seen, want - seen


def test_degenerate_batch():
    gpu, ref, proper = R.degenerate_call()
    assert gpu.B == 8 and list(R.DEGENERATE_LAYOUT).count('ordinary') == 3 and proper == [0, 3, 5, 6, 7]
    x = gpu.logits
    assert np.isnan(x[1]).all() and np.isposinf(x[2, 17]) and np.isneginf(x[4]).all() and np.isnan(x[5, ::2]).all()
    assert np.isnan(np.delete(x[7], 777)).all() and x[7, 777] == -3
    fin = np.where(np.isfinite(x[2]), x[2], -np.inf)
    assert R.DEGENERATE_TOKENS[2] == int(np.argmax(fin)) == 300            # arg-max over the finite logits, lowest id on the tie
    assert ref.expected()[proper.index(7)][2] == R.DEGENERATE_TOKENS[7] == 777


def test_processor_inputs():
    for V, ld, off, vocab in R.SHARD_CASES:
        assert off % 8 == 0 and off + V <= vocab and (off == 0 or off % 32 == 16) and (off == 0 or V == vocab // 8)
    cu_q, ids, per_seq, vocab, words = R.packed_seen_case()
    assert [len(s) for s in per_seq] == [0, 5, 0, 4, 0] and vocab % 32
    for t in range(len(ids)):                                              # "last r with cu_q[r] <= t" over r < nseq
        r = max(r for r in range(5) if cu_q[r] <= t)
        assert cu_q[r] <= t < cu_q[r + 1]
    want = R.mask_of(per_seq, words, vocab)
    assert not want[[0, 2, 4]].any() and want[1, 0] == 1 << 31 and want[1, 1] == 1 and want[3, (vocab - 1) >> 5] == 1 << ((vocab - 1) & 31)
    assert np.count_nonzero(want) == 4
    for name, V, ld, off, vocab, x, rows in R.process_edge_cases():
        ref = R.process_expected(x, V, off, rows)
        if name == 'penalty values':
            n = len(R.PENALTY_BITS)
            for r, out, src in zip(rows, ref, x):
                if r['p'] in (1.0, 0.0, -1.0):
                    assert R.same_bits_or_nan(out, src[:V])
                assert R.same_bits_or_nan(out[n:2 * n], src[n:2 * n])      # not seen
            half, two = ref[0].view(np.uint16)[:n], ref[1].view(np.uint16)[:n]
            assert half.tolist()[:8] == [0x0000, 0x8000, 0x0002, 0x8000, 0x7c00, 0xf7ff, 0x7c00, 0xfc00] and np.isnan(ref[0][8])
            assert two.tolist()[:8] == [0x0000, 0x8000, 0x0000, 0x8002, 0x77ff, 0xfc00, 0x7c00, 0xfc00]
        if name == 'shard+16':
            assert R.same_bits_or_nan(ref[0], x[0, :V]), 'ids 15 and 16 + 4096 lie outside the shard'
            assert np.flatnonzero(ref[1] != x[1, :V]).tolist() == [0, V - 1]
        if name == 'edges':
            assert np.flatnonzero(ref[0] != x[0, :V]).tolist() == [2047, 2048, 4096, 4098]
            assert (ref[1][[2047, 4098]] == -65504).all(), 'the ban wins over the penalty'
