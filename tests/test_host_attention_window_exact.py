"""CPU proof of the window and sink cases of tests/attention_exact_reference.py, the operands of
tests/test_gpu_attention_window_exact.py.

Preconditions: every case the GPU module runs holds the builder's assertions (with the sink in the denominator and the window in the
visibility) and the 1-in-1000 cap on outputs compared at 1 ulp; the live sets sit where the window edges are; the batch of contexts
and windows reaches every residue of the window's first token that the decode kernel treats differently.
Order independence: the oracle's fp32 restatement of the online softmax on the cropped context, at 1, 2, 3 and 16 splits and tiles of
16 and 64 tokens, with the sink added once behind the merge, returns the expected bits; so does the prefill restatement row by row.
Sensitivity: every error of the window and sink arithmetic, and every error the exact suite already knows restricted to the window,
applied to the reference COMPUTATION, changes the expected bits in every case that has the feature; the number of changed
(sequence, head) pairs is printed."""
import numpy as np
import pytest

from oracle import tm_oracle as o
from tests import attention_exact_reference as r

f16, f32 = np.float16, np.float32
DECODE = list(r.decode_window_cases())
PREFILL = list(r.prefill_window_cases())
DB = [(128, 8), (128, 4), (128, 16), (64, 8), (64, 4), (64, 16)]


def _decode_of(D, bits):
    return [r.decode_window_case(*a) for a in DECODE if (a[1], a[0]) == (D, bits)]


def _prefill_of(D, W=None):
    return [r.prefill_window_case(*a) for a in PREFILL if a[0] == D and W in (None, a[4])]


def _wbeg(n, W):
    return max(n - W, 0)


# ---- preconditions --------------------------------------------------------------------------------------------------------------
def test_offsets_and_sink_values():
    """the offset channel holds an fp16 integer; neighbouring heads never share a sink weight; all four admissible logits occur"""
    for a in DECODE:
        case = r.decode_window_case(*a)
        assert case.q_off == {('A', 8): 256, ('A', 4): 256, ('A', 16): 256, ('B', 8): 251, ('B', 4): 218, ('B', 16): 251}[case.tier, case.bits]
        if case.sinks is not None:
            unit = case.sinks.astype(np.float64) == 0
            assert (unit[1:] != unit[:-1]).all()
            if case.Hq >= 4:
                assert {0x0000, 0x8000, 0xfc00, 0xfbff} == set(case.sinks.view(np.uint16).tolist())


def test_thinning_covers_every_axis():
    for D, bits in DB:
        mine = [a for a in DECODE if (a[1], a[0]) == (D, bits)]
        assert {a[2] for a in mine} == set(r.GROUPS_WINDOW) and {(a[4], a[3]) for a in mine} == {(W, t) for W in r.WINDOWS_DECODE for t in 'AB'}
        assert {(a[4], a[5]) for a in mine} == {(W, k) for W in r.WINDOWS_DECODE for k in (0, 1)}
        assert {(a[3], a[5]) for a in mine} == {(t, k) for t in 'AB' for k in (0, 1)}
    for g in r.GROUPS_WINDOW:
        assert {a[5] for a in DECODE if a[2] == g} == {0, 1}
    for D in (128, 64):
        mine = [a for a in PREFILL if a[0] == D]
        assert {a[1] for a in mine} == set(r.GROUPS_PREFILL) and {(a[4], a[3]) for a in mine} == {(W, s) for W in r.WINDOWS_PREFILL for s in r.PREFILL_SHAPES}
        for W in r.WINDOWS_PREFILL:
            assert {a[2] for a in mine if a[4] == W} == {'A', 'B'} and {a[5] for a in mine if a[4] == W} == {0, 1}
        for g in r.GROUPS_PREFILL:
            assert {a[5] for a in PREFILL if a[1] == g} == {0, 1}


def test_contexts_and_windows_reach_every_window_start():
    """(n, W) -> wbeg: the table of tests/test_gpu_attention_window_exact.py's docstring"""
    nw = [(n, W, _wbeg(n, W)) for n in r.KLEN_WINDOW for W in r.WINDOWS_DECODE]
    assert any(W == n and b == 0 for n, W, b in nw) and any(W > n for n, W, b in nw)
    assert any(b == 1 for n, W, b in nw) and 1 in r.WINDOWS_DECODE
    for res in (0, 1, 31):
        assert any(b > 0 and b % 32 == res for n, W, b in nw), res
    assert any(b > 0 and b % 64 == 0 for n, W, b in nw)
    assert any(b > 0 and b >= (n - 1) // 64 * 64 and n % 64 for n, W, b in nw)                       # inside the newest partial block
    for splits in (2, 3, 16):
        assert any(len(r.window_splits(n, W, splits)) < splits for n, W, b in nw)
    for W in r.WINDOWS_DECODE[:-1]:                            # the negative control needs a batch that starts inside every context
        assert [n for n in r.KLEN_WINDOW if n > W + 1]


@pytest.mark.parametrize('D,bits', DB)
def test_decode_cases_hold_the_builder_assertions(D, bits):
    for case in _decode_of(D, bits):
        assert sum(int(s.loose.sum()) for s in case.seqs) * 1000 <= case.total
        G, W = case.Hq // case.Hkv, case.window
        for s in case.seqs:
            _, _, _, extra = r.reference(case, s, detail=True)
            _, _, _, wider = r.reference(case, s, ('win_shift', -1), detail=True)
            b = _wbeg(s.n, W)
            for hd in range(case.Hkv):
                w = extra[hd][0]
                assert not w[:b].any() and not w[s.n:].any() and (w[b] > 0).all() and (w[s.n - 1] > 0).all()
                assert 1 <= (w > 0).sum(0).min() and (w > 0).sum(0).max() <= 32
                if b > 0:                                      # the token in front of the window looks live, with the top weight
                    assert (wider[hd][0][b - 1] == 2.0**r.JMAX).all() and (wider[hd][1][b - 1] <= 0).all()


@pytest.mark.parametrize('D', [128, 64])
def test_prefill_cases_hold_the_builder_assertions(D):
    for case in _prefill_of(D):
        assert sum(int(s.loose.sum()) for s in case.seqs) * 1000 <= case.total
        G, W = case.Hq // case.Hkv, case.window
        for s in case.seqs:
            _, _, _, extra = r.reference(case, s, detail=True)
            _, _, _, wider = r.reference(case, s, ('win_shift', -1), detail=True)
            R = s.q.shape[0]
            p = s.hist + np.arange(R)
            col = np.arange(R * G)
            for hd in range(case.Hkv):
                w = extra[hd][0]
                assert (w[np.repeat(p, G), col] > 0).all()                                             # the diagonal
                rows = np.flatnonzero(p - W >= 0)
                if len(rows):
                    cols = (rows[:, None] * G + np.arange(G)[None]).reshape(-1)
                    assert (w[np.repeat(p[rows] - W + 1, G), cols] > 0).all()                         # the window's first token
                    assert not w[np.repeat(p[rows] - W, G), cols].any()
                    assert (wider[hd][0][np.repeat(p[rows] - W, G), cols] > 0).all()                  # the one in front of it


def test_control_case_shows_what_the_device_controls_rely_on():
    """in the reference: W + 1 and W - 1 change every sequence; without the sinks exactly the heads with a sink of weight one change"""
    case = r.control_case()
    assert sum(int(s.loose.sum()) for s in case.seqs) * 1000 <= case.total and all(s.n > case.window + 1 for s in case.seqs)
    unit = case.sinks.astype(np.float64) == 0
    for s in case.seqs:
        for sh in (-1, +1):
            assert ((r.reference(case, s, ('win_shift', sh)) != s.bits) & ~s.loose).any()
        diff = ((r.reference(case, s, ('no_sink', None)) != s.bits) & ~s.loose).any((0, 2))
        assert diff[unit].all() and not diff[~unit].any()


# ---- order independence ---------------------------------------------------------------------------------------------------------
def _bits(x):
    b = np.asarray(x, f16).view(np.uint16).copy()
    b[b == 0x8000] = 0
    return b


def _restated(q, K, V, scale, splits, tile, sinks):
    """o.decode_attention; with sinks, the same from its parts (o.split_ranges, o.attention_tiles, the merge of o.attention_merge)
    with the sink's exp2(f32(sink) * 1.4426950408889634f - m * c) added to the merged denominator once, all in float32"""
    if sinks is None:
        return o.decode_attention(q, K, V, scale, splits, tile)
    Hq, D = q.shape
    G = Hq // K.shape[0]
    c = f32((1.0 / np.sqrt(D) if scale is None else scale) * np.log2(np.e))
    out = np.zeros((Hq, D), f16)
    for g in range(K.shape[0]):
        parts = [o.attention_tiles(q[g * G:(g + 1) * G], K[g], V[g], c, tile, a, b) for a, b in o.split_ranges(K.shape[1], splits, tile) if b > a]
        Ms = np.stack([p[1] for p in parts])
        mstar = Ms.max(0)
        w = o._exp2f((Ms - mstar[None]) * c)
        Lt = sum(w[i] * parts[i][2] for i in range(len(parts))).astype(f32)
        Ot = sum(w[i][:, None] * parts[i][0] for i in range(len(parts))).astype(f32)
        with np.errstate(over='ignore', invalid='ignore'):
            Lt = (Lt + o._exp2f(sinks[g * G:(g + 1) * G].astype(f32) * r.LOG2E - mstar * c)).astype(f32)
        out[g * G:(g + 1) * G] = (Ot / Lt[:, None]).astype(f16)
    return out


@pytest.mark.parametrize('D,bits', DB)
def test_decode_restatement_is_order_independent(D, bits):
    for case in _decode_of(D, bits):
        scale = None if case.tier == 'A' else float(r.SCALE_B)
        for s in case.seqs:
            b = _wbeg(s.n, case.window)
            K, V = s.K[:, b:s.n], s.V[:, b:s.n]
            for tile in (16, 64):
                for splits in (1, 2, 3, 16):
                    got = _bits(_restated(s.q[0], K, V, scale, splits, tile, case.sinks))
                    assert np.array_equal(got, s.bits[0]), (case.window, case.tier, s.n, tile, splits)


@pytest.mark.parametrize('W', r.WINDOWS_PREFILL)
def test_prefill_restatement_is_order_independent(W):
    """o.prefill_attention on every row's crop (the row is the crop's newest token); with sinks the same walk with the sink joined"""
    for case in _prefill_of(128, W) + _prefill_of(64, W):
        scale = None if case.tier == 'A' else float(r.SCALE_B)
        for s in case.seqs:
            for i in range(len(s.q)):
                p = s.hist + i
                b = _wbeg(p + 1, W)
                K, V = s.K[:, b:p + 1], s.V[:, b:p + 1]
                for tile in (16, 64):
                    if case.sinks is None:
                        got = _bits(o.prefill_attention(s.q[i:i + 1], K, V, p - b, scale, tile)[0])
                    else:
                        got = _bits(_restated(s.q[i], K, V, scale, 1, tile, case.sinks))
                    assert np.array_equal(got, s.bits[i]), (W, case.tier, s.n, i, tile)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
def _changed(case, muts_of):
    """(number of (sequence, head) pairs whose expected bits change under any of the mutations muts_of(s), whether a rescale was
    there to be skipped)"""
    n, skipped = 0, False
    for s in case.seqs:
        hit = np.zeros(case.Hq, bool)
        for mut in muts_of(s):
            bits, _, _, extra = r.reference(case, s, mut, detail=True)
            hit |= (bits != s.bits).any((0, 2))
            skipped |= extra.get('skipped', False)
        n += int(hit.sum())
    return n, skipped


def _tile_muts(case, which, factor):
    """the first / last 32-token tile of every non-empty split of the window"""
    def muts(s):
        out = set()
        for splits in (2, 3, 16):
            for a, b in r.window_splits(s.n, case.window, splits):
                out.add((a, min((a // 32 + 1) * 32, b), factor) if which == 'first' else (max((b - 1) // 32 * 32, a), b, factor))
        return [('tile_factor', x) for x in sorted(out)]
    return muts


def _split_max_differs(case):
    """a head with a sink of weight one has, at some split count, a non-empty split whose own maximum lies below the merged one"""
    G = case.Hq // case.Hkv
    unit = case.sinks.astype(np.float64) == 0
    for s in case.seqs:
        for hd in range(case.Hkv):
            Kq = r._units(case, s, hd)[0]
            S = Kq @ s.q[0, hd * G:(hd + 1) * G].astype(np.float64).astype(np.int64).T
            for splits in (2, 3, 16):
                mx = np.array([S[a:b].max(0) for a, b in r.window_splits(s.n, case.window, splits)])
                if ((mx.min(0) < mx.max(0)) & unit[hd * G:(hd + 1) * G]).any():
                    return True
    return False


def _mutations(case):
    """name -> (has the feature (None: read off the walk), mutations of a sequence)"""
    decode = case.kind == 'decode'
    G, W, sinks = case.Hq // case.Hkv, case.window, case.sinks is not None
    if decode:
        inside = any(s.n > W for s in case.seqs)               # a window that starts inside the context
        multi = any(len(r.window_splits(s.n, W, 2)) > 1 for s in case.seqs)
    else:
        inside = any(s.n > W for s in case.seqs)
        wave = any(s.hist + i >= W for s in case.seqs for i in range(len(s.q)) if i % 16)
    m = {
        'window edge - 1: let in the token in front of the window': (inside, lambda s: [('win_shift', -1)]),
        'window edge + 1: drop the first token of the window': (inside and W > 1, lambda s: [('win_shift', +1)]),
        'sink omitted': (sinks, lambda s: [('no_sink', None)]),
        'sink of head h + 1 used for head h': (sinks, lambda s: [('next_sink', None)]),
        'drop the newest visible token (decode: ctx - 1; prefill: diagonal - 1)': (True, lambda s: [('ctx_shift', -1)]),
        'let in the token behind the context (decode: ctx; prefill: diagonal + 1)': (True, lambda s: [('ctx_shift', +1)]),
        'use token t + 1\'s V (scale, zero) for token t': (decode and case.bits != 16, lambda s: [('next_v_param', None)]),
        # at W = 1 every head sees the newest token alone, and that one is live for all of them
        'give head h the live set of head h + 1': (G > 1 and W > 1, lambda s: [('next_head', None)]),
        'skip the rescale once where the max moved': (None, lambda s: [('skip_rescale', -1 if decode else +1)]),
        'treat a dead token as weight 2^-20': (W > 1, lambda s: [('dead_weight', 20)]),
    }
    if decode:
        m['sink counted once per non-empty split'] = (sinks and multi, lambda s: [('sink_per_split', k) for k in (2, 3, 16)])
        m['sink weighted against a split\'s own maximum'] = (sinks and _split_max_differs(case),
                                                              lambda s: [('sink_split_max', k) for k in (2, 3, 16)])
        m['drop the first tile of a split'] = (True, _tile_muts(case, 'first', 0.0))
        m['drop the last tile of a split'] = (True, _tile_muts(case, 'last', 0.0))
        m['count the first tile of a split twice'] = (W > 1, _tile_muts(case, 'first', 2.0))
        m['count the last tile of a split twice'] = (W > 1, _tile_muts(case, 'last', 2.0))
    else:
        m['every row masked with the window edge of its wave\'s first row'] = (wave, lambda s: [('wave_edge', None)])
        m['drop a 64-key stage'] = (True, lambda s: [('tile_factor', (a, a + 64, 0.0)) for a in range(0, s.n, 64)])
        m['count a 64-key stage twice'] = (W > 1, lambda s: [('tile_factor', (a, a + 64, 2.0)) for a in range(0, s.n, 64)])
    return m


def _sensitivity(cases):
    totals, n_cases = {}, {}
    for case in cases:
        for name, (has, muts) in _mutations(case).items():
            if has is False:
                continue
            n, skipped = _changed(case, muts)
            if has is None:
                has = skipped
            if has:
                what = f'{case.kind} bits {case.bits} head_dim {case.D} Hq {case.Hq} tier {case.tier} window {case.window}'
                assert n > 0, f'"{name}" changes nothing in {what}'
                totals[name] = totals.get(name, 0) + n
                n_cases[name] = n_cases.get(name, 0) + 1
    for name, n in totals.items():
        print(f'[attention window exact sensitivity] {name}: {n} (sequence, head) pairs change in {n_cases[name]} cases')
    return n_cases


@pytest.mark.parametrize('D,bits', DB)
def test_decode_reference_is_sensitive(D, bits):
    cases = _decode_of(D, bits)
    n_cases = _sensitivity(cases)
    sink_cases = sum(c.sinks is not None for c in cases)
    assert n_cases['sink omitted'] == sink_cases == 6 and n_cases['window edge - 1: let in the token in front of the window'] == 10
    # every sink case with more than one tile in some window has a split below the merged maximum, but for tier A at windows of one
    # or two tiles, where both tiles hold a live token of every head (the window's first and the newest)
    assert n_cases['sink weighted against a split\'s own maximum'] >= sum(c.sinks is not None and (c.tier == 'B' and c.window > 1 or c.window >= 64)
                                                                          for c in cases)
    assert n_cases['skip the rescale once where the max moved'] >= sum(c.tier == 'B' and c.window >= 32 for c in cases)


@pytest.mark.parametrize('D', [128, 64])
def test_prefill_reference_is_sensitive(D):
    cases = _prefill_of(D)
    n_cases = _sensitivity(cases)
    assert n_cases['sink omitted'] == sum(c.sinks is not None for c in cases) >= 9
    assert n_cases['every row masked with the window edge of its wave\'s first row'] == 8 * 3         # all but W = 4096
    assert n_cases['skip the rescale once where the max moved'] >= sum(c.tier == 'B' and c.window >= 65 for c in cases)
