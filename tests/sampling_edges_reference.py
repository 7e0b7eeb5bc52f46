"""Inputs for the sampler, logprobs and logits-processor kernels (csrc/sampling.hip) at their structural edges.  Plain numpy, no GPU.

Expected values are never computed here: they come from oracle.tm_oracle (sample_filter, sample_draw, sample_logprobs,
logits_process).  This module builds the rows, models the kernels' bin ownership, and proves that a comparison with the oracle is
decided by the kernel's structure and not by rounding.

The margin rule.  sample_select_kernel sums count x weight per fp16 bin, the oracle cumsums the sorted candidates; both work in
fp64 on the same fp32 exponents, so a running sum differs by accumulation order only: at most V * 2^-53 relative to 1.
margins() restates the pipeline in np.longdouble and returns three distances: top_p from the nearest cumulative probability,
min_p from the nearest p_i / p_max among the candidates left, u from the nearest renormalised cumulative probability of the
survivors.  Every committed case keeps each of them >= floor_of(V) = 64 * V * 2^-53, without exception.  The min_p distance and
the u distance of the unfiltered all-defaults rows are held to 2^-20 as well (RELAXED: a fixed figure that does not shrink with V;
for every V used here it is the larger of the two, and these cases meet both).  The one place where 2^-20 cannot apply is
u = 1 - 2^-24 on a row that ends in zero-probability candidates: the cumulative sum before them is 1, 2^-24 away by construction;
such a row is held to floor_of(V).  The sum of ALL survivors is left out of the u distance: a draw that no prefix sum exceeds falls
back to the last survivor, the same token.  Two remarks on the min_p distance: candidates that share the
maximum's logit have ratio exactly 1 in both implementations (weight exp(0) = 1, p >= p * min_p holds for every min_p <= 1 in
floating point), so they are left out of it -- that is what makes min_p = 1.0 a legitimate case; and both sides of the comparison
carry the same normaliser, so no accumulated sum enters it at all.
A nominal parameter that misses its floor is replaced by the first float32 at or above it, within 16 ulps, that meets it
(settle(); Call.nudges counts them).  Nothing is dropped.

The bin model.  key_of / desc_bin / owner restate key_of() of the kernel: a positive pattern h sits in descending bin 0x7fff - h,
a negative 0x8000 | m in bin 0x8000 + m, -0.0 in the bin of +0.0 (bin 32768 stays empty), NaN in bin 65535.  Thread t of the
1024-thread walk owns bins 64 t .. 64 t + 63, wave w bins 4096 w .. 4096 w + 4095.

Order among zero-probability candidates.  The kernel orders NaN below -inf, the oracle ties them (NaN -> -inf, then by id).  The
order among zero-probability candidates of different kinds is not part of the contract: every row here whose candidate order is
compared holds -inf or NaN, never both.
"""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

from oracle import tm_oracle as o

f16, f32 = np.float16, np.float32
LD = np.longdouble
KBINS = 65536
U_LAST = f32(1.0 - 2.0**-24)                 # the largest uniform number the Philox stream can return
RELAXED = 2.0**-20
NUDGE_ULPS = 16
INF = float('inf')


# ------------------------------------------------------------------------------------------------
# bin model
# ------------------------------------------------------------------------------------------------
def key_of(bits):
    """fp16 bit pattern(s) -> the kernel's order-preserving 16-bit key (NaN lowest, -0.0 with +0.0)"""
    b = np.asarray(bits, np.int64) & 0xffff
    nan = ((b & 0x7c00) == 0x7c00) & ((b & 0x03ff) != 0)
    key = np.where(b & 0x8000, 0xffff - b, b | 0x8000)
    key = np.where(b == 0x8000, 0x8000, key)
    return np.where(nan, 0, key)


def desc_bin(bits):
    """index in the DESCENDING walk: bin j <-> key 65535 - j"""
    return KBINS - 1 - key_of(bits)


def owner(bits):
    """(thread, q, wave) of the 1024-thread walk that owns the bin of `bits`"""
    j = desc_bin(bits)
    return j // 64, j % 64, j // 4096


def bits_of_bin(j):
    """inverse of desc_bin (value_of_key of the kernel): the fp16 pattern whose value the bin stands for"""
    key = KBINS - 1 - np.asarray(j, np.int64)
    return np.where(key & 0x8000, key & 0x7fff, 0xffff - key).astype(np.uint16)


def value_of_bits(bits):
    return np.asarray(bits, np.uint16).view(f16)


# ------------------------------------------------------------------------------------------------
# margins
# ------------------------------------------------------------------------------------------------
def floor_of(V):
    return 64.0 * V * 2.0**-53


def _profile(row, T, top_k):
    """the candidates of one row in sampling order and their probabilities in longdouble (fp32 exponents, as kernel and oracle)"""
    v = np.asarray(row, f16).astype(f32)
    ids = np.arange(v.size)
    key = np.where(np.isnan(v), -np.inf, v)
    order = np.lexsort((ids, -key))
    k = v.size if top_k <= 0 else min(int(top_k), v.size)
    cand = order[:k]
    inv_t = f32(1.0) / f32(T if T > 0 else 1.0)
    with np.errstate(invalid='ignore'):
        z = ((v[cand] - v[cand[0]]).astype(f32) * inv_t).astype(f32)
    w = np.exp(z.astype(LD))
    w = np.where(np.isnan(w), LD(0), w)
    p = w / w.sum()
    return cand, z, p, np.cumsum(p)


def _distances(prof, top_p, min_p, u):
    cand, z, p, cum = prof
    top_p, min_p, u = LD(f32(top_p)), LD(f32(min_p)), LD(f32(u))
    d_p = d_m = INF
    kept, ksum = len(p), LD(1)
    if top_p < 1:
        d_p = float(np.abs(cum - top_p).min())
        hit = np.flatnonzero(cum > top_p)
        if hit.size:
            kept, ksum = int(hit[0]) + 1, cum[hit[0]]
    if min_p > 0:
        r = (p[:kept] / p[0])[z[:kept] != 0]          # ties of the maximum: ratio exactly 1 on both sides, see the docstring
        if r.size:
            d_m = float(np.abs(r - min_p).min())
        kept = int((p[:kept] >= p[0] * min_p).sum())
        ksum = p[:kept].sum()
    rc = (np.cumsum(p[:kept]) / ksum)[:-1]             # the draw falls back to the last survivor: its own sum decides nothing
    d_u = float(np.abs(rc - u).min()) if rc.size else INF
    return d_p, d_m, d_u


def margins(row, T, top_k, top_p, min_p, u):
    """(distance of top_p, of min_p, of u) from the nearest value at which the result would change; inf = filter off"""
    return _distances(_profile(row, T, top_k), top_p, min_p, u)


@dataclass
class Call:
    """one tm_sample call: logits [B, ld] (columns [V, ld) are padding) and the per-row parameters, all as the C-ABI takes them"""
    name: str
    V: int
    ld: int
    logits: np.ndarray
    temperature: np.ndarray
    top_k: np.ndarray
    top_p: np.ndarray
    min_p: np.ndarray
    u: np.ndarray
    tags: list
    claims: list = field(default_factory=list)
    margins: np.ndarray = None
    nudges: int = 0
    _expected: list = None

    @property
    def B(self):
        return len(self.tags)

    def all_defaults(self, b):
        return self.top_k[b] <= 0 and self.top_p[b] >= 1 and self.min_p[b] <= 0

    def floors(self, b):
        """what row b's three margins must reach"""
        base = floor_of(self.V)
        relaxed_u = self.all_defaults(b) and self.u[b] != U_LAST
        return base, max(base, RELAXED), max(base, RELAXED) if relaxed_u else base

    def expected(self):
        """[(candidate ids in sampling order, renormalised probabilities, drawn token)] from the oracle, computed once"""
        if self._expected is None:
            self._expected = []
            for b in range(self.B):
                ids, p = o.sample_filter(self.logits[b, :self.V], float(self.temperature[b]), int(self.top_k[b]),
                                         float(self.top_p[b]), float(self.min_p[b]))
                self._expected.append((ids, p, o.sample_draw(ids, p, float(self.u[b]))))
        return self._expected


def _make(name, V, ld, logits, rows, claims=None):
    arr = lambda k, d, t: np.asarray([r.get(k, d) for r in rows], t)
    call = Call(name, V, ld, np.ascontiguousarray(logits, f16), arr('temperature', 1.0, f32), arr('top_k', 0, np.int32),
                arr('top_p', 1.0, f32), arr('min_p', 0.0, f32), arr('u', 0.0, f32),
                [', '.join(f'{k}={v}' for k, v in r.items() if k != 'claim') or 'default' for r in rows],
                claims if claims is not None else [r.get('claim') for r in rows])
    return settle(call)


def settle(call):
    """Apply the margin rule: a parameter that misses its floor moves up by float32 steps, 16 at the most.  A row that cannot be
    settled keeps its nominal value and its short margin, for tests/test_host_sampling_edges.py to report."""
    call.margins = np.zeros((call.B, 3))
    for b in range(call.B):
        prof = _profile(call.logits[b, :call.V], call.temperature[b], call.top_k[b])
        par = [call.top_p[b], call.min_p[b], call.u[b]]
        need = call.floors(b)
        for i in range(3):
            for step in range(NUDGE_ULPS + 1):
                if _distances(prof, *par)[i] >= need[i]:
                    call.nudges += step > 0
                    break
                par[i] = np.nextafter(f32(par[i]), f32(2.0))
            else:
                par[i] = [call.top_p[b], call.min_p[b], call.u[b]][i]
        call.top_p[b], call.min_p[b], call.u[b] = par
        call.margins[b] = _distances(prof, *par)
    return call


def margin_report(calls):
    """(number of rows, smallest margin / its floor over all rows and filters, that margin, that floor)"""
    worst = (INF, INF, INF)
    rows = 0
    for c in calls:
        for b in range(c.B):
            rows += 1
            for m, need in zip(c.margins[b], c.floors(b)):
                if m / need < worst[0]:
                    worst = (m / need, m, need)
    return (rows,) + worst


# ------------------------------------------------------------------------------------------------
# section 2: boundary rows -- four adjacent fp16 values, sixteen tokens each, V = 64
# ------------------------------------------------------------------------------------------------
BOUNDARY_SETS = {
    'thread': (0x3c01, 0x3c00, 0x3bff, 0x3bfe),        # 1.0 = q 63 of thread 271 | 0x3bff = q 0 of thread 272
    'wave': (0x4001, 0x4000, 0x3fff, 0x3ffe),          # 2.0 = last bin of wave 3 | 0x3fff = first bin of wave 4
    'sign': (0x0002, 0x0001, (0x0000, 0x8000), 0x8001),  # bin 32767 | the empty bin 32768 | bin 32769; wave 7 -> 8; subnormals
    'top': (0x7bff, 0x7bfe, 0x7bfd, 0x7bfc),           # 65504 = q 0 of thread 16, the first bin a finite logit can occupy
    'bottom': (0xfbfd, 0xfbfe, 0xfbff, 0xfc00),        # -65504 = q 63 of thread 1007 | -inf = q 0 of thread 1008 (zero weight)
}
# the bins the table above claims: (group, bin, thread, q, wave)
BOUNDARY_OWNERS = {
    'thread': ((1, 17407, 271, 63, 4), (2, 17408, 272, 0, 4)),
    'wave': ((1, 16383, 255, 63, 3), (2, 16384, 256, 0, 4)),
    'sign': ((0, 32765, 511, 61, 7), (1, 32766, 511, 62, 7), (2, 32767, 511, 63, 7), (3, 32769, 512, 1, 8)),
    'top': ((0, 1024, 16, 0, 0),),
    'bottom': ((2, 64511, 1007, 63, 15), (3, 64512, 1008, 0, 15)),
}
BOUNDARY_TOP_KS = (1, 15, 16, 17, 32, 33, 48, 63, 64, 70)
GROUP = 16


def boundary_row(name):
    """(fp16 row [64], group of every token).  Ids are scrambled so that the tie order by id is visible."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    grp = rng.permutation(np.repeat(np.arange(4), GROUP))
    bits = np.zeros(64, np.uint16)
    for g, s in enumerate(BOUNDARY_SETS[name]):
        at = np.flatnonzero(grp == g)
        bits[at] = s if isinstance(s, int) else np.where(rng.permutation(GROUP) % 2 == 0, s[0], s[1])
    return bits.view(f16), grp


def boundary_values(name):
    return np.asarray([value_of_bits(s if isinstance(s, int) else s[0]).astype(np.float64) for s in BOUNDARY_SETS[name]])


def boundary_temperature(name):
    """the smallest power of two at which every pair of adjacent finite groups differs by a factor >= 0.9"""
    v = boundary_values(name)
    d = -np.diff(v[np.isfinite(v)])
    return float(2.0 ** np.ceil(np.log2(d.max() / -np.log(0.9))))


def _group_weights(name, T):
    v = boundary_values(name).astype(f32)
    z = ((v - v[0]).astype(f32) * (f32(1.0) / f32(T))).astype(f32)
    return np.exp(z.astype(LD))


@functools.lru_cache(maxsize=None)
def boundary_call(name):
    """The sweep of section 2 as the rows of one call.  claim = (which filter cuts, group of the cut, expected kept)."""
    row, grp = boundary_row(name)
    T = boundary_temperature(name)
    w = _group_weights(name, T)
    p = w / (GROUP * w.sum())                          # one member of each group
    before = np.concatenate([[LD(0)], np.cumsum(GROUP * p)])[:4]
    r = w / w[0]
    rows = []
    for k in BOUNDARY_TOP_KS:
        kept = min(k, 64)
        rows.append(dict(top_k=k, u=U_LAST, claim=('top_k', (kept - 1) // GROUP, kept)))
    for g in range(4):                                 # the middle of the 8th member of group g
        tp = f32(before[g] + 7.5 * p[g])
        rows.append(dict(top_p=tp, u=U_LAST, claim=('top_p', g, 16 * g + 8) if tp < 1 else ('off', 3, 64)))
    for g in range(3):                                 # between group g and g + 1; below a zero-weight group: half the ratio
        mp = f32(np.sqrt(r[g] * r[g + 1]) if r[g + 1] > 0 else r[g] / 2)
        rows.append(dict(min_p=mp, u=U_LAST, claim=('min_p', g, 16 * (g + 1))))
    rows.append(dict(min_p=1.0, u=U_LAST, claim=('min_p', 0, 16)))
    us = [(f32(0.0), 0, 0)]
    live = [g for g in range(4) if p[g] > 0]           # a zero-weight group (-inf) is never drawn: its positions collapse into 1 - 2^-24
    for g in live:
        for m in (0, GROUP - 1):                       # the middle of the first and of the last member of group g
            us.append((f32(before[g] + (m + 0.5) * p[g]), g, m))
    us.append((U_LAST, live[-1], GROUP - 1))
    seen = set()
    for u, g, m in us:
        if float(u) not in seen:
            seen.add(float(u))
            rows.append(dict(u=u, claim=('u', g, m)))
    # top_k = 40 (8 members of group 2), a top_p at the middle of the 4th of them, a min_p that removes group 2 again
    z40 = GROUP * (w[0] + w[1]) + 8 * w[2]
    rows.append(dict(top_k=40, top_p=f32((GROUP * (w[0] + w[1]) + 3.5 * w[2]) / z40), min_p=f32(np.sqrt(r[1] * r[2])), u=U_LAST,
                     claim=('combined', 1, 32)))
    for rr in rows:
        rr['temperature'] = T
    return _make(f'boundary-{name}', 64, 64, np.tile(row, (len(rows), 1)), rows)


def rival_outcomes(call, b):
    """What three neighbouring rules would return for row b, as {(name): (kept, token)}: ties taken by DESCENDING id, and the
    candidate list cut one candidate earlier / later (for a row without a filter: the draw landing one candidate earlier / later)."""
    V = call.V
    row = call.logits[b, :V]
    par = (float(call.temperature[b]), int(call.top_k[b]), float(call.top_p[b]), float(call.min_p[b]))
    u = float(call.u[b])
    out = {}
    ids, p = o.sample_filter(row[::-1], *par)
    out['ties by descending id'] = (len(ids), V - 1 - o.sample_draw(ids, p, u))
    ids, p, tok = call.expected()[b]
    full, _ = o.sample_filter(row, par[0], 0, 1.0, 0.0)
    pos = int(np.flatnonzero(ids == tok)[0])
    if call.all_defaults(b):
        if pos > 0:
            out['draw one earlier'] = (len(ids), int(ids[pos - 1]))
        if pos + 1 < len(ids):
            out['draw one later'] = (len(ids), int(ids[pos + 1]))
        return out
    w = np.exp(((row[full].astype(f32) - row[full[0]].astype(f32)) * (f32(1) / f32(par[0]))).astype(np.float64))
    for name, n in (('cut one earlier', len(ids) - 1), ('cut one later', len(ids) + 1)):
        if 1 <= n <= V:
            q = w[:n] / w[:n].sum()
            out[name] = (n, o.sample_draw(full[:n], q, u))
    return out


# ------------------------------------------------------------------------------------------------
# section 3: vocabulary sizes
# ------------------------------------------------------------------------------------------------
SMALL_VOCABS = ((1, 8), (5, 8), (7, 8), (8, 8), (9, 16), (1023, 1024), (1024, 1024), (1025, 1032), (2049, 2056))
BIG_VOCABS = ((151936, 152064), (137221, 137224))      # 137221 = 131072 + 3 * 2048 + 5: second trip, partial last vector
SECOND_TRIP = 131072                                   # 64 workgroups x 2048 logits: ids from here on need the second trip
SMALL_CAP = 4


def _random_logits(rng, B, ld):
    x = (rng.standard_normal((B, ld)) * 2.5).astype(f16)
    x[:, ::3] = np.round(x[:, ::3].astype(f32) * 4).astype(f16) / f16(4)       # lots of exact ties
    return x


@functools.lru_cache(maxsize=None)
def small_vocab_call(V, ld):
    """Eight rows; ties (first and last id share a value), one -inf, a flat row, padding at 100.0."""
    rng = np.random.default_rng(V)
    rows = [dict(), dict(top_k=1), dict(top_k=3), dict(top_p=0.5), dict(top_p=0.0), dict(min_p=0.1),
            dict(temperature=0.0, top_p=0.5), dict(temperature=-1.0)]
    x = _random_logits(rng, len(rows), ld)
    if V >= 4:
        x[:, V - 1] = x[:, 0]
    if V >= 3:
        x[:, 1] = f16(-np.inf)
    x[2, :] = f16(1.5)
    x[:, V:] = f16(100.0)
    u = rng.random(len(rows)).astype(f32)
    u[0], u[7] = 0.0, U_LAST
    for r, v in zip(rows, u):
        r['u'] = v
    return _make(f'small-{V}', V, ld, x, rows)


BIG_FLAT_ROW, BIG_HIGH_ROW, BIG_TAIL_ROW = 12, 14, 9


@functools.lru_cache(maxsize=None)
def big_vocab_call(V, ld):
    """The twelve rows of test_sampling_matches_oracle (seed V) and three more: a flat row at -3.25 with top_p = 0.3 (one bin of V
    members), temperature 0 with top_p = 0.5, and a row whose maximum and ten next-best logits sit at ids >= 131072."""
    rng = np.random.default_rng(V)
    rows = [dict(), dict(top_k=1), dict(top_k=40), dict(top_k=40, top_p=0.8), dict(top_p=0.9), dict(top_p=0.3, temperature=0.7),
            dict(min_p=0.05), dict(top_k=200, top_p=0.95, min_p=0.02, temperature=1.3), dict(top_p=0.0), dict(top_k=V + 5),
            dict(temperature=0.01), dict(top_p=0.999, temperature=2.0),
            dict(top_p=0.3), dict(temperature=0.0, top_p=0.5), dict()]
    B = len(rows)
    x = _random_logits(rng, B, ld)
    x[:, 5:50:7] = f16(-np.inf)
    x[2, :] = f16(1.5)
    x[BIG_FLAT_ROW, :] = f16(-3.25)
    high = np.concatenate([[SECOND_TRIP, V - 1], SECOND_TRIP + 1 + rng.choice(V - SECOND_TRIP - 2, 9, replace=False)])
    x[BIG_HIGH_ROW, high] = (16.0 - 0.25 * np.arange(11)).astype(f16)          # the maximum at 131072, the runner-up at V - 1
    x[:, V:] = f16(100.0)
    u = rng.random(B).astype(f32)
    u[0], u[4] = 0.0, U_LAST
    u[BIG_TAIL_ROW] = 0.97                             # a draw far behind the first 1024 candidates
    u[BIG_HIGH_ROW] = 0.5
    for r, v in zip(rows, u):
        r['u'] = v
    return _make(f'big-{V}', V, ld, x, rows)


# ------------------------------------------------------------------------------------------------
# section 4: logprobs boundaries, V = 1100 (the smallest multiple-of-4 row that holds 1025 candidates comfortably)
# ------------------------------------------------------------------------------------------------
LP_V, LP_LD = 1100, 1104
LP_CAPS = (1, 5, 64, 1024)
LP_LEVELS = (0x4000, 0x3fff, 0x3c00)                   # 2.0 | the next value down, first bin of wave 4 | 1.0


def _level_row(rng, sizes):
    """a row of len(sizes) + 1 levels: sizes[i] tokens at LP_LEVELS[i], the rest at the next level, ids scrambled"""
    lvl = np.full(LP_V, len(sizes))
    at = 0
    for i, n in enumerate(sizes):
        lvl[at:at + n] = i
        at += n
    bits = np.asarray(LP_LEVELS, np.uint16)[rng.permutation(lvl)]
    row = np.full(LP_LD, 100.0, f16)
    row[:LP_V] = bits.view(f16)
    return row


def _u_at(row, pos):
    """the middle of candidate `pos` of the unfiltered row's cumulative distribution"""
    _, _, p, cum = _profile(row[:LP_V], 1.0, 0)
    return f32(cum[pos] - p[pos] / 2)


@functools.lru_cache(maxsize=None)
def logprobs_call(C):
    """claim = (kept, nA, position of the drawn token or None): kept candidates, candidates in strictly better bins than the cut bin
    of the first min(kept, C), and where the draw is placed."""
    rng = np.random.default_rng(4000 + C)
    n0 = max(1, C // 4)
    rows, logits = [], []

    def add(sizes, claim, **par):
        logits.append(_level_row(rng, sizes))
        rows.append(dict(par, claim=claim))
        return logits[-1]

    three = (n0, max(1, C // 2))                       # cuts by top_k inside the second / third level
    for k in (C - 1, C, C + 1):
        if k >= 1:
            L = min(k, C)
            nA = 0 if L <= n0 else (n0 if L <= sum(three) else sum(three))
            add(three, (k, nA, None), top_k=k, u=0.4)
    add((C,), (LP_V, 0, None), u=0.3141)                 # the best group is exactly the list: nA = 0, the cut bin ends at the cap
    add((C + 7,), (LP_V, 0, None), u=0.6)              # the list is the lowest ids of a larger tie
    if C > 1:
        add((C - 1,), (LP_V, C - 1, None), u=0.7)      # one member from the cut bin
        add((n0, C - n0), (LP_V, n0, None), u=0.2)     # two groups end exactly at the cap
    if C == 1024:                                      # the forced-last rule: the draw at position 1023, then at 1024
        for pos in (1023, 1024):
            row = add((C - 1,), (LP_V, C - 1, pos))
            rows[-1]['u'] = _u_at(row, pos)
    if C == 5:                                         # a draw behind the cap of a short list: nothing is forced
        row = add((4,), (LP_V, 4, 700))
        rows[-1]['u'] = _u_at(row, 700)
    return _make(f'logprobs-{C}', LP_V, LP_LD, np.stack(logits), rows)


# ------------------------------------------------------------------------------------------------
# section 5: degenerate rows between ordinary ones
# ------------------------------------------------------------------------------------------------
DEGENERATE_V = 1000
DEGENERATE_CAP = 8
# batch row -> what it is; the five degenerate rows are those of test_sampling_degenerate_rows_get_a_defined_token
DEGENERATE_LAYOUT = ('ordinary', 'all nan', '+inf maximum', 'ordinary', 'all -inf', 'nan sprinkled', 'ordinary', 'one finite')
DEGENERATE_TOKENS = {1: 0, 2: 300, 4: 0, 7: 777}


@functools.lru_cache(maxsize=None)
def degenerate_call():
    """Returns (call as the GPU sees it, call with NaN -> -inf that the oracle and the margins see).  min_p is not passed (NULL)."""
    rng = np.random.default_rng(3)
    V = DEGENERATE_V
    x = (rng.standard_normal((8, V)) * 2).astype(f16)
    x[0, 5:50:7] = f16(-np.inf)                        # ordinary rows hold -inf, never NaN
    x[1, :] = f16(np.nan)
    x[2, 17] = f16(np.inf)
    x[2, 400] = x[2, 300] = f16(9.0)
    x[4, :] = f16(-np.inf)
    x[5, ::2] = f16(np.nan)
    x[7, :] = f16(np.nan)
    x[7, 777] = f16(-3.0)
    rows = [dict(top_k=50, top_p=0.9, u=0.77), dict(u=0.3), dict(top_p=0.9, u=0.6), dict(u=0.55, temperature=0.8),
            dict(top_k=5, u=0.1), dict(top_p=0.8, u=0.42), dict(top_k=3, u=U_LAST), dict(u=0.9)]
    clean = np.where(np.isnan(x), f16(-np.inf), x)
    proper = [b for b, kind in enumerate(DEGENERATE_LAYOUT) if kind in ('ordinary', 'nan sprinkled', 'one finite')]
    ref = _make('degenerate', V, V, clean[proper], [rows[b] for b in proper])
    gpu = Call('degenerate-gpu', V, V, x, *(np.asarray([r.get(k, d) for r in rows], t) for k, d, t in
               (('temperature', 1.0, f32), ('top_k', 0, np.int32), ('top_p', 1.0, f32), ('min_p', 0.0, f32), ('u', 0.0, f32))),
               list(DEGENERATE_LAYOUT))
    for i, b in enumerate(proper):                     # what the margin rule moved, if anything
        gpu.top_p[b], gpu.u[b] = ref.top_p[i], ref.u[i]
    return gpu, ref, proper


# ------------------------------------------------------------------------------------------------
# section 6: the calls that share one workspace
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reuse_calls():
    """(batch 13 of the big vocabulary, batch 3 at V = 1000, batch 13 at V = 9 with logprobs, the batch-3 call again)"""
    big = big_vocab_call(*BIG_VOCABS[0])
    take = lambda c, rows, name: settle(Call(name, c.V, c.ld, c.logits[rows], c.temperature[rows], c.top_k[rows], c.top_p[rows],
                                             c.min_p[rows], c.u[rows], [c.tags[b] for b in rows]))
    big13 = take(big, [0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14], 'reuse-big')
    rng = np.random.default_rng(1000)
    rows = [dict(u=0.35), dict(top_k=40, top_p=0.8, u=0.9), dict(min_p=0.05, temperature=0.7, u=0.15)]
    x = _random_logits(rng, 3, 1000)
    x[:, 5:50:7] = f16(-np.inf)
    mid = _make('reuse-1000', 1000, 1000, x, rows)
    nine = small_vocab_call(9, 16)
    idx = [0, 1, 2, 3, 4, 5, 6, 7, 0, 3, 5, 6, 7]
    tiny = take(nine, idx, 'reuse-9')
    return big13, mid, tiny, mid


# ------------------------------------------------------------------------------------------------
# section 7 and 3 C: seen masks and logits processors
# ------------------------------------------------------------------------------------------------
SHARD_CASES = ((151936, 151936, 0, 151936), (18992, 18992, 18992, 151936), (18992, 18992, 7 * 18992, 151936),
               (11568, 11568, 3 * 11568, 92544))      # (V, ld, vocab_offset, global vocabulary); TP-8 offsets = 16 (mod 32)
KMAX_BAD, KMAX_END = 32, 9


def mask_of(rows_of_ids, words, vocab):
    """the seen mask a Python loop builds: ids outside [0, vocab) are ignored"""
    want = np.zeros((len(rows_of_ids), words), np.uint32)
    for b, ids in enumerate(rows_of_ids):
        for t in ids:
            t = int(t)
            if 0 <= t < vocab:
                want[b, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return want


def packed_seen_case(vocab=1003):
    """cu_q with the first, a middle and the last sequence empty; ids outside the vocabulary, duplicates, both sides of a word
    boundary and the last id of a vocabulary that is no multiple of 32.  Returns (cu_q, ids, ids per sequence, vocab, words)."""
    assert vocab % 32
    cu_q = np.asarray([0, 0, 5, 5, 9, 9], np.int32)
    ids = np.asarray([31, -1, 32, vocab, 31, vocab - 1, vocab + 40, 7, 7], np.int32)
    per_seq = [ids[cu_q[r]:cu_q[r + 1]] for r in range(5)]
    return cu_q, ids, per_seq, vocab, (vocab + 31) // 32


def process_shard_rows(off, V):
    """the rows of test_logits_process_matches_oracle"""
    return [dict(p=1.3), dict(p=0.6, bad=[5, 17, 0]), dict(), dict(p=2.5, end=[off + 7, off + V - 1], k=10, ml=14),
            dict(bad=[off + 3], end=[off + 11, 0, off + 12], k=13, ml=14), dict(p=1.0001, bad=list(range(off + 100, off + 132)))]


def process_shard_case(V, ld, off, vocab):
    """(logits [6, ld], rows) as in test_logits_process_matches_oracle, the seen ids drawn from the GLOBAL vocabulary"""
    rng = np.random.default_rng(V + off)
    rows = process_shard_rows(off, V)
    for r in rows:
        r['seen'] = rng.integers(0, vocab, int(rng.integers(1, 300))).tolist() + [off, off + V - 1, off + V, max(off - 1, 0)]
    x = (rng.standard_normal((len(rows), ld)) * 4).astype(f16)
    x[:, 1::97] = f16(-60000.0)                        # penalised to -inf in fp16
    return x, rows


PENALTY_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00)   # +-0, +-2^-24, +-65504, +-inf, NaN
PENALTIES = (0.5, 2.0, 1.0, 0.0, -1.0)


def process_edge_cases():
    """[(name, V, ld, off, global vocab, logits, rows)], rows = dict(p, bad, seen) as process_shard_rows, seen = ids of the row"""
    rng = np.random.default_rng(7)
    cases = []
    V, ld = 4099, 4104
    x = (rng.standard_normal((3, ld)) * 4).astype(f16)
    edge = [2047, 2048, 4096, 4098, 2047]              # the workgroup edge, the scalar tail, a duplicate
    cases.append(('edges', V, ld, 0, V, x, [dict(bad=edge, seen=[]), dict(bad=edge, p=2.0, seen=[2047, 4098, 2046, 2049, 4097, 8]),
                                            dict(p=2.0, seen=[2047, 2048, 4096, 4098, 4095])]))
    V = 4096
    x = (rng.standard_normal((4, V)) * 4).astype(f16)
    near = [15, 16, 17, 16 + 4095, 16 + 4096, 47, 48]
    cases.append(('shard+16', V, V, 16, 8192, x, [dict(bad=[15, 16 + 4096], seen=[]), dict(bad=[16, 16 + 4095], seen=[]),
                                                  dict(bad=[15, 16 + 4096], p=2.0, seen=near), dict(p=0.5, seen=near)]))
    V = 24
    n = len(PENALTY_BITS)
    x = (rng.standard_normal((len(PENALTIES), V)) * 4).astype(f16)
    x[:, :n] = np.asarray(PENALTY_BITS, np.uint16).view(f16)                   # seen
    x[:, n:2 * n] = np.asarray(PENALTY_BITS, np.uint16).view(f16)              # not seen
    cases.append(('penalty values', V, V, 0, V, x, [dict(p=p, seen=list(range(n)) + [2 * n + 1]) for p in PENALTIES]))
    return cases


def process_expected(logits, V, off, rows):
    return [o.logits_process(logits[b, :V], r.get('seen', []), float(f32(r.get('p', 1.0))), r.get('bad', []), r.get('end', []),
                             int(r.get('k', 5)), int(r.get('ml', 0)), vocab_offset=off) for b, r in enumerate(rows)]


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, f16), np.ascontiguousarray(b, f16)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint16)[~nan], b.view(np.uint16)[~nan])
