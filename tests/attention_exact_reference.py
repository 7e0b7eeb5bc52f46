"""Attention operands for which every correct order of computation returns the same bits.  Plain numpy, no GPU.

Two facts carry the construction.

1. The softmax weights are powers of two.  A q head has exactly two non-zero channels, a GATE channel (value QG) and a WEIGHT
   channel (value q_w); every other channel of q is 0, so whatever the other channels of K hold multiplies into exact zeros (they
   hold random lattice values: a swizzle or addressing slip that pulls one into a hot channel moves a score by a multiple of 32).
   K sits on the KV quantiser's lattice lo + step * code with the row minimum and maximum pinned, so that o.kv_quant_params finds
   (scale, zero) = (step, lo) and both dequantisation forms return the fp16 input (asserted).  K[t, gate] is `hi` for a LIVE token
   and `lo` for a DEAD one; the gap (hi - lo) * QG puts a dead token's exponent 150 or more below the maximum: exp2 gives 0.
     tier A (membership): softmax_scale = 0 (the kernels' 1 / sqrt(head_dim)), q_w = QG, every live token of a head has
       K[t, weight] = step, the live score is QG * (hi + step) = QG * |lo|, a POWER OF TWO.  Live weights are exp2(0) = 1.  The power
       of two matters: the MFMA kernels evaluate fmaf(s, c, -(m * c)), and s = m gives exactly 0 only if m * c is not rounded.
     tier B (dyadic weights): softmax_scale = float32(ln 2 / 32), whose product with 1.4426950408889634f is exactly 2^-5 in float32
       (asserted in tests/test_host_attention_exact.py), q_w = 32 / step: scores are multiples of 32, one lattice step of
       K[t, weight] is one power of two of weight, live tokens hold K[t, weight] = -j * step, j = 0 .. 8.
2. The weighted sums are exact.  V rows sit on one of three lattices (three (scale, zero) pairs, neighbouring tokens never share
   one), weights are 2^-j: with lsb = 2^-8 * (smallest V step) the builder asserts sum |p| (|v| + |zero|) / lsb <= 2^23 and
   sum p / 2^-8 < 2^24, so every partial sum in every order is an fp32 number.  What is left is ONE division: the expected value is
   the rational sum 2^-j v / sum 2^-j, taken in integers and rounded to fp16 once.  In decode V is adjusted until every output lies
   further than 2^-20 * sum |p v| / sum p from an fp16 rounding boundary (more than the fp64 reference with its float32 scale can
   move it, and more than the 2^-22 |x| that two fp32 roundings of o * (1 / l) need) and is no fp16 subnormal.  Prefill rows share
   too many tokens for that: there every output is moved 2^-22 |x| away (4 x the 1.5 * 2^-24 |x| of o * (1 / l)), and the fp64
   reference is held to the same bits where the wider margin holds and to 1 ulp elsewhere.  Outputs that could not be moved would be
   compared at 1 ulp; their share is capped at 1 in 1000 per case (none so far).

Liveness is not stored: the reference reads it off q and K by exact integer arithmetic (scores, their maximum, the exponent of every
token), so a builder mistake shows as a failed assertion, not as a wrong expectation.

Every q head of a GQA group has its own (gate, weight) channel pair, the channel permutation is drawn per (sequence, kv head); in
prefill the pair also rotates with the query row.  Decode live sets are placed on purpose (_pattern); the slots of the newest block
behind the context hold rows that LOOK live for every head (a mask that lets one in adds a whole token).  Prefill row i (position
hist + i) has hist + i and hist + i + 1 live in its pair -- a diagonal off by one in either direction adds or removes a token --
and live tokens at the 32-key and 64-key boundaries and in the history.

Window and sinks (build_window; the cases above keep their argument tuples, hence their seeds, operands and bits).  A token is
visible from max(ctx - W, 0) on.  In decode the window's first token and the newest one are live for every head and the token in
front of the window looks live (tier B: with the top weight); prefill row at position p has p - W look-alive and p - W + 1 live in
its pair.  The kernels add exp2(f32(sink) * 1.4426950408889634f - m * scale_log2) to the denominator, m the maximum of the raw
scores: exact, contracted or not, for a sink of +0, -0, -inf or -65504, or where m * scale_log2 is an integer.  With live scores
near 8192 a sink of 0 would be nothing, so q gets a third non-zero channel, the one where every K row holds the pinned minimum `lo`:
every score moves by q_off * lo, relative weights and every assertion stay, and the live maximum sits at exponent 0 (tier A) or
EXP_B - j (tier B).  Heads take the four sink values in turn; the reference adds the sink's weight 2^(8 - e_s) to the denominator
only, and V is settled with it in place.  Assertion 7 for these cases is tests/attention_window_reference.py (float64 over the
cropped context, the sink an extra column)."""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

from oracle import tm_oracle as o

f16, f32, f64 = np.float16, np.float32, np.float64
QG = 256                                     # q[gate]
JMAX = 8                                     # live weights 2^0 .. 2^-8
DEAD_EXP = 150.0                             # a dead token's exponent lies at least this far below the maximum
BUDGET = 2.0**23
SCALE_B = f32(np.log(2.0) / 32)              # float32(ln 2 * 2^-5)
LOG2E = f32(1.4426950408889634)
NAN16 = 0x7e00
KLEN_DECODE = (1, 63, 64, 65, 129, 256, 257, 1089, 4161)
GROUPS_DECODE = (1, 4, 6, 8, 16, 20)
PREFILL_SHAPES = (((1, 64, 65), (0, 64, 31)), ((130,), (62,)), ((200, 37), (0, 300)))
GROUPS_PREFILL = (1, 2, 4, 6, 7)


def softmax_scale(tier, D):
    """what the C-ABI is given: 0 = the kernels' default"""
    return 0.0 if tier == 'A' else float(SCALE_B)


def scale_log2(tier, D):
    """the float32 factor the kernels multiply scores with (c_api.hip)"""
    s = SCALE_B if tier == 'B' else f32(1.0) / np.sqrt(f32(D))
    return f32(s * LOG2E)


class Lattice:
    def __init__(self, bits):
        self.bits = bits
        self.ncode = 15 if bits == 4 else 255                # 16 bits: the 8-bit lattice, stored as it is
        self.step = 2.0 if bits == 4 else 0.25
        self.lo = -16.0 if bits == 4 else -32.0
        self.hi = self.lo + self.step * self.ncode
        self.v = [(self.step, self.lo), (self.step / 2, self.lo / 2), (self.step * 2, self.lo * 2)]   # V (scale, zero) variants
        self.vlsb = self.step / 2

    def q_w(self, tier):
        return QG if tier == 'A' else int(32 / self.step)


@dataclass
class Seq:
    q: np.ndarray            # fp16 [R, Hq, D]   (R = 1 in decode)
    K: np.ndarray            # fp16 [Hkv, nalloc, D]; rows >= n: look-alive rows behind the context (decode), none in prefill
    V: np.ndarray
    vvar: np.ndarray         # int [Hkv, nalloc]: V lattice variant of every row
    n: int                   # context length
    hist: int                # prefill: tokens in front of row 0 (decode: n - 1)
    bits: np.ndarray = None  # expected uint16 [R, Hq, D]
    loose: np.ndarray = None  # bool [R, Hq, D]: closer than 2^-22 |x| to a rounding boundary, compared at 1 ulp


@dataclass
class Case:
    kind: str
    bits: int
    D: int
    Hq: int
    Hkv: int
    tier: str
    seqs: list = field(default_factory=list)
    window: int = 0          # sliding window (0 = none): the query at position p sees the keys t with 0 <= p - t < window
    sinks: np.ndarray = None  # fp16 [Hq] sink logits (None = no sinks)
    q_off: int = 0           # q's value in the channel where every K row holds `lo` (0 = no offset channel, the cases without window)

    @property
    def lat(self):
        return Lattice(self.bits)

    @property
    def klen(self):
        return [s.n for s in self.seqs]


# ---- the exact reference --------------------------------------------------------------------------------------------------------
def _ctx_of(case, s):
    """visible context of every query row [R]"""
    R = s.q.shape[0]
    return np.full(1, s.n) if case.kind == 'decode' else s.hist + 1 + np.arange(R)


def _units(case, s, hd):
    """integer images of one kv head: K in K steps, V in V lsbs, V zero in V lsbs, V codes"""
    lat = case.lat
    Kq = np.rint(s.K[hd].astype(f64) / lat.step).astype(np.int64)
    Vu = np.rint(s.V[hd].astype(f64) / lat.vlsb).astype(np.int64)
    vs = np.array([v[0] for v in lat.v])[s.vvar[hd]]
    vz = np.array([v[1] for v in lat.v])[s.vvar[hd]]
    return Kq, Vu, vs, vz


def _wlo_of(case, ctx):
    """first visible token of every query row [R]: max(ctx - window, 0), which is decode's wbeg and the prefill row's p - W + 1"""
    return np.maximum(ctx - case.window, 0) if case.window else np.zeros_like(ctx)


def window_splits(n, window, splits, tile=32):
    """the token ranges of the non-empty splits of the windowed decode kernel: the tiles from the one the window starts in to the
    newest, ceil(tiles / splits) to a split"""
    wbeg = max(n - window, 0) if window else 0
    tlo, tend = wbeg // tile, (n + tile - 1) // tile
    per = (tend - tlo + splits - 1) // splits
    out = [(max((tlo + i * per) * tile, wbeg), min((tlo + (i + 1) * per) * tile, n)) for i in range(splits)]
    return [(a, b) for a, b in out if b > a]


def _sink_weight(case, smax, sinks, check):
    """integer weight 2^(8 - e_s) of the sink of every query column, e_s = m * scale_log2 - sink * log2(e): what the kernels add to
    the denominator, exp2(f32(sink) * 1.4426950408889634f - m * scale_log2), in the unit of _weights"""
    mc = smax.astype(f64) * (case.lat.step * float(scale_log2(case.tier, case.D)))
    sk = sinks.astype(f64)
    with np.errstate(over='ignore', under='ignore'):
        ws = np.exp2(JMAX + sk * float(LOG2E) - mc)
    if check:                                                  # exact whether or not the expression is contracted into an fma
        assert (np.isin(sk, (0.0, -65504.0)) | np.isneginf(sk)).all(), 'sink logits: +0, -0, -inf, -65504'
        assert (mc == np.rint(mc)).all() and (case.tier == 'B' or not mc.any()), 'the maximum times scale_log2 must be an integer'
        assert (ws[sk != 0] == 0).all() and (np.abs(mc) <= JMAX).all()
    return ws


def _weights(case, S, vis, check):
    """S int64 [n, C] scores in K steps, vis bool [n, C] -> (integer weights 2^(8 - j) [n, C], exponents e [n, C], dead [n, C],
    the visible maximum [C])"""
    lat, c = case.lat, float(scale_log2(case.tier, case.D))
    smax = np.where(vis, S, np.iinfo(np.int64).min // 2).max(0)
    e = (smax[None] - S).astype(f64) * (lat.step * c)
    live = vis & ((e <= JMAX) if case.tier == 'B' else (e == 0))
    dead = vis & ~live
    if check:
        assert vis.any(0).all() and live.any(0).all(), 'a query without a live token'                       # assertion 3
        assert (e[dead] >= DEAD_EXP).all(), 'a dead token within 150 of the maximum'                         # assertion 4
        if case.tier == 'B':
            assert not (S[vis] * lat.step % 32).any(), 'scores must be multiples of 32'                     # assertion 2
            assert (e[live] == np.rint(e[live])).all()
        else:                                                  # m * c must not be rounded: fmaf(m, c, -(m * c)) = 0
            m = (smax * lat.step).astype(f32)
            assert ((m * f32(c)).astype(f64) == m.astype(f64) * c).all(), 'tier A: the live score must be a power of two'
    w = np.where(live, np.exp2(JMAX - np.where(live, e, 0.0)), 0.0)
    return w, e, dead, smax


def _round(N, Dn, A, vlsb):
    """fp16 rounding of vlsb * N / Dn -> (bits, strict, good): strict = further than 2^-22 |x| from a rounding boundary (the
    issue's margin), good = further than 2^-20 * vlsb * A / Dn and not subnormal (the builder's target)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        x = N / Dn[:, None] * vlsb
        a = A / Dn[:, None] * vlsb
    r = x.astype(f16)
    up = np.nextafter(r, f16(np.inf)).astype(f64)
    dn = np.nextafter(r, f16(-np.inf)).astype(f64)
    r64 = r.astype(f64)
    dist = np.minimum(np.abs(x - (r64 + up) / 2), np.abs(x - (r64 + dn) / 2))
    strict = dist > 2.0**-22 * np.abs(x)
    good = (dist > 2.0**-20 * a) & ((x == 0) | (np.abs(x) >= 2.0**-14))
    bits = r.view(np.uint16).copy()
    bits[bits == 0x8000] = 0
    bits[np.isnan(x)] = NAN16
    return bits, strict, good


def ulp16(a, b):
    """distance of two fp16 bit patterns in representable steps (sign-magnitude aware; NaN patterns are far from everything)"""
    a, b = a.astype(np.int32), b.astype(np.int32)
    a = np.where(a & 0x8000, -(a & 0x7fff), a)
    b = np.where(b & 0x8000, -(b & 0x7fff), b)
    return np.abs(a - b)


def reference(case, s, mut=None, check=False, detail=False):
    """expected uint16 [R, Hq, D] of one sequence by integer arithmetic.  `mut` = (name, argument) applies one deliberate error to
    the COMPUTATION (tests/test_host_attention_exact.py: every one of them has to change the result)."""
    lat, G = case.lat, case.Hq // case.Hkv
    R = s.q.shape[0]
    name, arg = mut if mut else (None, None)
    ctx = _ctx_of(case, s)
    wlo = _wlo_of(case, ctx)
    nalloc = s.K.shape[1]
    if name == 'win_shift':                                   # -1: let in the token in front of the window; +1: drop its first token
        sh = wlo + arg
        wlo = np.where((case.window > 0) & (ctx > case.window) & (sh < ctx), sh, wlo)
    if name == 'wave_edge':                                   # prefill: every row masked with the lower edge of its wave's first row
        wlo = wlo[np.arange(R) // 16 * 16]
    sinks = case.sinks
    if sinks is not None and name == 'next_sink':             # head h counts head h + 1's sink
        sinks = np.roll(sinks, -1)
    if name == 'ctx_shift':                                   # -1: drop the newest visible token; +1: let in the one behind it
        sh = ctx + arg
        ok = (sh >= 1) & (sh <= nalloc)
        ctx = np.where(ok, sh, ctx)
    bits = np.zeros((R, case.Hq, case.D), np.uint16)
    strict = np.ones(bits.shape, bool)
    good = np.ones(bits.shape, bool)
    extra = {}
    t = np.arange(nalloc)
    for hd in range(case.Hkv):
        Kq, Vu, vs, vz = _units(case, s, hd)
        qh = s.q[:, hd * G:(hd + 1) * G].astype(f64).astype(np.int64)        # [R, G, D]
        if name == 'next_head':                               # head h computes with head h + 1's q (its live set)
            qh = np.roll(qh, -1, axis=1)
        S = Kq @ qh.reshape(R * G, -1).T                      # [nalloc, R * G]
        vis = (t[:, None] < np.repeat(ctx, G)[None, :]) & (t[:, None] >= np.repeat(wlo, G)[None, :])
        w, e, dead, smax = _weights(case, S, vis, check)
        if name == 'tile_factor':                             # arg = (first token, end token, factor): a tile dropped or counted twice
            w = w * np.where((t >= arg[0]) & (t < arg[1]), arg[2], 1.0)[:, None]
        if name == 'dead_weight':                             # a dead token leaks 2^-20
            w = w + dead * 2.0**(JMAX - arg)
        if name == 'next_v_param':                            # token t's codes with token t + 1's (scale, zero)
            code = (s.V[hd].astype(f64) - vz[:, None]) / vs[:, None]
            vs2, vz2 = np.roll(vs, -1), np.roll(vz, -1)
            Vu = (code * vs2[:, None] + vz2[:, None]) / lat.vlsb
        if name == 'skip_rescale':
            N, Dn, skipped = _walk(case, S, vis, Vu.astype(f64), arg)
            A = np.abs(N)
            extra['skipped'] = extra.get('skipped', False) or bool(skipped.any())     # whether the error had a place to happen
        else:
            N, Dn, A = w.T @ Vu.astype(f64), w.sum(0), w.T @ np.abs(Vu).astype(f64)
        ws = None
        if sinks is not None and name != 'no_sink':           # the sink joins the denominator alone: nothing for N or A
            ws = _sink_weight(case, smax, np.tile(sinks[hd * G:(hd + 1) * G], R), check)
            if name == 'sink_per_split':                      # arg = splits: once per non-empty split instead of once
                ws = ws * len(window_splits(s.n, case.window, arg))
            if name == 'sink_split_max':                      # arg = splits: against the lowest maximum of a split, not the merged one
                low = np.min([S[a:b].max(0) for a, b in window_splits(s.n, case.window, arg)], 0)     # all of [a, b) is visible
                ws = _sink_weight(case, low, np.tile(sinks[hd * G:(hd + 1) * G], R), False)
            Dn = Dn + ws * (2.0**-JMAX if name == 'skip_rescale' else 1.0)      # _walk's unit is the maximum's weight
        if check:                                             # assertion 5: every partial sum in every order is an fp32 number
            lsb = np.where(w > 0, w, np.inf).min(0)           # the smallest weight of every query
            if ws is not None:
                lsb = np.minimum(lsb, np.where(ws > 0, ws, np.inf))
            assert ((w.T @ (np.abs(Vu) + np.abs(vz / lat.vlsb)[:, None])) / lsb[:, None]).max() <= BUDGET and (Dn / lsb).max() < 2.0**24
        b_, s_, g_ = _round(N, Dn, A, lat.vlsb)
        bits[:, hd * G:(hd + 1) * G] = b_.reshape(R, G, -1)
        strict[:, hd * G:(hd + 1) * G] = s_.reshape(R, G, -1)
        good[:, hd * G:(hd + 1) * G] = g_.reshape(R, G, -1)
        extra[hd] = (w, e)
    return (bits, strict, good, extra) if detail else bits


def _walk(case, S, vis, Vu, direction):
    """the online softmax, one 64-token tile at a time (direction -1: newest first, +1: oldest first), in float64 -- exact for
    these operands -- with ONE rescale left out: the first time a maximum moves while something has been accumulated"""
    c = float(scale_log2(case.tier, case.D)) * case.lat.step
    n, C = S.shape
    m = np.full(C, -np.inf)
    N, Dn = np.zeros((C, Vu.shape[1])), np.zeros(C)
    skipped = np.zeros(C, bool)
    starts = list(range(0, n, 64))
    for a in (starts[::-1] if direction < 0 else starts):
        Sv = np.where(vis[a:a + 64], S[a:a + 64].astype(f64), -np.inf)
        mnew = np.maximum(m, Sv.max(0))
        with np.errstate(invalid='ignore', under='ignore'):
            alpha = np.where(np.isinf(m), 0.0, np.exp2((m - mnew) * c))
            skip = ~skipped & (mnew != m) & (Dn > 0)
            alpha = np.where(skip, 1.0, alpha)
            skipped |= skip
            p = np.where(np.isinf(Sv), 0.0, np.exp2((Sv - mnew[None]) * c))
        N = N * alpha[:, None] + p.T @ Vu[a:a + 64]
        Dn = Dn * alpha + p.sum(0)
        m = mnew
    return N, Dn, skipped


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _pattern(rng, k, n):
    """decode live sets, each one a place where kernels go wrong (module docstring); tiles are the 64-token cache blocks"""
    T = (n + 63) // 64
    if k == 0:
        return [n - 1]                                        # only the newest token
    if k == 1:
        return [0]                                            # only token 0
    if k == 2:
        return [t for t in (63, 64) if t < n] or [n - 1]      # both sides of a block boundary
    if k == 3:
        return sorted({n - 1, max(n - 2, 0), (T - 1) * 64})   # first and last token of the newest (partial) block
    if k == 4:                                                # one token in every residue of tile mod 4, at 64- and 32-token tiles
        out = []
        for tile in range(max(T - 4, 0), T):
            for half in (0, 32):
                a, b = tile * 64 + half, min(tile * 64 + half + 32, n)
                if a < b:
                    out.append(int(rng.integers(a, b)))
        return out
    if k == 5:                                                # three tokens inside the middle one of three splits
        per = (T + 2) // 3
        a, b = min(per * 64, (T - 1) * 64), min(2 * per * 64, n)
        b = max(b, a + 1)
        return sorted({int(x) for x in rng.integers(a, min(b, n), 3)})
    if k == 6:                                                # five tokens of the oldest tile: the longest dead-then-rescale walk
        return sorted({int(x) for x in rng.choice(min(64, n), min(5, n), replace=False)})
    return sorted({int(x) for x in rng.choice(n, min(7, n), replace=False)})       # seven tokens anywhere


N_PATTERNS = 8
BOUNDARY = (0, 31, 32, 63, 64, 95, 96, 127, 128)


def _build_seq(case, rng, n, R, hist):
    """one sequence: q [R, Hq, D], K / V [Hkv, nalloc, D]"""
    lat, D, Hkv, G, tier, W = case.lat, case.D, case.Hkv, case.Hq // case.Hkv, case.tier, case.window
    decode = case.kind == 'decode'
    nalloc = (n + 63) // 64 * 64 if decode else n
    P = (D - 2) // 2                                          # (gate, weight) channel pairs; two channels pin the K row's range
    assert G <= P
    kcode = rng.integers(0, lat.ncode + 1, (Hkv, nalloc, D))
    q = np.zeros((R, case.Hq, D), f16)
    c0 = int(-lat.lo / lat.step)                              # code of the value 0
    for hd in range(Hkv):
        perm = rng.permutation(D)
        gate, wch = perm[0:2 * P:2], perm[1:2 * P:2]
        kcode[hd, :, perm[D - 2]] = 0
        kcode[hd, :, perm[D - 1]] = lat.ncode
        kcode[hd][:, gate] = 0                                # everybody dead ...
        live = [set() for _ in range(P)]
        look = [set() for _ in range(P)]                      # window: the token in front of the lower edge LOOKS live
        q[:, hd * G:(hd + 1) * G, perm[D - 2]] = case.q_off   # the offset channel: K holds `lo` there for every token
        if decode:
            wbeg = max(n - W, 0) if W else 0
            for hg in range(G):
                live[hg] = set(_pattern(rng, (hg + hd * G + n) % N_PATTERNS, n))    # those in front of the window look live only
                if W:
                    live[hg].update((wbeg, n - 1))
                    look[hg].update(t for t in (wbeg - 1,) if t >= 0)
                q[0, hd * G + hg, gate[hg]] = QG
                q[0, hd * G + hg, wch[hg]] = lat.q_w(tier)
        else:
            for i in range(R):
                for hg in range(G):
                    p = (i * G + hg) % P
                    live[p].update(t for t in (hist + i, hist + i + 1) if t < n)
                    if W:
                        live[p].update(t for t in (hist + i - W + 1,) if t >= 0)
                        look[p].update(t for t in (hist + i - W,) if t >= 0)
                    q[i, hd * G + hg, gate[p]] = QG
                    q[i, hd * G + hg, wch[p]] = lat.q_w(tier)
            cand = sorted({t for t in BOUNDARY + (hist - 1, hist, n - 1) if 0 <= t < n})
            for p in range(min(P, R * G)):
                live[p].update(int(t) for t in rng.choice(cand, min(3, len(cand)), replace=False))
        for p in range(P):                                    # ... but the live ones
            ts = np.array(sorted(live[p]), np.int64)
            if len(ts):
                kcode[hd, ts, gate[p]] = lat.ncode
                kcode[hd, ts, wch[p]] = c0 + 1 if tier == 'A' else c0 - rng.integers(0, JMAX + 1, len(ts))
        for p in range(P):                                    # in tier B with the top weight
            ts = np.array(sorted(look[p]), np.int64)
            if len(ts):
                kcode[hd, ts, gate[p]] = lat.ncode
                kcode[hd, ts, wch[p]] = c0 + 1 if tier == 'A' else c0
        kcode[hd, n:, :][:, gate] = lat.ncode                 # behind the context: rows that look live to every head
        kcode[hd, n:, :][:, wch] = c0 + 1 if tier == 'A' else c0
    K = (lat.lo + lat.step * kcode).astype(f16)
    vvar = (np.arange(nalloc)[None, :] + rng.integers(0, 3, (Hkv, 1))) % 3         # neighbouring tokens never share a V lattice
    s = Seq(q, K, None, vvar, n, hist)
    s.vcode = rng.integers(1, lat.ncode, (Hkv, nalloc, D))    # 0 and ncode only where the row's range is pinned
    s.vpins = np.stack([rng.permuted(np.tile(np.arange(D), (nalloc, 1)), axis=1)[:, :2] for _ in range(Hkv)])
    hd_, t_ = np.meshgrid(np.arange(Hkv), np.arange(nalloc), indexing='ij')
    s.vcode[hd_, t_, s.vpins[..., 0]] = 0
    s.vcode[hd_, t_, s.vpins[..., 1]] = lat.ncode
    _set_v(case, s)
    return s


def _set_v(case, s):
    lat = case.lat
    vs = np.array([v[0] for v in lat.v])[s.vvar]
    vz = np.array([v[1] for v in lat.v])[s.vvar]
    s.V = (vz[..., None] + vs[..., None] * s.vcode).astype(f16)


def _settle(case, s):
    """move single V codes (never a pinned one) until every output of the sequence is `good` (_round); returns the expectation"""
    lat, G = case.lat, case.Hq // case.Hkv
    rng = np.random.default_rng(s.n)
    for it in range(200):
        bits, strict, good, extra = reference(case, s, check=(it == 0), detail=True)
        bad = np.argwhere(~(good if case.kind == 'decode' else strict))    # prefill rows share too many tokens to reach `good`
        if not len(bad):
            if it:
                reference(case, s, check=True)                # the adjusted V holds the assertions as well
            s.good = good
            return bits, strict
        for r, h, d in bad:                                   # a new code for one live token of that output (never a pinned one)
            hd = h // G
            ts = [t for t in np.flatnonzero(extra[hd][0][:, r * G + h % G]) if d not in s.vpins[hd, t]]
            if ts:
                s.vcode[hd, ts[rng.integers(len(ts))], d] = rng.integers(1, lat.ncode)
            else:                                             # every live token is pinned there: one of them gets its pin elsewhere
                live = np.flatnonzero(extra[hd][0][:, r * G + h % G])
                t = live[rng.integers(len(live))]
                d2 = int(rng.choice([x for x in range(case.D) if x not in s.vpins[hd, t]]))
                s.vcode[hd, t, [d, d2]] = s.vcode[hd, t, [d2, d]]
                s.vpins[hd, t][s.vpins[hd, t] == d] = d2
        _set_v(case, s)
    raise AssertionError('the outputs do not settle away from the fp16 rounding boundaries')


def _assert_round_trip(case, s):
    """assertion 1: quantise -> dequantise returns the fp16 input in both forms, with the (scale, zero) the lattice promises"""
    lat = case.lat
    if case.bits == 16:
        return
    for x, par in ((s.K, None), (s.V, s.vvar)):
        data, p = o.kv_quantize(x, case.bits)
        code = data if case.bits == 8 else o.kv_unpack_int4(data)
        sc = np.full(x.shape[:2], lat.step) if par is None else np.array([v[0] for v in lat.v])[par]
        ze = np.full(x.shape[:2], lat.lo) if par is None else np.array([v[1] for v in lat.v])[par]
        assert np.array_equal(p[..., 0].astype(f64), sc) and np.array_equal(p[..., 1].astype(f64), ze)
        for fn in (o.kv_dequant_decode, o.kv_dequant_flatten):
            assert np.array_equal(fn(code, p[..., 0], p[..., 1]).view(np.uint16), x.view(np.uint16))


def _assert_oracle(case, s):
    """assertion 7: the plain high-precision reference -- o.attention_reference_unfused in fp64 and, in prefill, the tiled
    o.prefill_attention -- rounds to the bits of the integer computation"""
    scale = None if case.tier == 'A' else float(SCALE_B)
    n = s.n
    if case.q_off:                                            # window / sinks: float64 over the cropped context, the sink an extra column
        from tests.attention_window_reference import window_decode, window_prefill
        if case.kind == 'decode':
            ref = window_decode(s.q[0], s.K[:, :n], s.V[:, :n], case.window, scale, case.sinks)[None]
        else:
            ref = window_prefill(s.q, s.K, s.V, s.hist, case.window, scale, case.sinks)
        assert not np.isnan(ref).any()
        ref = ref.view(np.uint16).copy()
        ref[ref == 0x8000] = 0
        assert np.array_equal(ref[s.good], s.bits[s.good]) and ulp16(ref, s.bits)[~s.good].max(initial=0) <= 1, case
        return
    for i in range(s.q.shape[0]):
        ctx = n if case.kind == 'decode' else s.hist + i + 1
        ref = o.attention_reference_unfused(s.q[i], s.K[:, :ctx], s.V[:, :ctx], scale).astype(f16).view(np.uint16).copy()
        ref[ref == 0x8000] = 0
        g = s.good[i]                                         # where the reference's own float32 scale cannot move the rounding
        assert np.array_equal(ref[g], s.bits[i][g]) and ulp16(ref, s.bits[i])[~g].max(initial=0) <= 1, (case, i)
    if case.kind == 'prefill':
        ref = o.prefill_attention(s.q, s.K[:, :n], s.V[:, :n], s.hist, scale).view(np.uint16).copy()
        ref[ref == 0x8000] = 0
        assert np.array_equal(ref[~s.loose], s.bits[~s.loose]) and ulp16(ref, s.bits).max() <= 1


@functools.lru_cache(maxsize=None)
def build(kind, bits, D, Hq, Hkv, tier, shape):
    """shape: decode -> tuple of context lengths; prefill -> (qlens, hist).  Every assertion of the module docstring is made here."""
    return _build(Case(kind, bits, D, Hq, Hkv, tier), (kind, bits, D, Hq, Hkv, tier, shape))


SINK_VALUES = (0.0, -np.inf, -0.0, -65504.0)                  # by head, in turn: neighbouring heads differ by a whole unit of weight
EXP_B = 3                                                     # tier B: the top live weight sits at exponent 3, the sink (logit 0) at 0


@functools.lru_cache(maxsize=None)
def build_window(kind, bits, D, Hq, Hkv, tier, shape, window, with_sinks):
    """the same with a sliding window (0 = none), sinks (SINK_VALUES by head) and the offset channel: q holds q_off where every K row
    holds `lo`, so that the live maximum times scale_log2 is 0 (tier A) or a small integer (tier B, EXP_B for the top weight) and a
    sink logit of 0 is a weight among the live ones"""
    lat = Lattice(bits)
    sinks = np.array([SINK_VALUES[(h + window) % 4] for h in range(Hq)], f16) if with_sinks else None
    if tier == 'A':
        q_off = QG * (lat.hi + lat.step) / -lat.lo            # the live score QG * (hi + step) becomes 0
    else:
        q_off = (QG * lat.hi - 32 * EXP_B) / -lat.lo          # the score of a live token with weight 2^0 becomes 32 * EXP_B
    assert q_off == int(q_off) and f16(q_off) == q_off
    case = Case(kind, bits, D, Hq, Hkv, tier, window=window, sinks=sinks, q_off=int(q_off))
    return _build(case, (kind, bits, D, Hq, Hkv, tier, shape, window, with_sinks))


def _build(case, args):
    kind, shape = case.kind, args[6]
    seed = zlib.crc32(repr(args).encode())
    rng = np.random.default_rng(seed)
    todo = [(n, 1, n - 1) for n in shape] if kind == 'decode' else [(h + n, n, h) for n, h in zip(*shape)]
    total = loose = 0
    for n, R, hist in todo:
        s = _build_seq(case, rng, n, R, hist)
        s.bits, strict = _settle(case, s)
        s.loose = ~strict
        _assert_round_trip(case, s)
        _assert_oracle(case, s)
        total += strict.size
        loose += int(s.loose.sum())
        case.seqs.append(s)
    assert loose * 1000 <= total, f'{loose} of {total} outputs sit on a rounding boundary'                   # assertion 6
    case.total = total
    return case


def decode_case(bits, D, group, tier, klen=KLEN_DECODE):
    Hkv = 1 if group >= 16 else 2
    return build('decode', bits, D, group * Hkv, Hkv, tier, tuple(klen))


def prefill_case(D, group, tier, shape):
    return build('prefill', 16, D, group * 2, 2, tier, shape)


KLEN_WINDOW = (1, 31, 33, 64, 65, 97, 129, 200, 330, 1089)
WINDOWS_DECODE = (1, 32, 33, 64, 100, 4096)
GROUPS_WINDOW = (1, 2, 3, 4, 7, 8)                            # heads per workgroup 1, 2, 3, 4, seven chunks of 1, two chunks of 4
WINDOWS_PREFILL = (1, 16, 17, 32, 33, 64, 65, 100, 4096)


def decode_window_case(bits, D, group, tier, window, with_sinks, klen=KLEN_WINDOW):
    return build_window('decode', bits, D, group * 2, 2, tier, tuple(klen), window, bool(with_sinks))


def prefill_window_case(D, group, tier, shape, window, with_sinks):
    return build_window('prefill', 16, D, group * 2, 2, tier, shape, window, bool(with_sinks))


CONTROL_WINDOW = 33
KLEN_CONTROL = (64, 65, 97, 129, 200, 330)                    # every context longer than CONTROL_WINDOW + 1


def control_case():
    """the device's negative controls: every window starts inside its context (first tokens 31, 32, 64, 96, 167, 297), so a launch
    with W + 1 lets in a token that looks live and one with W - 1 drops a live one in every sequence; launched without its sinks it
    loses a unit of weight in every other head"""
    return decode_window_case(8, 128, 4, 'B', CONTROL_WINDOW, True, KLEN_CONTROL)


def decode_window_cases():
    """thinned: every window in both tiers with every (head_dim, bits); groups and sinks rotate so that every (head_dim, bits) meets
    every group, and every window and every group meet sinks off and on"""
    for di, D in enumerate((128, 64)):
        for bi, bits in enumerate((8, 4, 16)):
            for wi, W in enumerate(WINDOWS_DECODE):
                for ti, tier in enumerate('AB'):
                    yield bits, D, GROUPS_WINDOW[(wi + 3 * ti + bi + di) % 6], tier, W, (wi // 2 + ti + di) % 2


def prefill_window_cases():
    """thinned: every window with every batch shape at every head_dim; tiers, groups and sinks rotate so that every window meets both
    tiers and sinks off and on"""
    for di, D in enumerate((128, 64)):
        for wi, W in enumerate(WINDOWS_PREFILL):
            for si, shape in enumerate(PREFILL_SHAPES):
                yield D, GROUPS_PREFILL[(wi + 2 * si + di) % 5], 'AB'[(wi + si + di) % 2], shape, W, (wi + di + (si + 1) // 2) % 2


def decode_cases():
    for D, bits in ((128, 8), (128, 4), (128, 16), (64, 8), (64, 4), (64, 16)):
        for group in GROUPS_DECODE:
            for tier in 'AB':
                yield bits, D, group, tier


def prefill_cases():
    for D in (128, 64):
        for group in GROUPS_PREFILL:
            for shape in PREFILL_SHAPES:
                for tier in 'AB':
                    yield D, group, tier, shape


# ---- the paged cache, vectorised ------------------------------------------------------------------------------------------------
def fill_cache(pool, L, table, layer, K, V):
    """write K / V fp16 [Hkv, n, D] as tokens 0 .. n - 1 of the sequence with block table `table` into the pool
    (o.PagedKVCache.store_token for every token, without the Python loop)"""
    n = K.shape[1]
    t = np.arange(n)
    blk, ti = np.asarray(table)[t // L.block_len], t % L.block_len
    base = L.layer_offset(layer)
    for hd in range(L.kv_heads):
        for x, doff, poff in ((K[hd], L.k_data(hd, 0), L.k_param(hd, 0)), (V[hd], L.v_data(hd, 0), L.v_param(hd, 0))):
            if L.bits == 16:
                data = np.ascontiguousarray(x).view(np.uint8).reshape(n, -1)
            else:
                data, par = o.kv_quantize(x, L.bits)
                cols = base + poff + ti[:, None] * 4 + np.arange(4)[None, :]
                pool[blk[:, None], cols] = np.ascontiguousarray(par.astype(f16)).view(np.uint8).reshape(n, 4)
            cols = base + doff + ti[:, None] * L.token_data_size + np.arange(L.token_data_size)[None, :]
            pool[blk[:, None], cols] = data
