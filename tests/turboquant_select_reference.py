"""TurboQuant decode attention (csrc/attention_decode_tq.hip, quant_policy 42) by WHICH TOKENS each head attends.  Plain numpy, no GPU.

The kernel cannot be held bit for bit (the value side multiplies non-dyadic centroids by fp32(n / sqrt(128)) and the output passes an
fp32 butterfly), but its structure can: here the softmax weights are exactly 1 on a chosen LIVE set and exactly 0 elsewhere, so the
output of a (sequence, head) is the plain mean of its live V rows, and one dropped, doubled or foreign token moves it by 1 / L of a row.

K rows are Walsh patterns.  With w_j = row j of H (tests/turboquant_reference.py), a token of CLASS j has K codes idx = 7, s = 1
where w_j > 0 and idx = 0, s = 0 where w_j < 0, params (n, g) = (power of two >= 1, 0): in the rotated domain the row is
+-n * fp16(c3[7] / sqrt(128)) with the signs of w_j.  A head that listens to class j has q = 2048 * e_j in the original domain; the
kernel's own rotation gives H q = 2048 * w_j exactly (sums with zeros) and q' = fp16(fp32(2048) * kTqRsqrtD) * w_j = 181 * w_j.  A
token of class j then scores S = n * 128 * 181 * 0.19018... = n * 4406.2 (every product and partial sum an fp32 number, the same
instruction sequence for every token), a token of another class scores 0 (w_j . w_k = 0), a NEGATED row (codes swapped) scores -S.
With sc = log2(e) / sqrt(128) the gap S * sc >= 561 is far beyond the <= -150 at which exp2 returns 0: live weights are exp2(0) = 1,
dead weights 0, every rescale factor 1 or 0, the denominator the number of live tokens, every merge across lanes, waves and splits
adds zeros or weights 1.  (q = 512 * e_j would give a gap of 140: too small.)

V rows are random: all four codes, fp16 norms drawn from [0.25, 4] without repetition per (sequence, kv head), one live token per
case with norm 0.  The expected row is the float64 mean over the live tokens of tq.dequant_original(V codes, V params); the bound is
the project's own for a TurboQuant row that passes the fp32 butterfly once and is rounded to fp16 once, 2^-10 * max |expected row|
(tests/test_gpu_turboquant.py).  Of that the fp16 rounding takes 2^-11; the kernel's fp16 V centroids (0x3e0b, 0x373f) sit
2.1e-4 = 0.22 * 2^-10 above C2, both by the same factor, so the whole row is scaled by it; butterfly and accumulation noise
(<= (7 * 11.3 + L) * 2^-24) is nothing.

Dead tokens: rows of classes no head of the kv head listens to (any n up to 2^15, g != 0 allowed), rows of a class ANOTHER head of
the group listens to (live there, dead here), negated live rows, and in the newest block the rows behind the context, which hold in
turn the pattern that scores highest for each head of the group, with n = 64 and V norm 64: they look live and would dominate.
Everything else in the pool is 0xFF (fill_pool).

Liveness is not stored: derive() reads it off q and K in float64 (tq.dequant_rotated against the fp16 q'), asserts that it is the
set the builder meant, that all live scores are equal, that every dead token of the context lies at least 2 * 150 / sc below, that a
live set has 1 .. 40 tokens, and SENSITIVITY: removing any single live token, or adding with weight 1 any single dead token of the
context or the first row behind it, moves the expected row by more than 4 x the bound in some channel (V norms are redrawn where not;
the count is kept and must stay below 1 % of the rows).

Cases: Hkv = 2, one case per GQA group 1 .. 8, 10 (every HPW instantiation of the kernel with one head chunk and with several), 13
sequences with contexts 1 .. 1089 in one launch.  Head h of sequence b takes live-set pattern (h + b) % 8 (_pattern); heads whose
sets overlap settle it smallest set first, a head left without a token shares the class of the newest token's owner (context 1: all
heads attend the one token; there heads with odd h + kv head use q = -2048 * e_j, the one place with a negative maximum, which is
what makes a never-written split slot that reads as zeros show).  The two kv heads draw their classes from one list shifted by one:
head h of kv head 1 listens to the class of head h + 1 of kv head 0.  The SWEEP case holds eleven sequences of context 300 whose
token -> head assignment is rolled by 29 positions each: over the module every position 0 .. 299 is live for one head and dead for
another of the same group (asserted, coverage_300)."""
import functools
from dataclasses import dataclass, field

import numpy as np

from tests import turboquant_reference as tq

f16, f32, f64 = np.float16, np.float32, np.float64
D, HKV, LAYERS, LAYER, TILE, BLOCK = 128, 2, 2, 1, 32, 64
CONTEXTS = (1, 31, 32, 33, 64, 65, 127, 128, 129, 160, 257, 300, 1089)
GROUPS = (1, 2, 3, 4, 5, 6, 7, 8, 10)
SPLITS = (1, 2, 3, 16)
SWEEP_GROUP, SWEEP_CTX = 8, 300
SWEEP_SHIFTS = tuple(29 * i for i in range(11))       # the 32-token live tile moves by 29: 10 * 29 + 32 >= 300
QMAG = 2048
LOOK_N = 64                                           # K n and V norm of the look-alive rows behind the context
MAX_LIVE = 40
RSQRT_D = f32(0.08838834764831845)                    # kTqRsqrtD (csrc/turboquant.h)
SC = f32((f32(1.0) / np.sqrt(f32(D))) * f32(1.4426950408889634))   # scale_log2 as c_api.hip forms it for softmax_scale = 0
DEAD_GAP = 2 * 150 / float(SC)
BOUND_REL = 2.0 ** -10
NAN16 = 0x7e00
H = tq.hadamard(D)
_NORM_GRID = np.arange(0x3400, 0x4401, dtype=np.uint16).view(f16)   # every fp16 in [0.25, 4]


def hpw_chunks(group):
    """(heads per workgroup, head chunks) as launch_decode_attention_tq picks them"""
    hpw = next(c for c in (4, 3, 2, 1) if group % c == 0)
    return hpw, group // hpw


def where(ctx, t, splits):
    """(tile, wave, split) that token t of a context passes through in the kernel"""
    tiles = (ctx + TILE - 1) // TILE
    per = (tiles + splits - 1) // splits
    tile = t // TILE
    split = tile // per
    tile_end = min((split + 1) * per, tiles)
    return tile, (tile_end - 1 - tile) % 4, split     # one split: wave = (tiles - 1 - tile) % 4


def rotate_q(q):
    """fp16 [..., D] -> the kernel's q' = fp16(fp32(H q) * kTqRsqrtD)"""
    return ((np.asarray(q, f16).astype(f64) @ H).astype(f32) * RSQRT_D).astype(f16)


def _pattern(p, ctx):
    t = np.arange(ctx)
    tiles = (ctx + TILE - 1) // TILE
    if p == 0:                                        # the newest token
        return t[-1:]
    if p == 1:                                        # the oldest token
        return t[:1]
    if p == 2:                                        # both sides of every tile boundary
        return t[(t % TILE == TILE - 1) | (t % TILE == 0)][-MAX_LIVE:]
    if p == 3:                                        # one token per tile, every wave and every split
        s = np.array([TILE * k + (5 * k) % TILE for k in range(tiles)])
        return s[s < ctx][-MAX_LIVE:]
    if p == 4:                                        # the (partial) newest tile
        return t[TILE * (tiles - 1):]
    if p == 5:                                        # one whole tile in the middle
        full = ctx // TILE
        return t[TILE * (full // 2): TILE * (full // 2) + TILE] if full else t[:0]
    if p == 6:                                        # ctx - 2 and the first token of every block: the block-table index
        return t[(t % BLOCK == 0) | (t == ctx - 2)][-MAX_LIVE:]
    return TILE * (tiles - 2) + np.arange(8, 16) if tiles >= 2 else t[:0]   # 7: one load-instruction row, all tg, one r


def _assign(ctx, group, b):
    """-> owner int [ctx] (the head of the group a token is live for, -1: none), leader int [group] (the head whose class head h
    listens to: itself unless it was left without a token)"""
    want = [_pattern((h + b) % 8, ctx) for h in range(group)]
    owner = np.full(ctx, -1)
    leader = np.arange(group)
    empty = []
    for h in sorted(range(group), key=lambda h: (len(want[h]), h)):
        free = want[h][owner[want[h]] < 0]
        if len(free):
            owner[free] = h
        else:
            empty.append(h)
    for h in empty:                                   # falls back to the newest token
        if owner[ctx - 1] < 0:
            owner[ctx - 1] = h
        else:
            leader[h] = owner[ctx - 1]
    return owner, leader


@dataclass
class Seq:
    ctx: int
    nalloc: int              # rows written: the context rounded up to its block (the rows behind it look live)
    q: np.ndarray            # fp16 [Hq, D]
    kcodes: np.ndarray       # uint8 [Hkv, nalloc, D]
    kpar: np.ndarray         # fp16 [Hkv, nalloc, 2]
    vcodes: np.ndarray
    vpar: np.ndarray
    meant: list              # per q head: the live set the builder meant (derive() asserts it is what the scores say)
    live: list = None        # per q head: sorted token positions, read off the scores
    vo: np.ndarray = None    # float64 [Hkv, nalloc, D]: V rows in the original domain
    expected: np.ndarray = None   # float64 [Hq, D]
    bound: np.ndarray = None      # float64 [Hq]


@dataclass
class Case:
    group: int
    name: str
    seqs: list = field(default_factory=list)
    redraws: int = 0

    @property
    def Hq(self):
        return HKV * self.group

    @property
    def klen(self):
        return [s.ctx for s in self.seqs]

    @property
    def rows(self):
        return sum(HKV * s.ctx for s in self.seqs)


def _class_row(cls, negated):
    """K codes uint8 [D] of a token of class `cls`"""
    pos = (H[cls] > 0) != bool(negated)
    return np.where(pos, 15, 0).astype(np.uint8)


def _build_seq(rng, pool, ctx, group, b, shift=0):
    nalloc = -(-ctx // BLOCK) * BLOCK
    owner, leader = _assign(ctx, group, b)
    owner = np.roll(owner, shift)
    Hq = HKV * group
    q = np.zeros((Hq, D), f16)
    kcodes = np.zeros((HKV, nalloc, D), np.uint8)
    kpar = np.zeros((HKV, nalloc, 2), f16)
    vcodes = rng.integers(0, 4, (HKV, nalloc, D)).astype(np.uint8)
    vpar = np.zeros((HKV, nalloc, 2), f16)
    meant = []
    for kv in range(HKV):
        cls = [int(pool[(h + kv) % len(pool)]) for h in range(group)]          # kv head 1: the classes of kv head 0 shifted by one
        foreign = [int(c) for c in pool if int(c) not in cls]
        neg = [ctx == 1 and (h + kv) % 2 == 1 for h in range(group)]           # q = -2048 e_j: the maximum score is negative
        nlive = [(1, 2, 4)[h % 3] for h in range(group)]
        for h in range(group):
            q[kv * group + h, cls[leader[h]]] = -QMAG if neg[h] else QMAG
            meant.append(np.flatnonzero(owner == leader[h]))
        for t in range(ctx):
            h = owner[t]
            if h >= 0:                                                         # live for head h (and the heads it leads)
                kcodes[kv, t], kpar[kv, t] = _class_row(cls[h], False), (nlive[h], 0)
            elif rng.random() < 0.6:                                           # a class nobody here listens to
                kcodes[kv, t] = _class_row(foreign[rng.integers(len(foreign))], rng.random() < 0.5)
                kpar[kv, t] = (2.0 ** rng.integers(0, 16), rng.choice([0.0, 0.0078125, 0.03125, 0.05]))
            else:                                                              # a negated live row
                h = int(rng.integers(group))
                kcodes[kv, t], kpar[kv, t] = _class_row(cls[leader[h]], not neg[h]), (nlive[leader[h]] * 2.0 ** rng.integers(0, 4), 0)
        for t in range(ctx, nalloc):                                           # behind the context: what scores highest for each head in turn
            h = (t - ctx) % group
            kcodes[kv, t], kpar[kv, t] = _class_row(cls[leader[h]], neg[h]), (LOOK_N, 0)
        vpar[kv, :ctx, 0] = rng.choice(_NORM_GRID, ctx, replace=False)
        vpar[kv, ctx:, 0] = LOOK_N
    return Seq(ctx, nalloc, q, kcodes, kpar, vcodes, vpar, meant)


def scores(s, group):
    """float64 [Hq, nalloc]: q' . K^ from the stored bytes, every row summed in the same order"""
    qr = rotate_q(s.q).astype(f64)
    out = np.empty((len(s.q), s.nalloc))
    for kv in range(HKV):
        kr = tq.dequant_rotated(s.kcodes[kv], s.kpar[kv], True)
        for h in range(kv * group, (kv + 1) * group):
            out[h] = (kr * qr[h]).sum(-1)
    return out


def _moves(s, kv, live):
    """float64 [ncand]: for every token of the context and the first row behind it, the largest channel change of the mean row when
    that token is removed from (live) or added with weight 1 to (dead) the live set"""
    ncand = min(s.ctx + 1, s.nalloc)
    L = len(live)
    v = s.vo[kv, :ncand]
    mu = s.vo[kv, live].mean(0)
    move = np.abs(v - mu).max(-1) / (L + 1)
    move[live] = np.abs(v[live] - mu).max(-1) / (L - 1) if L > 1 else np.inf    # removing the only token leaves 0 / 0
    return move


def derive(case, rng):
    """live sets, expected rows and bounds of every sequence; asserts the conditions (module docstring), redraws V norms for
    sensitivity"""
    g = case.group
    for b, s in enumerate(case.seqs):
        S = scores(s, g)[:, :s.ctx]
        s.live = []
        for h in range(case.Hq):
            top = S[h].max()
            live = np.flatnonzero(S[h] == top)
            dead = np.delete(S[h], live)
            what = f'{case.name} sequence {b} (context {s.ctx}) head {h}'
            assert np.array_equal(live, s.meant[h]), f'{what}: live set {live} is not the one meant {s.meant[h]}'
            assert 1 <= len(live) <= MAX_LIVE, f'{what}: {len(live)} live tokens'
            assert not len(dead) or top - dead.max() >= DEAD_GAP, f'{what}: a dead token only {top - dead.max()} below the live score'
            s.live.append(live)
        for _ in range(20):
            s.vo = tq.dequant_original(s.vcodes, s.vpar, False)
            s.expected = np.stack([s.vo[h // g, s.live[h]].mean(0) for h in range(case.Hq)])
            s.bound = BOUND_REL * np.abs(s.expected).max(-1)
            weak = set()
            for h in range(case.Hq):
                weak |= {(h // g, int(t)) for t in np.flatnonzero(_moves(s, h // g, s.live[h]) <= 4 * s.bound[h])}
            if not weak:
                break
            for kv, t in weak:
                free = np.setdiff1d(_NORM_GRID, s.vpar[kv, :, 0])
                s.vpar[kv, t, 0] = rng.choice(free)
            case.redraws += len(weak)
        else:
            raise AssertionError(f'{case.name} sequence {b}: sensitivity not reached')
    assert case.redraws < 0.01 * case.rows, f'{case.name}: {case.redraws} V norms redrawn of {case.rows} rows'


def _zero_norm(case):
    """one live token of the case gets V norm 0 (n = 0: a row of +0, never NaN), in a live set of three or more"""
    for s in case.seqs:
        if s.ctx < 2 * TILE:
            continue
        for h, live in enumerate(s.meant):
            if len(live) >= 3:
                s.vpar[h // case.group, live[len(live) // 2], 0] = 0
                return
    raise AssertionError(f'{case.name}: no live set of three tokens')


@functools.lru_cache(maxsize=None)
def build(group, sweep=False):
    """the case of a GQA group (13 sequences, CONTEXTS), or the sweep case (SWEEP_SHIFTS); built once, never changed"""
    rng = np.random.default_rng(4200 + 100 * group + sweep)
    case = Case(group, f'group {group}' + (' sweep' if sweep else ''))
    pool = rng.permutation(np.arange(1, D))[:group + 8]                         # classes: heads first, the rest foreign
    if sweep:
        b = CONTEXTS.index(SWEEP_CTX)
        case.seqs = [_build_seq(rng, pool, SWEEP_CTX, group, b, shift) for shift in SWEEP_SHIFTS]
    else:
        case.seqs = [_build_seq(rng, pool, ctx, group, b) for b, ctx in enumerate(CONTEXTS)]
    _zero_norm(case)
    derive(case, rng)
    print(f'[tq select] {case.name}: {len(case.seqs)} sequences, {case.rows} rows, {case.redraws} V norms redrawn')
    return case


def all_cases():
    return [build(g) for g in GROUPS] + [build(SWEEP_GROUP, True)]


def coverage_300():
    """bool [300]: positions of a context-300 sequence that are live for some head and dead for another head of the same group, over
    every case of the module"""
    covered = np.zeros(SWEEP_CTX, bool)
    for case in all_cases():
        for s in case.seqs:
            if s.ctx != SWEEP_CTX:
                continue
            for kv in range(HKV):
                m = np.zeros((case.group, SWEEP_CTX), bool)
                for h in range(case.group):
                    m[h, s.live[kv * case.group + h]] = True
                covered |= m.any(0) & ~m.all(0)
    return covered


# ---- the pool ----------------------------------------------------------------------------------------------------------------------
def tables(case, spare=2):
    """shuffled block tables with `spare` blocks nobody owns -> (tables, total blocks)"""
    rng = np.random.default_rng(case.group)
    nblk = [s.nalloc // BLOCK for s in case.seqs]
    perm = rng.permutation(sum(nblk) + spare)
    tabs, off = [], 0
    for nb in nblk:
        tabs.append(perm[off:off + nb])
        off += nb
    return tabs, len(perm)


def fill_pool(case, tabs, total):
    """uint8 [total, block_size]: the bytes of every sequence written by layout offsets into layer LAYER, 0xFF everywhere else"""
    L = tq.TqBlockLayout(LAYERS, HKV)
    pool = np.full((total, L.block_size), 0xFF, np.uint8)
    base = L.layer_offset(LAYER)
    for s, tab in zip(case.seqs, tabs):
        kb, vb = tq.pack_k(s.kcodes), tq.pack_v(s.vcodes)                       # [Hkv, nalloc, 64 / 32]
        for j, blk in enumerate(tab):
            sl = slice(j * BLOCK, (j + 1) * BLOCK)
            for hd in range(HKV):
                for off, rows in ((L.k_data(hd, 0), kb[hd, sl]), (L.v_data(hd, 0), vb[hd, sl]),
                                  (L.k_param(hd, 0), s.kpar[hd, sl].view(np.uint8)), (L.v_param(hd, 0), s.vpar[hd, sl].view(np.uint8))):
                    pool[blk, base + off: base + off + rows.size] = rows.reshape(-1)
    return pool


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def ratios(case, b, got):
    """float64 [Hq]: worst |got - expected| / bound per head of sequence b (a NaN or a difference against a zero bound: inf)"""
    s = case.seqs[b]
    err = np.abs(np.asarray(got).astype(f64).reshape(case.Hq, D) - s.expected)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / s.bound[:, None])
    return np.where(np.isnan(r), np.inf, r).max(-1)


def explain(case, b, h, got_row, splits):
    """the worst channel and the single-token change (least squares over removing one live token or adding one other row with weight
    1) that explains got - expected best, with the tile, wave and split that token passes through"""
    s = case.seqs[b]
    kv, live = h // case.group, s.live[h]
    got_row = np.asarray(got_row).astype(f64)
    ch = int(np.nanargmax(np.where(np.isnan(got_row), np.inf, np.abs(got_row - s.expected[h]))))
    msg = f'live set {live.tolist()}; channel {ch}: got {float(got_row[ch])!r}, expected {float(s.expected[h, ch])!r} (bound {s.bound[h]:.3e})'
    if not np.isfinite(got_row).all():
        return msg + '; the row is not finite: a partial that was never written, or a row whose weights are all 0'
    L = len(live)
    mu = s.expected[h]
    delta = (s.vo[kv] - mu) / (L + 1)
    delta[live] = (mu - s.vo[kv, live]) / (L - 1) if L > 1 else np.inf
    res = ((delta - (got_row - mu)) ** 2).sum(-1)
    t = int(np.argmin(res))
    tile, wave, split = where(max(s.ctx, t + 1), t, splits)           # a row behind the context: where a context that long puts it
    kind = 'removing live' if t in live else ('adding the row behind the context,' if t >= s.ctx else 'adding dead')
    return msg + (f'; best single-token explanation: {kind} token {t} (tile {tile}, wave {wave}, split {split}), residual '
                  f'{np.sqrt(res[t]):.3e} of {np.linalg.norm(got_row - mu):.3e}')
