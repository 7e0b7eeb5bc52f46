"""Exactly summable mixture-of-experts blocks: router, grouped w1w3 with the gated SiLU, grouped w2 and the combine all have
ONE correct bit pattern per output, whatever the row tile, the segment layout, the router or the order of summation.  Plain numpy,
no GPU; built on tests/gemm_exact_reference.py (ExactWeights, model_w, check_budget, to_f16).

Two facts carry the exact construction across the gated SiLU and the softmax.
  1. a saturated gate is exact: every gated epilogue is a / (1.0f + expf(-a)) * u; for a >= 18, 1 + expf(-a) rounds to 1 and the
     quotient is a itself.  The gate accumulators here are powers of two in [32, 256], so act = h(2^g * up) is one fp16 rounding
     of an exact product.
  2. tied integer logits give exact routing weights: the k picked experts of a token all hold the maximum logit, so
     p_j = expf(0) = 1, denom = k, w_j = routed_scale / k -- a power of two for the (k, routed_scale) used here.

x [T][H], integer valued.  Channels 0 .. E-1 are the router logits (the gate matrix is eye(E) on those rows and exactly zero
elsewhere): the picks hold LOGIT_TOP, every other expert a strictly smaller integer.  Channel H-2 (the bias channel) holds 1 or 2
per token -- the only channel the gate (even) columns of w1w3 see, so a row given to the wrong token changes the gate as well as
the up accumulator.  Channel H-1 switches the shared gate: +1 (logit 32, sigma = 1) or -4 (logit -128, expf(128) = inf,
sigma = 1 / inf = 0).  The rest: integers in [-3, 3].

Expert e of a geometry (H, I) (its own seeds: a foreign expert's weights give another integer):
  w1w3 up (odd) columns: ExactWeights' codes q with zeros 4 .. 11 (integers q - z in -11 .. 11) times 2^e,
      e = E0_13 + (group + c[column]) % 2: two adjacent groups of a column never share a scale.  The zeros' range and the spread of
      2 exponents (ExactWeights: 0 .. 15 and 4) keep w2's sums, whose terms carry act's 2^13 range, inside the budget;
  w1w3 gate (even) columns: q == z (a real dequantisation to zero) off the bias row; on it q - z = 2^((j + e) % 3) with scale 2^5
      (the other groups of the column: 2^6), so the gate accumulator is x_bias * {32, 64, 128}, in [32, 256];
  w2: the same construction, exponents E0_2 + (group + c[column]) % 2;
each as u4 (q, s, z), as fp16 [K][N] and as e4m3 codes with power-of-two 128 x 128 block scales (w1w3 in the gated [w1 | w3] form;
'w8' operands: the up columns and w2 take the block exponents, the gate columns are the same in both families).

Expected values, float64 integers with one rounding each: act = h(gate * up), y2 = h(act . W2),
out = h(sum_j y2_j * routed_scale / k [+ shared * sigma]).  Lattices: up accumulators are multiples of 2^E0_13, act of
LA = 2^(5 + E0_13), y2 and `shared` of L2 = LA * 2^E0_2, the combine's terms of L2 * min(1, routed_scale / k); forward() asserts
sum |terms| / lattice <= 2^23 for every accumulator of both GEMMs and of the combine, that act / y2 / out are finite and (when not
zero) normal fp16 numbers, that the gate accumulators are powers of two in [32, 256] and that o.gated_silu_epilogue of the exact
accumulators equals act bit for bit; make_x() asserts that o.moe_gate returns the intended ids in the intended order and weights
of exactly routed_scale / k.

Routings: 'random'; 'one' (expert 3 takes every token, the other picks come from 2 (k - 1) experts, the rest are empty); 'edge'
(expert 1 exactly 2 * hint rows, expert 2 exactly 2 * hint + 1, hint = ceil(T k / E): the launchers' row tile is sized for
2 * hint; needs T >= 2 * hint + 1, with top_k = 1 T >= 4 * hint + 1: not T = 1); 'boundary' (boundary_x, the router alone): the
k-th and (k+1)-th logits tie.

forward(..., mut=) restates the faults this path can have, for the sharpness proofs of tests/test_host_moe_exact.py."""
import functools
import types

import numpy as np

from oracle import tm_oracle as o
from tests import gemm_exact_reference as g

f16, f32, f64 = np.float16, np.float32, np.float64
GEOMETRIES = ((256, 384), (384, 128))                           # (H, I); the second: w2 has 24 column tiles and one k-block
CONFIGS = ((8, 2, 1.0), (8, 1, 2.0), (72, 8, 1.0), (128, 4, 0.5))   # (E, top_k, routed_scale)
TOKENS = (1, 37, 64, 65, 300)
ROUTINGS = ('random', 'one', 'edge')
FAMILIES = ('w', 'w8')                                          # u4 / fp16 operands, e4m3 operands
E0_13, E0_2 = -12, -4
GATE_E = 5                                                      # the gate columns' scale on the bias row: 2^5
LA = 2.0**(GATE_E + E0_13)                                      # act's lattice
L2 = LA * 2.0**E0_2                                             # y2's (and shared's) lattice
BUDGET = 2.0**23
LOGIT_TOP = 3
X_MAX = 3
SHARED_LOGIT = 32                                               # shared-gate weight on the switch channel
MUTATIONS = ('segment', 'dup_row', 'drop13', 'drop2', 'code13', 'code2', 'swap13', 'swap2', 'skip_pair', 'twice_pair', 'no_scale',
             'no_shared', 'shared_sigma0', 'tie_high')


def _fold(e, e0):
    """ExactWeights' exponents e0 + (g + c) % 4 folded to e0 + (g + c) % 2: adjacent groups still never share one"""
    return e0 + (e - e0) % 2


class Expert:
    """expert e of geometry (H, I): w1w3 [H][2 I] with (gate_j, up_j) interleaved columns and w2 [I][H]"""

    def __init__(self, H, I, e):
        assert H % 128 == 0 and I % 128 == 0
        self.H, self.I, self.e = H, I, e
        G, bias = H // 128, H - 2
        a = g.ExactWeights(H, 2 * I, seed=[13, H, I, e], e0=E0_13)
        a.e, a.e8g = _fold(a.e, E0_13), _fold(a.e8g, E0_13)
        gate_e = GATE_E + (bias // 128 - np.arange(G)) % 2                          # 2^5 in the bias row's group, 2^6 next to it
        a.e[:, 0::2] = gate_e[:, None]
        a.e8g[:, :I // 128] = gate_e[:, None]
        self.c = 2**((np.arange(I) + e) % 3)                                        # the gate columns' integer on the bias row
        a.z[:] = 4 + a.z % 8
        a.q[:, 0::2] = np.repeat(a.z[:, 0::2], 128, axis=0)
        a.q[bias, 0::2] += self.c.astype(np.uint8)
        a.wint = (a.q.astype(np.int16) - np.repeat(a.z, 128, axis=0).astype(np.int16))
        b = g.ExactWeights(I, H, seed=[2, H, I, e], e0=E0_2)
        b.e, b.e8 = _fold(b.e, E0_2), _fold(b.e8, E0_2)
        b.z[:] = 4 + b.z % 8
        b.wint = (b.q.astype(np.int16) - np.repeat(b.z, 128, axis=0).astype(np.int16))
        self.a, self.b = a, b
        gate_cols = a.w()[:, 0::2]
        assert np.array_equal(gate_cols[bias], self.c * 2.0**GATE_E) and not np.delete(gate_cols, bias, axis=0).any()
        assert np.array_equal(a.w8(True)[:, 0::2], gate_cols)
        assert (a.wint[:, 0::2] == 0).sum() == (H - 1) * I and (a.q <= 15).all()

    def w13(self, fam):
        return self.a.w() if fam == 'w' else self.a.w8(True)

    def w2(self, fam):
        return self.b.w() if fam == 'w' else self.b.w8()

    def e13(self, fam):
        return self.a.e if fam == 'w' else self.a.e8_columns(True)

    def e2(self, fam):
        return self.b.e if fam == 'w' else self.b.e8_columns()

    def operands(self, fmt):
        """what tm_moe_set_expert is given: (w13 weight, scales, zeros, w2 weight, scales, zeros), None where the format has none"""
        if fmt == 'u4':
            q13, s13, z13 = self.a.u4()
            q2, s2, z2 = self.b.u4()
            return o.pack_u4_row(q13), s13, z13, o.pack_u4_row(q2), s2, z2
        if fmt == 'f16':
            return self.a.f16_weight(), None, None, self.b.f16_weight(), None, None
        assert fmt == 'fp8'
        c13, s13 = self.a.fp8(gated=True)
        c2, s2 = self.b.fp8()
        return c13, s13, None, c2, s2, None

    def dequantised(self, fmt):
        """(w13, w2) fp16 through the oracle's dequantisers: what o.moe_ffn takes"""
        if fmt == 'u4':
            return o.w4a16_dequant(*self.a.u4()), o.w4a16_dequant(*self.b.u4())
        if fmt == 'f16':
            return self.a.f16_weight(), self.b.f16_weight()
        return o.fp8_dequant(*self.a.fp8(gated=True), gated=True), o.fp8_dequant(*self.b.fp8())


@functools.lru_cache(maxsize=160)
def expert(H, I, e):
    return Expert(H, I, e)


def family(fmt):
    return 'w8' if fmt == 'fp8' else 'w'


class Block:
    def __init__(self, H, I, E, k, scale):
        assert E + 2 <= H and k <= E
        self.H, self.I, self.E, self.k, self.scale = H, I, E, k, scale
        self.w = scale / k
        assert np.log2(self.w) == np.round(np.log2(self.w)), 'routed_scale / top_k must be a power of two'
        self.lc = L2 * min(1.0, self.w)                                             # the combine's lattice

    def gate(self):
        gt = np.zeros((self.H, self.E), f16)
        gt[:self.E] = np.eye(self.E, dtype=f16)
        return gt

    def shared_gate(self):
        sg = np.zeros(self.H, f16)
        sg[self.H - 1] = SHARED_LOGIT
        return sg

    def expert(self, e):
        return expert(self.H, self.I, int(e))

    def hint(self, T):
        return (T * self.k + self.E - 1) // self.E

    def feasible(self, T, routing):
        """'edge' needs 2 * hint rows of expert 1 and 2 * hint + 1 of expert 2 (on disjoint tokens when top_k = 1)"""
        if routing != 'edge':
            return True
        a = 2 * self.hint(T)
        return a + 1 <= T if self.k > 1 else 2 * a + 1 <= T


def route(logits, k):
    """top-k on the logits, ties to the lower expert id: the ids in the order (-logit, id)"""
    E = logits.shape[1]
    return np.stack([np.lexsort((np.arange(E), -row))[:k] for row in logits]).astype(np.int32)


def tables(ids, E):
    """offsets [E + 1], f2n [T k], en2f [k][T]: the flat rows are the (token, choice) pairs sorted by expert, tokens ascending"""
    T, k = ids.shape
    order = np.argsort(ids.ravel(), kind='stable')
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids.ravel(), minlength=E))]).astype(np.int32)
    inv = np.empty(T * k, np.int32)
    inv[order] = np.arange(T * k, dtype=np.int32)
    return offsets, (order // k).astype(np.int32), np.ascontiguousarray(inv.reshape(T, k).T)


def _picks(B, T, routing, rng):
    E, k = B.E, B.k
    if routing == 'random':
        return [rng.permutation(E)[:k].tolist() for _ in range(T)], {}
    pool = [0, 6, 1, 7, 4, 5][:2 * (k - 1)] if E == 8 else list(range(8, 8 + 2 * (k - 1)))
    if routing == 'one':
        assert len(pool) == 2 * (k - 1)
        return [[3] + pool[(t % 2) * (k - 1):(t % 2 + 1) * (k - 1)] for t in range(T)], {3: T}
    assert routing == 'edge' and B.feasible(T, routing)
    a = 2 * B.hint(T)
    picks = [[] for _ in range(T)]
    for t in range(a):
        picks[t].append(1)
    for t in range(T - a - 1, T):
        picks[t].append(2)
    others = [0, 3, 4, 5, 6, 7] if E == 8 else list(range(8, E))
    i = 0
    for t in range(T):
        while len(picks[t]) < k:
            picks[t].append(others[i % len(others)])
            i += 1
    return picks, {1: a, 2: a + 1}


def make_x(B, T, routing, seed=0):
    """(x int64 [T][H], ids int32 [T][k] in the router's order); asserts the routing through o.moe_gate"""
    rng = np.random.default_rng([seed, B.H, B.E, B.k, T, ROUTINGS.index(routing)])
    H, E, k = B.H, B.E, B.k
    picks, want = _picks(B, T, routing, rng)
    x = rng.integers(-X_MAX, X_MAX + 1, (T, H)).astype(np.int64)
    x[:, :E] = rng.integers(-X_MAX, LOGIT_TOP, (T, E))                              # strictly below the picks' logit
    ids = np.sort(np.asarray(picks, np.int32), axis=1)                              # tied: the lower id comes first
    assert all(len(set(p)) == k for p in picks)
    x[np.arange(T)[:, None], ids] = LOGIT_TOP
    x[:, H - 2] = rng.integers(1, 3, T)
    x[:, H - 1] = rng.choice([1, -4], T)
    if T > 1:
        x[0, H - 2], x[-1, H - 2] = 1, 2
        x[0, H - 1], x[-1, H - 1] = 1, -4
    check_routing(B, x, ids)
    hist = np.bincount(ids.ravel(), minlength=E)
    assert all(hist[e] == n for e, n in want.items()), f'{routing} T {T}: histogram {hist}'
    return x, ids


def check_routing(B, x, ids):
    assert np.array_equal(route(x[:, :B.E], B.k), ids)
    lg, oid, ow = o.moe_gate(x.astype(f16), B.gate(), B.k, True, B.scale)
    assert np.array_equal(lg, x[:, :B.E].astype(f32)), 'the router logits are not the integers of x'
    assert np.array_equal(oid, ids), 'o.moe_gate does not return the intended ids in the intended order'
    assert np.array_equal(ow.view(np.uint32), np.full(ids.shape, B.w, f32).view(np.uint32)), 'weights are not routed_scale / k'


def sigma_of(x):
    """the shared gate's sigmoid per token: exactly 1 or 0"""
    logit = x[:, -1] * SHARED_LOGIT
    assert ((logit >= 32) | (logit <= -128)).all()
    return (logit >= 32).astype(f64)


def make_shared(B, T, seed=0):
    """fp16 [T][H] on y2's lattice: integers below 2^11 times L2 * 2^(0 .. 10)"""
    rng = np.random.default_rng([seed, 77, B.H, T])
    v = rng.integers(-2047, 2048, (T, B.H)) * L2 * np.exp2(rng.integers(0, 11, (T, B.H)))
    s = v.astype(f16)
    assert np.array_equal(s.astype(f64), v)
    return s


def boundary_x(E, k, T, H, seed=0):
    """(x int64 [T][H], intended ids [T][k]) for the router alone: a experts above a tie group that straddles the k-th place, the
    rest strictly below.  Token t's form is t % 4: 0 a random group and a random number of experts above; 1 (E > 64) the group is
    one lane's experts l, l + 64, ... of the wide kernel and k - 1 experts lie above (the last place is decided inside a lane);
    2 (E > 64) two experts, the lower id in the HIGHER lane (id l_hi against 64 s + l_lo, l_lo < l_hi), k - 1 above; 3 every
    expert ties (the picks are 0 .. k - 1).  Forms 1 and 2 fall back to form 0 at E <= 64."""
    assert k < E and E + 2 <= H
    rng = np.random.default_rng([seed, E, k, T])
    x = rng.integers(-X_MAX, X_MAX + 1, (T, H)).astype(np.int64)
    ids = np.zeros((T, k), np.int32)
    V = 2
    for t in range(T):
        form = t % 4
        if form in (1, 2) and E <= 64:
            form = 0
        if form == 3:
            group, above = np.arange(E), np.zeros(0, np.int64)
        elif form == 1:
            lane = int(rng.integers(0, min(64, E - 64)))
            group = np.arange(lane, E, 64)
            above = rng.permutation(np.setdiff1d(np.arange(E), group))[:k - 1]
        elif form == 2:
            l_lo = int(rng.integers(0, min(63, E - 64)))
            l_hi = int(rng.integers(l_lo + 1, 64))
            s = int(rng.integers(1, (E - 1 - l_lo) // 64 + 1))
            group = np.array([l_hi, 64 * s + l_lo])
            above = rng.permutation(np.setdiff1d(np.arange(E), group))[:k - 1]
        else:
            a = int(rng.integers(0, k))
            m = int(rng.integers(k - a + 1, min(E - a, k - a + 5) + 1))
            perm = rng.permutation(E)
            above, group = perm[:a], np.sort(perm[a:a + m])
        row = rng.integers(V - 5, V, E)
        row[group] = V
        row[above] = V + rng.integers(1, 3, len(above))                             # ties among the experts above are ordered by id too
        x[t, :E] = row
        top = sorted(above.tolist(), key=lambda e: (-row[e], e))
        ids[t] = top + np.sort(group)[:k - len(above)].tolist()
        assert len(above) < k < len(above) + len(group)
    assert np.array_equal(route(x[:, :E], k), ids)
    return x, ids


def _mutated_weights(ex, fam, mut, rng):
    """(w13, w2) of expert `ex` with one fault in an up column of w1w3 or in w2"""
    w13, w2 = ex.w13(fam), ex.w2(fam)
    kind = mut[:-2] if mut[-2:] == '13' else mut[:-1]
    W, w, e_cols = (ex.a, w13, ex.e13(fam)) if mut.endswith('13') else (ex.b, w2, ex.e2(fam))
    K, N = w.shape
    while True:
        k, n = int(rng.integers(0, K)), int(rng.integers(0, N))
        if mut.endswith('13') and (n % 2 == 0 or k >= ex.H - 2):                   # an up column, a channel every token fills
            continue
        if kind == 'drop' and W.wint[k, n] == 0:
            continue
        if kind == 'swap' and len(e_cols) < 2:
            raise ValueError('a linear with one group has no scales to swap')
        break
    wc, ec = g.mutate(W.wint.astype(np.int64), e_cols, W.q, kind, k, n, rng)
    w[:, n] = g.column(wc, ec)
    return w13, w2


def forward(B, fam, x, ids, shared=None, mut=None, seed=0):
    """the whole block in float64 integers.  Returns act [T k][I], y2 [T k][H] (flat rows) and out [T][H], fp16, plus the tables.
    mut: one of MUTATIONS (the budget and lattice assertions run on the unmutated model only)"""
    T, k, E, H, I = len(x), B.k, B.E, B.H, B.I
    rng = np.random.default_rng([seed, 5, T, MUTATIONS.index(mut) if mut else 99])
    check = mut is None
    if mut == 'tie_high':                                                           # token 0's last pick goes to a higher tied id
        assert (x[0, :E] == LOGIT_TOP).sum() > k, 'tie_high needs a (k+1)-th expert at the top logit'
        ids = ids.copy()
        ids[0, k - 1] = np.flatnonzero(x[0, :E] == LOGIT_TOP)[k]
    offsets, f2n, en2f = tables(ids, E)
    P = T * k
    rows_x = x[f2n].astype(f64)
    expert_of = np.repeat(np.arange(E), np.diff(offsets))
    used = np.flatnonzero(np.diff(offsets))
    if mut == 'segment':                                                            # a segment's last row computed by the next expert
        e0 = used[0]
        expert_of[offsets[e0 + 1] - 1] = e0 + 1 if e0 + 1 < E else e0 - 1
    if mut == 'dup_row':                                                            # a segment's first row re-reads its neighbour's last
        cand = [f for f in offsets[used[1:]] if f2n[f] != f2n[f - 1]] if len(used) > 1 else []
        f = cand[0] if cand else next(f for f in range(1, P) if f2n[f] != f2n[f - 1])
        rows_x[f] = rows_x[f - 1]
    hit = int(rng.choice(np.unique(expert_of))) if mut in ('drop13', 'drop2', 'code13', 'code2', 'swap13', 'swap2') else -1
    act, y2 = np.zeros((P, I), f16), np.zeros((P, H), f16)
    worst = [0.0, 0.0, 0.0]
    for e in np.unique(expert_of):
        sel = np.flatnonzero(expert_of == e)
        ex = B.expert(e)
        w13, w2 = _mutated_weights(ex, fam, mut, rng) if e == hit else (ex.w13(fam), ex.w2(fam))
        xe = rows_x[sel]
        acc = xe @ w13
        gate, up = acc[:, 0::2], acc[:, 1::2]
        a = g.to_f16(gate * up)
        if check:
            worst[0] = max(worst[0], g.check_budget(xe, w13, 2.0**E0_13, BUDGET))
            assert np.isin(gate, (32.0, 64.0, 128.0, 256.0)).all(), 'a gate accumulator is not a power of two in [32, 256]'
            assert np.array_equal(o.gated_silu_epilogue(acc.astype(f32)).view(np.uint16), a.view(np.uint16))
            ai = a.astype(f64) / LA
            assert np.array_equal(ai, np.round(ai))
            worst[1] = max(worst[1], g.check_budget(ai, w2, 2.0**E0_2, BUDGET))
        act[sel] = a
        y2[sel] = g.to_f16(a.astype(f64) @ w2)
    w = 1.0 / k if mut == 'no_scale' else B.w
    acc = np.zeros((T, H), f64)
    load = np.zeros((T, H), f64)
    if shared is not None:
        sigma = sigma_of(x)
        if mut == 'shared_sigma0':
            sigma = sigma.copy()
            sigma[np.flatnonzero(sigma == 0)[0]] = 1.0
        if mut != 'no_shared':
            acc += shared.astype(f64) * sigma[:, None]
            load += np.abs(shared.astype(f64)) * sigma[:, None]
    for j in range(k):
        term = w * y2[en2f[j]].astype(f64)
        if mut in ('skip_pair', 'twice_pair') and j == k - 1:
            term[T // 2] *= 0.0 if mut == 'skip_pair' else 2.0
        acc += term
        load += np.abs(term)
    out = g.to_f16(acc + 0.0)
    if check:
        lc = B.lc
        assert np.array_equal(acc / lc, np.round(acc / lc))
        worst[2] = float(load.max() / lc)
        assert worst[2] <= BUDGET, f'the combine is not exactly summable: {worst[2]}'
        for name, v in (('act', act), ('y2', y2), ('out', out)):
            nz = np.abs(v[v != 0].astype(f64))
            assert nz.size and nz.min() >= 2.0**-14, f'{name}: a subnormal fp16 value'
    return types.SimpleNamespace(ids=ids, offsets=offsets, f2n=f2n, en2f=en2f, act=act, y2=y2, out=out, w=np.full((T, k), w, f32),
                                 worst=worst)


def bits(a):
    """uint16 view with -0 mapped to +0"""
    v = np.ascontiguousarray(a).view(np.uint16).copy()
    v[v == 0x8000] = 0
    return v
