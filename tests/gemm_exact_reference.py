"""Exactly summable GEMM operands: every partial sum of x . W is representable in fp32, so the result does not depend on the
order of summation -- every tiling, split count, merge order and weight layout must return the SAME bits, namely the one fp16
rounding of an integer that numpy computes here.  Plain numpy, no GPU.

Weights.  W[k][n] = Wint[k][n] * 2^e[g][n], g = k // 128, Wint = q - z with q drawn per (k, n) and z per (group, column) uniformly
in 0 .. 15, and e = e0 + (g + c[n]) % 4 with c[n] drawn per column: two adjacent groups of a column NEVER share a scale, two
adjacent columns share one with probability 1 / 4 and a zero with probability 1 / 16 -- a neighbour's scale or zero gives another
integer.  u4 operands: (q, s = 2^e, z), whose on-chip dequantisation h(fma(h(q), s, h(-z s))) is exactly Wint * 2^e.  The fp16
linear takes W itself.  The e4m3 linears take Wint as codes (integers up to 15 are exact in e4m3) with power-of-two 128 x 128
block scales 2^e8[g][n // 128], e8 = e0 + (g + c8[block]) % 4, also in the gated [w1 blocks | w3 blocks] form.  With e0 >= -14
every non-zero |W| is a normal fp16 number.

Dense activations.  x integer in [-7, 7], at least one +-7 in every (row, 128-channel group): the fp8 activation quantiser then
finds absmax 7, scale 7 / 448 = 2^-6 and codes e4m3(64 x), all exact.

Few-hot sweep.  Launch t, row m takes pair p = (t M + m) mod K / 2 and holds two non-zeros in group p % G at offsets p // G and
p // G + 64, one of them +-7: over ceil(K / (2 M)) launches every k index is hit by some row (K = 4096, M = 64: 32 launches),
and every output is a sum of two terms, below 2^11 units of its scale: exact in fp16, so a single wrong term always shows.

Budget.  With lsb = 2^e0 (it divides every term) the builder asserts sum_k |x| |W| / lsb <= 2^23 for every output (few-hot:
< 2^11) and refuses anything else; sums are taken in float64 (exact: 2^23 < 2^53) and rounded to fp16 once."""
import functools

import numpy as np

from oracle import tm_oracle as o

f16, f32, f64 = np.float16, np.float32, np.float64
GROUP = 128
E0_PLAIN = -6                     # exponents -6 .. -3: K = 4096 outputs of sigma ~ 130, 3 to 4 bits below the fp16 ulp are rounded away
E0_GATED = -12                    # exponents -12 .. -9: K = 4096 accumulators of sigma ~ 2, SiLU is not saturated
DENSE_BUDGET = 2.0**23
FEWHOT_BUDGET = 2.0**11
# (K, N) of both test modules: 3 and 14 k-blocks (no whole stages), 5 x 32 columns, 48 columns (the general kernel only)
SHAPES = ((384, 64), (1024, 160), (1792, 512), (4096, 1024), (384, 48))
GATED_SHAPE = (4096, 1024)
X_SEED = 20240


class ExactWeights:
    """the integer weights of one K x N linear and their u4 / fp16 / e4m3 operands"""

    def __init__(self, K, N, seed, e0=E0_PLAIN):
        assert K % GROUP == 0 and N % 16 == 0 and -14 <= e0 and e0 + 3 <= 0, (K, N, e0)
        rng = np.random.default_rng(seed)
        G, NB = K // GROUP, (N + 127) // 128
        self.K, self.N, self.G, self.e0 = K, N, G, e0
        self.q = rng.integers(0, 16, (K, N)).astype(np.uint8)
        self.z = rng.integers(0, 16, (G, N)).astype(np.uint8)
        self.wint = self.q.astype(np.int64) - np.repeat(self.z, GROUP, axis=0).astype(np.int64)
        g = np.arange(G)[:, None]
        self.e = e0 + (g + rng.integers(0, 4, N)[None, :]) % 4                      # [G][N]
        self.e8 = e0 + (g + rng.integers(0, 4, NB)[None, :]) % 4                    # [G][NB]: plain e4m3 block scales
        self.e8g = None
        if N % 256 == 0:                                                            # gated e4m3: [w1 blocks | w3 blocks]
            self.e8g = e0 + (g + rng.integers(0, 4, N // 128)[None, :]) % 4
        self.lsb = 2.0**e0

    # ---- exact operands (float64) ----
    def w(self):
        return model_w(self.wint, self.e)

    def w8(self, gated=False):
        return model_w(self.wint, self.e8_columns(gated))

    def e8_columns(self, gated=False):
        """the e4m3 linears' exponent per column [G][N]"""
        if not gated:
            return np.repeat(self.e8, 128, axis=1)[:, :self.N]
        assert self.e8g is not None, 'gated e4m3 needs N % 256 == 0'
        half = self.N // 256
        out = np.empty((self.G, self.N), np.int64)
        out[:, 0::2] = np.repeat(self.e8g[:, :half], 128, axis=1)
        out[:, 1::2] = np.repeat(self.e8g[:, half:], 128, axis=1)
        return out

    # ---- what the library is given ----
    def u4(self):
        """(q uint8 [K][N], scales fp16 [G][N], zeros fp16 [G][N])"""
        return self.q, np.exp2(self.e.astype(f64)).astype(f16), self.z.astype(f16)

    def f16_weight(self):
        w = self.w()
        w16 = w.astype(f16)
        assert np.array_equal(w16.astype(f64), w)
        return w16

    def fp8(self, gated=False):
        """(e4m3 codes [K][N], fp32 block scales [G][ceil(N / 128)])"""
        codes = o.fp8_e4m3_from_f32(self.wint.astype(f32))
        assert np.array_equal(o.fp8_e4m3_to_f32(codes).astype(np.int64), self.wint)
        return codes, np.exp2((self.e8g if gated else self.e8).astype(f64)).astype(f32)


def model_w(wint, e_cols):
    """Wint [K][N] * 2^e [K / 128][N] in float64 (exact); every non-zero magnitude is a normal fp16 number"""
    w = wint.astype(f64) * np.exp2(np.repeat(e_cols, GROUP, axis=0).astype(f64))
    nz = np.abs(w[w != 0])
    assert nz.size == 0 or nz.min() >= 2.0**-14, 'a non-zero weight below the normal fp16 range'
    return w


def dense_x(M, K, seed):
    """integer x [M][K] in [-7, 7] with at least one +-7 in every (row, group)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-7, 8, (M, K)).astype(np.int64)
    G = K // GROUP
    pos = rng.integers(0, GROUP, (M, G)) + np.arange(G)[None, :] * GROUP
    x[np.arange(M)[:, None], pos] = rng.choice([-7, 7], (M, G))
    assert (np.abs(x.reshape(M, G, GROUP)).max(axis=2) == 7).all()
    return x


def fewhot_launches(K, M):
    return -(-(K // 2) // M)


def fewhot_rows(K, M, t, seed=0):
    """launch t of the sweep: (k0, k1, x0, x1) per row"""
    G, P = K // GROUP, K // 2
    p = (t * M + np.arange(M)) % P
    k0 = (p % G) * GROUP + p // G
    k1 = k0 + 64
    rng = np.random.default_rng([seed, K, M, t])
    seven = rng.choice([-7, 7], M)
    other = rng.integers(1, 8, M) * rng.choice([-1, 1], M)
    first = (p + t) % 2 == 0                                   # which of the two holds the +-7
    return k0, k1, np.where(first, seven, other), np.where(first, other, seven)


def fewhot_x(K, M, t, seed=0):
    k0, k1, x0, x1 = fewhot_rows(K, M, t, seed)
    x = np.zeros((M, K), np.int64)
    x[np.arange(M), k0] = x0
    x[np.arange(M), k1] = x1
    return x


def fewhot_coverage(K, M):
    """how many rows of the whole sweep hit each k"""
    hit = np.zeros(K, np.int64)
    for t in range(fewhot_launches(K, M)):
        k0, k1, _, _ = fewhot_rows(K, M, t)
        np.add.at(hit, k0, 1)
        np.add.at(hit, k1, 1)
    return hit


def check_budget(x, w, lsb, budget, strict=False):
    """sum_k |x| |W| / lsb per output against the budget; raises on a shape that breaks it"""
    assert np.array_equal(np.round(w / lsb), w / lsb), 'lsb does not divide every weight'
    load = (np.abs(x).astype(f64) @ np.abs(w)) / lsb
    worst = float(load.max(initial=0.0))
    if (worst >= budget) if strict else (worst > budget):
        raise ValueError(f'operands are not exactly summable: sum |x| |W| / lsb = {worst} against a budget of {budget}')
    return worst


def exact_acc(x, w, lsb, budget=DENSE_BUDGET, strict=False):
    """float64 accumulators of x . W, exact; refuses operands over the budget"""
    check_budget(x, w, lsb, budget, strict)
    acc = x.astype(f64) @ w
    assert np.array_equal(acc.astype(f32).astype(f64), acc)     # representable in fp32 (follows from the budget)
    return acc


def to_f16(acc):
    """the one rounding; finite"""
    with np.errstate(over='raise'):
        y = acc.astype(f16)
    assert np.isfinite(y).all()
    return y


def expected(x, w, lsb, gated=False):
    """fp16 [M][N] (gated: [M][N / 2] = o.gated_silu_epilogue of the exact fp32 accumulators)"""
    acc = exact_acc(x, w, lsb)
    return o.gated_silu_epilogue(acc.astype(f32)) if gated else to_f16(acc)


def fewhot_expected(K, M, t, w, lsb, seed=0):
    """fp16 [M][N] of launch t: two terms per output, under 2^11 units, exactly representable in fp16"""
    x = fewhot_x(K, M, t, seed)
    k0, k1, x0, x1 = fewhot_rows(K, M, t, seed)
    acc = x0[:, None] * w[k0] + x1[:, None] * w[k1] + 0.0     # (+ 0.0: an accumulator that starts at +0 never ends at -0)
    y = acc.astype(f16)
    assert np.array_equal(y.astype(f64), acc), 'a few-hot output is not exactly representable in fp16'
    return x, y


def fewhot_check_budget(K, M, wint):
    """(|x0| |Wint[k0]| + |x1| |Wint[k1]|) < 2^11 for every output of the sweep, in units of the group's own scale"""
    worst = 0
    for t in range(fewhot_launches(K, M)):
        k0, k1, x0, x1 = fewhot_rows(K, M, t)
        assert np.array_equal(k0 // GROUP, k1 // GROUP)
        load = np.abs(x0)[:, None] * np.abs(wint[k0]) + np.abs(x1)[:, None] * np.abs(wint[k1])
        worst = max(worst, int(load.max()))
    if worst >= FEWHOT_BUDGET:
        raise ValueError(f'few-hot outputs of up to {worst} units: not below 2^11')
    return worst


# ---- mutations of the numpy model (the faults a tiling can have), for the sharpness tests ----
def mutate(wint, e_cols, q, kind, k, n, rng):
    """returns (Wint column n, e column n) after one fault at (k, n): 'code' = one code off by +-1, 'drop' = the k term missing,
    'swap' = the scales of the site's group and the next one (the previous one for the last group) exchanged"""
    wc, ec = wint[:, n].copy(), e_cols[:, n].copy()
    if kind == 'code':
        d = 1 if q[k, n] == 0 else -1 if q[k, n] == 15 else int(rng.choice([-1, 1]))
        wc[k] += d
    elif kind == 'drop':
        wc[k] = 0
    elif kind == 'swap':
        g = k // GROUP
        g2 = g + 1 if g + 1 < len(ec) else g - 1
        ec[g], ec[g2] = ec[g2], ec[g]
    else:
        raise ValueError(kind)
    return wc, ec


def column(wc, ec):
    return wc.astype(f64) * np.exp2(np.repeat(ec, GROUP).astype(f64))


@functools.lru_cache(maxsize=None)
def weights(K, N, gated=False):
    """the one set of weights per (shape, plain | gated) that every test shares; the seeds are fixed"""
    return ExactWeights(K, N, seed=K * 31 + N + (7 if gated else 0), e0=E0_GATED if gated else E0_PLAIN)
