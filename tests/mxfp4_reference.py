"""MXFP4 experts and the gpt-oss MoE block in plain numpy: the specification the kernels of gemm_mxfp4.hip / moe.hip are held to.

Arithmetic (the reference's fp16 path: kernels/gemm/transform.h:83-90, cast.cu:220-227, activation.cu:17-24,
moe_ffn_layer.cc:43-53,272-275,310-313, moe_utils_v2.cu:1032-1105):
  code c in 0..15: sign c >> 3, magnitude E2M1[c & 7] (code 8 is -0);  scale byte s: the fp16 with exponent field
  f = clamp(s - 112, 0, 30), i.e. +0 for s <= 112, 2^15 for s >= 142, else 2^(s - 127);  w[k, n] = fp16(value * scale), one multiply;
  y = fp16(sum_k f32(x) f32(w)), fp32 accumulation;
  router: logit = (fp32 dot) + bias[e], then oracle.moe_gate's top-k / softmax;
  w1w3 epilogue: g = h(acc[2j]), u = h(acc[2j+1]); g = h(g + bg), u = h(u + bu); g = min(g, 7), u = clamp(u, -7, 7);
      act = h(g / (1 + expf(-1.702 g)) * (1 + u)) in fp32;
  combine: out[t] = h(sum_j w[t][j] * f32(h(y[pair j of t] + b2[expert])))), the fp32 chain in the order j = 0 .. k-1.

Layouts are the checkpoint's: blocks uint8 [N][K/2] (low nibble = even k), scales uint8 [N][K/32]; w1w3's N rows are
(gate_j, up_j)-interleaved.  `mut` arguments restate the faults this path can have (tests/test_host_mxfp4.py proves each one changes
an output bit).

exact_block() builds blocks with ONE correct bit pattern per output whatever the row tile or the order of summation, in the style of
tests/moe_exact_reference.py: integer x, integer router logits and biases whose picks tie at the top (weights exactly 1 / k, and the
bias decides the picks), e2m1 x 2^e weights under a two-exponent scale spread, biases on the lattices, gate pre-activations in
(7, 256] (clamped to exactly 7: 7 / (1 + expf(-11.914)) * (1 + u) rounds to the fp16 7 (1 + u) for every 1 + u of at most 8
significant bits, whatever the last bit of expf) or exactly 0 (act = +-0), up pre-activations multiples of 1/16, some past +-7.  The
builder asserts every budget: sum |terms| / lattice <= 2^24 for both GEMMs, representable pre-activations, an exact combine."""
import math
import types
from dataclasses import dataclass

import numpy as np

from oracle import tm_oracle as o

f16, f32, f64 = np.float16, np.float32, np.float64
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], f32)
SCALE_BYTES = (0, 112, 113, 127, 141, 142, 143, 255)      # flush, flush edge, smallest normal, one, 2^14, the clamp, past it
ALPHA, LIMIT = f32(1.702), f32(7.0)
MUTATIONS = ('nibbles', 'scale_group', 'gate_up', 'neighbour_bias', 'no_clamp', 'no_alpha', 'no_one_plus_up', 'no_router_bias')


def to_f16(v64):
    """one rounding of exact float64 values to fp16"""
    with np.errstate(over='ignore'):
        return np.asarray(v64, f64).astype(f16)


def hadd(a, b):
    """fp16 add, one rounding (the float64 sum of two fp16 values is exact)"""
    return to_f16(np.asarray(a, f16).astype(f64) + np.asarray(b, f16).astype(f64))


def e2m1_value(codes):
    """codes 0..15 -> fp16 values (code 8: -0)"""
    c = np.asarray(codes, np.uint8)
    v = E2M1[c & 7].astype(f16)
    return np.where(c >> 3 == 1, -v, v).astype(f16)


def scale_f16(s):
    """ue8m0 byte -> the fp16 scale (AdjustUe8m0ScaleForHalf): exponent field clamp(s - 112, 0, 30)"""
    f = np.clip(np.asarray(s, np.int32) - 112, 0, 30).astype(np.uint16)
    return (f << 10).astype(np.uint16).view(f16)


def unpack_codes(blocks):
    """blocks uint8 [N][K/2] -> codes uint8 [N][K]: low nibble = even k"""
    b = np.asarray(blocks, np.uint8)
    c = np.empty((b.shape[0], b.shape[1] * 2), np.uint8)
    c[:, 0::2], c[:, 1::2] = b & 15, b >> 4
    return c


def pack_codes(codes):
    c = np.asarray(codes, np.uint8)
    return np.ascontiguousarray(c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def dequant(blocks, scales, mut=None):
    """-> w fp16 [K][N].  mut 'nibbles': high nibble = even k; 'scale_group': group g reads the scale of group g + 1 (cyclic)"""
    c = unpack_codes(blocks)
    if mut == 'nibbles':
        c = c.reshape(c.shape[0], -1, 2)[:, :, ::-1].reshape(c.shape)
    s = np.asarray(scales, np.uint8)
    if mut == 'scale_group':
        s = np.roll(s, -1, axis=1)
    with np.errstate(over='ignore'):
        w = e2m1_value(c) * np.repeat(scale_f16(s), 32, axis=1)      # fp16 x fp16: the float32 product is exact, one rounding
    return np.ascontiguousarray(w.astype(f16).T)


def gptoss_act(gu, bias=None, mut=None):
    """gu fp16 [R][2I] (the w1w3 GEMM's output), bias fp16 [2I] or None -> act fp16 [R][I]"""
    gu = np.asarray(gu, f16)
    if bias is not None:
        gu = hadd(gu, np.asarray(bias, f16)[None, :])
    g, u = gu[:, 0::2].astype(f32), gu[:, 1::2].astype(f32)
    if mut == 'gate_up':
        g, u = u, g
    if mut != 'no_clamp':
        g = np.minimum(g, LIMIT)
        u = np.maximum(-LIMIT, np.minimum(u, LIMIT))
    a = f32(1.0) if mut == 'no_alpha' else ALPHA
    with np.errstate(over='ignore', invalid='ignore'):
        s = g / (f32(1.0) + np.exp(-a * g, dtype=f32))
        out = s if mut == 'no_one_plus_up' else s * (f32(1.0) + u)
        return out.astype(f32).astype(f16)


def router(x, gate, bias, top_k, norm_topk=True, routed_scale=1.0, mut=None):
    """oracle.moe_gate with the bias (fp32 [E] or None) added to the fp32 logits before the top-k"""
    logits = (np.asarray(x, f16).astype(f32) @ np.asarray(gate, f16).astype(f32)).astype(f32)
    if bias is not None and mut != 'no_router_bias':
        logits = (logits + np.asarray(bias, f32)[None, :]).astype(f32)
    T, E = logits.shape
    ids, w = np.zeros((T, top_k), np.int32), np.zeros((T, top_k), f32)
    for t in range(T):
        order = np.lexsort((np.arange(E), -logits[t]))[:top_k]
        ex = np.exp((logits[t] - logits[t].max()).astype(f32)).astype(f32)
        denom = ex[order].sum(dtype=f32) if norm_topk else ex.sum(dtype=f32)
        ids[t], w[t] = order, ex[order] / denom * f32(routed_scale)
    return logits, ids, w


def block_forward(x, gate, gate_bias, experts, top_k, norm_topk=True, routed_scale=1.0, act=1, mut=None, exact=False):
    """The whole block.  experts[e] = dict(w13 fp16 [H][2I], w2 fp16 [I][H], b13 fp16 [2I] or None, b2 fp16 [H] or None) on
    DEQUANTISED weights.  act 1: the gpt-oss activation, 0: oracle.gated_silu_epilogue (no biases).  exact: the GEMMs in float64 (for
    operands whose sums are exact; else float32 matmul).  -> out fp16 [T][H], ids, w"""
    x = np.asarray(x, f16)
    _, ids, w = router(x, gate, gate_bias, top_k, norm_topk, routed_scale, mut)
    T, H = x.shape
    E = len(experts)
    acc_t = f64 if exact else f32
    y = np.zeros((T, top_k, H), f16)
    for e in np.unique(ids):
        t, j = np.nonzero(ids == e)
        ex = experts[int(e)]
        bsrc = experts[(int(e) + 1) % E] if mut == 'neighbour_bias' else ex
        acc = x[t].astype(acc_t) @ ex['w13'].astype(acc_t)
        if act == 1:
            a = gptoss_act(to_f16(acc), bsrc['b13'], mut)
        else:
            a = o.gated_silu_epilogue(acc.astype(f32))
        y2 = to_f16(a.astype(acc_t) @ ex['w2'].astype(acc_t))
        if bsrc['b2'] is not None:
            y2 = hadd(y2, bsrc['b2'][None, :])
        y[t, j] = y2
    out = np.zeros((T, H), f32)
    with np.errstate(over='ignore', invalid='ignore'):
        for j in range(top_k):      # fma(w, y, acc): the product is rounded once with the sum (float64 holds it exactly)
            out = (out.astype(f64) + w[:, j:j + 1].astype(f64) * y[:, j].astype(f64)).astype(f32)
        return out.astype(f16), ids, w


# ---- random MXFP4 experts -------------------------------------------------------------------------------------------------------
def random_linear(rng, K, N, scale_byte=121):
    """uniform codes, scale bytes in {b - 1, b, b + 1} -> dict(blocks [N][K/2], scales [N][K/32])"""
    return dict(blocks=rng.integers(0, 256, (N, K // 2), dtype=np.uint8),
                scales=(scale_byte + rng.integers(-1, 2, (N, K // 32))).astype(np.uint8))


def random_expert(rng, H, I, bias=True, scale_byte=121):
    a, b = random_linear(rng, H, 2 * I, scale_byte), random_linear(rng, I, H, scale_byte)
    return dict(w1w3=a, w2=b, w13=dequant(**a), w2d=dequant(**b),
                b13=(0.25 * rng.standard_normal(2 * I)).astype(f16) if bias else None,
                b2=(0.1 * rng.standard_normal(H)).astype(f16) if bias else None)


def dense(ex):
    """an expert of random_expert / exact_block in block_forward's form"""
    return dict(w13=ex['w13'], w2=ex['w2d'], b13=ex['b13'], b2=ex['b2'])


# ---- exactly summable blocks ----------------------------------------------------------------------------------------------------
TOP = 4                 # the picks' logit
BUDGET = 2.0**24
E13, E2 = -3, -4        # lowest scale exponents of the up columns of w1w3 / of w2
GATE_E = 2              # the gate columns' scale exponent on the bias row's group
LU = 2.0**(E13 - 1)     # lattice of the up pre-activations: 1/16
LA = LU                 # act = 7 n / 16
L2 = LA * 2.0**(E2 - 1)
FLUSH_BYTE = 100


def _exact_expert(H, I, e):
    rng = np.random.default_rng([41, H, I, e])
    row = H - 2                                                  # the bias channel of x
    G13, G2 = H // 32, I // 32
    c13 = rng.integers(0, 16, (2 * I, H)).astype(np.uint8)
    s13 = (127 + E13 + (np.arange(G13)[None, :] + np.arange(2 * I)[:, None]) % 2).astype(np.uint8)
    # gate rows (even): zero codes (+0 and -0) off the bias channel, there 2, 3, 4 or 6 under 2^GATE_E: accumulators x_b * {8 .. 24};
    # every fifth gate row is zero throughout (act = +-0).  Groups without the bias channel: a flushing scale byte on odd gates
    gates = np.arange(0, 2 * I, 2)
    c13[gates] = np.where(rng.integers(0, 2, (I, H)) == 1, 8, 0).astype(np.uint8)
    live = (np.arange(I) % 5) != 4
    c13[gates[live], row] = (4 + (np.arange(I)[live] + e) % 4).astype(np.uint8)
    s13[gates] = 127 + GATE_E
    s13[gates[1::2], :row // 32] = FLUSH_BYTE
    c2 = rng.integers(0, 16, (H, I)).astype(np.uint8)
    s2 = (127 + E2 + (np.arange(G2)[None, :] + np.arange(H)[:, None]) % 2).astype(np.uint8)
    a, b = dict(blocks=pack_codes(c13), scales=s13), dict(blocks=pack_codes(c2), scales=s2)
    b13 = np.zeros(2 * I, f64)
    b13[0::2] = np.where(live, rng.integers(0, 3, I), 0)         # gate biases: integers >= 0 (g stays > 7), 0 on the zero gates
    b13[1::2] = rng.integers(-24, 25, I) * LU
    return dict(w1w3=a, w2=b, w13=dequant(**a), w2d=dequant(**b), b13=b13.astype(f16), b2=(rng.integers(-64, 65, H) * L2 * 8).astype(f16),
                live=live)


def exact_block(H, I, E, k, T, seed=0):
    """-> namespace(x fp16 [T][H], gate, gate_bias, experts, ids, out fp16 [T][H], act / y per pair for diagnosis)"""
    assert E + 2 <= H and math.log2(k) == int(math.log2(k))
    rng = np.random.default_rng([seed, H, I, E, k, T])
    experts = [_exact_expert(H, I, e) for e in range(E)]
    gate = np.zeros((H, E), f16)
    gate[:E] = np.eye(E, dtype=f16)
    gate_bias = (np.arange(E) % 3).astype(f32)
    x = rng.integers(-1, 2, (T, H)).astype(np.int64)
    picks = np.sort(np.stack([rng.permutation(E)[:k] for _ in range(T)]), axis=1).astype(np.int32)
    for t in range(T):                                           # final logit = x + bias: TOP on the picks, strictly less elsewhere
        x[t, :E] = [rng.integers(-3, TOP - int(gate_bias[e_])) for e_ in range(E)]
        x[t, picks[t]] = TOP - gate_bias[picks[t]].astype(np.int64)
    x[:, H - 2] = rng.integers(1, 3, T)
    xh = x.astype(f16)
    lg, ids, w = router(xh, gate, gate_bias, k)
    assert np.array_equal(lg, (x[:, :E] + gate_bias[None, :]).astype(f32)) and np.array_equal(ids, picks)
    assert np.array_equal(w.view(np.uint32), np.full((T, k), 1.0 / k, f32).view(np.uint32)), 'weights are not exactly 1 / k'
    _, ids_nb, _ = router(xh, gate, gate_bias, k, mut='no_router_bias')
    assert T < 3 or not np.array_equal(ids_nb, ids), 'the router bias does not change a pick'
    worst = [0.0, 0.0]
    for e in np.unique(ids):
        ex = experts[int(e)]
        xe = xh[np.nonzero(ids == e)[0]].astype(f64)
        w13, w2 = ex['w13'].astype(f64), ex['w2d'].astype(f64)
        assert np.isfinite(w13).all() and np.isfinite(w2).all()
        acc = xe @ w13
        worst[0] = max(worst[0], float((np.abs(xe) @ np.abs(w13)).max() / LU))
        gu = acc + ex['b13'].astype(f64)[None, :]
        n = gu / LU
        assert np.array_equal(n, np.round(n)) and np.abs(acc / LU).max() < 2048 and np.abs(n).max() < 2048, 'pre-activation not in fp16'
        g, u = gu[:, 0::2], gu[:, 1::2]
        assert ((g[:, ex['live']] > 7) & (g[:, ex['live']] <= 256)).all() and not g[:, ~ex['live']].any()
        act = gptoss_act(to_f16(acc), ex['b13'])
        want = np.where(ex['live'][None, :], 7.0 * (1.0 + np.clip(u, -7, 7)), 0.0)
        assert np.array_equal(act.astype(f64), want), 'the activation is not pinned'
        assert (np.abs(u) > 7).any() and (np.abs(u) < 7).any()
        worst[1] = max(worst[1], float((np.abs(act.astype(f64)) @ np.abs(w2)).max() / L2))
    assert max(worst) <= BUDGET, f'not exactly summable: {worst}'
    out, ids2, _ = block_forward(xh, gate, gate_bias, [dense(ex) for ex in experts], k, exact=True)
    assert np.array_equal(ids2, ids) and np.isfinite(out.astype(f32)).all() and np.abs(out.astype(f32)).max() > 0
    return types.SimpleNamespace(x=xh, gate=gate, gate_bias=gate_bias, experts=experts, ids=ids, w=w, out=out, worst=worst)


def bits(a):
    """uint16 view with -0 mapped to +0"""
    v = np.ascontiguousarray(np.asarray(a, f16)).view(np.uint16).copy()
    v[v == 0x8000] = 0
    return v


# ---- a 2-layer model: fp16 attention, MXFP4 experts with biases and the gpt-oss activation ------------------------------------------
@dataclass
class GptOssMoeConfig(o.ModelConfig):
    moe_expert_format: int = 3
    moe_act: int = 1
    moe_bias: int = 1


GPTOSS_MOE_CFG = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=128, vocab=1024, rms_eps=1e-5,
                      rope=o.RopeParam(128, 10000.0), moe_experts=8, moe_top_k=2, moe_norm_topk=True, kv_bits=8)


def make_gptoss_weights(cfg, seed=0):
    """oracle.make_synthetic_weights' fp16 attention / norms / embeddings; every layer's experts redrawn as MXFP4 with biases, plus a
    router bias"""
    w = o.make_synthetic_weights(cfg, seed=seed, quantized=False)
    rng = np.random.default_rng([seed, 4])
    for L in w['layers']:
        ex = [random_expert(rng, cfg.hidden, cfg.inter, scale_byte=119) for _ in range(cfg.moe_experts)]
        L['experts'] = [dict(w1w3=e['w1w3'], w2=e['w2'], w1w3_bias=e['b13'], w2_bias=e['b2'], _dense=dense(e)) for e in ex]
        L['moe_gate_bias'] = (0.5 * rng.standard_normal(cfg.moe_experts)).astype(f32)
    return w


class GptOssMoeOracleModel(o.OracleModel):
    """oracle.OracleModel.forward with the FFN line replaced by block_forward"""

    def forward(self, ids_per_seq, decode_splits=1):
        cfg = self.cfg
        D, Hq, Hkv = cfg.head_dim, cfg.q_heads, cfg.kv_heads
        lens = [len(t) for t in ids_per_seq]
        ids = np.concatenate([np.asarray(t, np.int64) for t in ids_per_seq])
        offs = np.concatenate([[0], np.cumsum(lens)])
        resid = o.embedding_lookup(self.w['tok_embeddings'], ids)
        x = o.rmsnorm(resid, self.w['layers'][0]['attn_norm'], cfg.rms_eps)
        for li, Lw in enumerate(self.w['layers']):
            qkv = o._linear(x, Lw['w_qkv'], cfg.group)
            attn = np.zeros((len(ids), Hq * D), f16)
            for b, n in enumerate(lens):
                if n == 0:
                    continue
                sl = slice(offs[b], offs[b + 1])
                hist = self.seq_len[b]
                cos, sin = o.rope_cos_sin(cfg.rope, np.arange(hist, hist + n))
                q = o.rope_apply(qkv[sl, :Hq * D].reshape(n, Hq, D), cos, sin)
                k = qkv[sl, Hq * D:(Hq + Hkv) * D].reshape(n, Hkv, D)
                v = qkv[sl, (Hq + Hkv) * D:].reshape(n, Hkv, D)
                o.process_kv(self.cache, self.tables[b], li, k, v, cos, sin, hist)
                if n == 1:
                    kv = [self.cache.load_dequant(self.tables[b], li, hd, 0, hist + 1, 'decode') for hd in range(Hkv)]
                    attn[sl] = o.decode_attention(q[0], np.stack([a for a, _ in kv]), np.stack([c for _, c in kv]), self.c,
                                                  decode_splits).reshape(1, -1)
                else:
                    Kf, Vf = o.flatten_kv(self.cache, self.tables[b], li, hist + n)
                    attn[sl] = o.prefill_attention(q, Kf, Vf, hist, self.c).reshape(n, -1)
            resid, x = o.residual_rmsnorm(resid, o._linear(attn, Lw['wo'], cfg.group), Lw['ffn_norm'], cfg.rms_eps)
            d, _, _ = block_forward(x, Lw['moe_gate'], Lw['moe_gate_bias'], [E_['_dense'] for E_ in Lw['experts']], cfg.moe_top_k,
                                    cfg.moe_norm_topk, cfg.moe_routed_scale)
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        logits = o.lm_head(x[last], self.w['output'])
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits
