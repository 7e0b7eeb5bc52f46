"""Numpy restatement of the MXFP4 W4A4 dense linear (FP4 weights, FP4 activations quantised per group of 32), shared by
tests/test_host_mxfp4_dense.py and tests/test_gpu_mxfp4_dense.py.

Contract:
  e2m1         code c & 7 -> {0, 0.5, 1, 1.5, 2, 3, 4, 6}, bit 3 = sign; e8m0 scale byte b = 2^(b - 127), 255 never produced or accepted
  weights      blocks uint8 [N][K/2] (byte j of row n: k = 2j in the low nibble, 2j + 1 in the high nibble), scales uint8 [N][K/32]
  activations  per row and group of 32, finite fp16 input: amax = max |x|, e = floor(log2(amax)) - 2 (-127 when amax == 0),
               scale byte e + 127, code = e2m1_rne_sat(x / 2^e): round to nearest, ties to the even mantissa, magnitudes above 6
               saturate to 6, the sign of zero is kept (the OCP MX v1.0 rule)
  linear       y[m, n] = h( sum_g 2^(sx[m,g] - 127) 2^(sw[n,g] - 127) sum_{k in g} xq[m,k] wq[n,k] ), the sum over K in fp32;
               gated: the gated-SiLU epilogue on the fp32 values of the (gate_j, up_j)-interleaved columns.

Mutations (`mut`) that tests/test_host_mxfp4_dense.py requires to change the answers: 'scale_rule' (e off by one), 'ties_away'
(ties away from zero instead of to the even mantissa), 'nibbles' (high nibble first), 'scale_group' (a group's scale taken from its
neighbour).

Exact operands (exact_weight / exact_x): x elements are e2m1 values up to |4| times 2^a(m, g) with one pivot of +-4 or +-6 per group, so
that amax = pivot, e = a and the codes are the elements themselves; weight codes lie within +-2 with scales 2^c(n, g);
a(m, g) = (3m + 5g) mod 5 - 2 and c(n, g) = (7n + 3g) mod 4 - 2: the product of the two scales differs for neighbouring rows, columns and
groups (5g drops out of a mod 5: the rows' exponents change with m, the change from group to group comes from c), with periods coprime
to every tile dimension.  Every product is a multiple of the column's quantum 2^(min a + min c - 2) and the sum of their magnitudes stays
below 2^23 quanta (asserted), so every order of accumulation, every split of K and every k-phase gives the same fp32 value.  Gated form:
x and the gate columns are non-negative, a = |a(m, g)|, the gate columns have c in {0, 1} and code 2.0 against every group's pivot (one
position per group for all rows), so the gate accumulator is >= 32 (4 groups x 4 x 2), where g / (1 + expf(-g)) is g itself in fp32;
the up columns' exponents are lowered by 8 to keep g * u finite in fp16.
"""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import tm_oracle as o

f16, f32 = np.float16, np.float32
LUT = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
GROUP = 32
MUTATIONS = ('scale_rule', 'ties_away', 'nibbles', 'scale_group')


# ---- arithmetic ---------------------------------------------------------------------------------------------------------
def e2m1_value(codes):
    c = np.asarray(codes).astype(np.int64)
    return np.where(c & 8, -1.0, 1.0) * LUT[c & 7]


def e2m1_rne_sat(v, mut=None):
    """float64 -> 4-bit codes; the midpoints between neighbouring values go to the code with the even mantissa bit (= even code)"""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    if mut == 'ties_away':
        c = (a >= 0.25).astype(np.int64) + (a >= 0.75) + (a >= 1.25) + (a >= 1.75) + (a >= 2.5) + (a >= 3.5) + (a >= 5)
    else:
        c = (a > 0.25).astype(np.int64) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5)
    return (c | (np.signbit(v).astype(np.int64) << 3)).astype(np.uint8)


def pack_codes(codes, mut=None):
    """codes uint8 [..., K] -> bytes [..., K/2], k = 2j in the low nibble"""
    c = np.asarray(codes, np.uint8)
    lo, hi = (c[..., 1::2], c[..., 0::2]) if mut == 'nibbles' else (c[..., 0::2], c[..., 1::2])
    return (lo | (hi << 4)).astype(np.uint8)


def unpack_codes(blocks, mut=None):
    b = np.asarray(blocks, np.uint8)
    out = np.empty(b.shape[:-1] + (b.shape[-1] * 2,), np.uint8)
    lo, hi = b & 15, b >> 4
    out[..., 0::2], out[..., 1::2] = (hi, lo) if mut == 'nibbles' else (lo, hi)
    return out


def quant(x, mut=None):
    """fp16 [M][K] -> (blocks uint8 [M][K/2], scale bytes uint8 [M][K/32])"""
    x = np.asarray(x, f16)
    assert np.isfinite(x.astype(f32)).all() and x.shape[1] % GROUP == 0
    M, K = x.shape
    xg = x.astype(np.float64).reshape(M, K // GROUP, GROUP)
    amax = np.abs(xg).max(axis=-1)
    with np.errstate(divide='ignore'):
        e = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - 2, -127.0)
    if mut == 'scale_rule':
        e = np.where(amax > 0, e + 1, e)
    codes = e2m1_rne_sat(xg / np.exp2(e)[..., None], mut)
    return pack_codes(codes.reshape(M, K), mut), (e + 127).astype(np.uint8)


def scale_value(sb, mut=None):
    sb = np.asarray(sb)
    assert not (sb == 255).any(), 'scale byte 255 (NaN) is never produced or accepted'
    if mut == 'scale_group':
        sb = np.roll(sb, 1, axis=-1)
    return np.exp2(sb.astype(np.float64) - 127)


def dequant(blocks, scales, mut=None):
    """float64 [rows][K] = lut[code] * 2^(s - 127) (exact: 3 significant bits times a power of two)"""
    v = e2m1_value(unpack_codes(blocks, mut))
    return v * np.repeat(scale_value(scales, mut), GROUP, axis=-1)


def acc_f64(x, blocks, scales, mut=None):
    """(float64 sum over K of the dequantised codes' products, sum of their magnitudes)"""
    xb, xs = quant(x, mut)
    a, w = dequant(xb, xs, mut), dequant(blocks, scales, mut)
    return a @ w.T, np.abs(a) @ np.abs(w).T


def linear(x, blocks, scales, gated=False, mut=None):
    acc = acc_f64(x, blocks, scales, mut)[0].astype(f32)
    return o.gated_silu_epilogue(acc) if gated else acc.astype(f16)


def quantize_weight(w_out_in):
    """a [out][in] weight -> (blocks, scale bytes) by the activation rule (what a Quark MXFP4 export holds, up to its scale rounding)"""
    w16 = np.asarray(w_out_in, f32).astype(f16)
    return quant(w16)


# ---- exactly summable operands -------------------------------------------------------------------------------------------
def row_exp(M, G, gated=False):
    a = (3 * np.arange(M)[:, None] + 5 * np.arange(G)[None, :]) % 5 - 2
    return np.abs(a) if gated else a


def col_exp(N, G, gated=False):
    n, g = np.arange(N)[:, None], np.arange(G)[None, :]
    c = (7 * n + 3 * g) % 4 - 2
    if gated:
        c = np.where(n % 2 == 0, (n // 2 + g) % 2, c - 8)
    return c


def pivot_pos(g):
    return (3 * g + 1) % GROUP


def exact_weight(K, N, gated=False, seed=0):
    """(blocks [N][K/2], scale bytes [N][K/32]): codes within +-2"""
    rng = np.random.default_rng(1000 + K * 7 + N + seed)
    G = K // GROUP
    mag = rng.integers(0, 5, (N, K))
    sign = rng.integers(0, 2, (N, K))
    if gated:
        sign[0::2] = 0
        for g in range(G):
            mag[0::2, g * GROUP + pivot_pos(g)] = 4
    sign[mag == 0] = 0
    codes = (mag | (sign << 3)).astype(np.uint8)
    return pack_codes(codes), (col_exp(N, G, gated) + 127).astype(np.uint8)


def exact_x(M, K, gated=False, seed=0):
    """fp16 [M][K] as the module docstring describes; not gated: the pivot's place depends on (m, g), sign and size (4 or 6) alternate"""
    rng = np.random.default_rng(2000 + M * 13 + K + seed)
    G = K // GROUP
    v = LUT[rng.integers(0, 7, (M, K))]
    if not gated:
        v = v * rng.choice([-1.0, 1.0], (M, K))
    v = v.reshape(M, G, GROUP)
    m, g = np.meshgrid(np.arange(M), np.arange(G), indexing='ij')
    pos = np.broadcast_to(pivot_pos(np.arange(G))[None, :], (M, G)) if gated else (5 * m + 3 * g) % GROUP
    piv = np.where((m + g) % 2 == 0, 4.0, 6.0) * (1.0 if gated else np.where((m // 2 + g) % 2 == 0, 1.0, -1.0))
    v[m, g, pos] = piv
    x = (v * np.exp2(row_exp(M, G, gated))[:, :, None]).reshape(M, K)
    x16 = x.astype(f16)
    assert np.array_equal(x16.astype(np.float64), x)
    return x16


def assert_exactly_summable(x16, blocks, scales, gated=False):
    """the activation codes and scale bytes come back exactly; per column every product is a multiple of the quantum and the sum of the
    magnitudes is below 2^23 quanta; the float64 sum does not depend on the order; outputs fit fp16.  Returns the expected fp16 output."""
    M, K = x16.shape
    G = K // GROUP
    xb, xs = quant(x16)
    assert np.array_equal(xs.astype(np.int64) - 127, row_exp(M, G, gated)), 'the activation scale bytes are not the exponents a(m, g)'
    a, w = dequant(xb, xs), dequant(blocks, scales)
    assert np.array_equal(a, x16.astype(np.float64)), 'the activation codes are not exact'
    assert np.abs(e2m1_value(unpack_codes(blocks))).max() <= 2.0
    quantum = np.exp2(row_exp(M, G, gated).min() + (scales.astype(np.int64) - 127).min(axis=1) - 2)      # [N]
    full, mag = a @ w.T, np.abs(a) @ np.abs(w).T
    assert np.all(mag < 2.0**23 * quantum[None, :])
    assert np.array_equal(np.round(full / quantum) * quantum, full)
    perm = np.random.default_rng(5).permutation(K)
    assert np.array_equal(a[:, perm] @ w[:, perm].T, full) and np.array_equal(a[:, ::-1] @ w[:, ::-1].T, full)
    assert np.array_equal(full.astype(f32).astype(np.float64), full)
    if gated:
        gate = full[:, 0::2].astype(f32)
        assert gate.min() >= 32.0
        assert np.array_equal(o.silu_f32(gate).view(np.uint32), gate.view(np.uint32))
    y = linear(x16, blocks, scales, gated)
    assert np.isfinite(y.astype(f32)).all()
    return y


# ---- toy Quark checkpoints -----------------------------------------------------------------------------------------------------
def quant_config(**over):
    """quantization_config of a Quark MXFP4 W4A4 export (the layout lmdeploy_amd.turbomind.checkpoint.QUARK writes down), with the
    KV-cache entries a reader has to read past"""
    spec = dict(dtype='fp4', qscheme='per_group', group_size=32, scale_format='e8m0', ch_axis=-1, is_dynamic=False)
    kv = dict(dtype='fp8_e4m3', qscheme='per_tensor', is_dynamic=False)
    layer = dict(weight=dict(spec), input_tensors=dict(spec, is_dynamic=True), output_tensors=kv)
    q = dict(quant_method='quark', export=dict(pack_method='reorder', kv_cache_group=['*k_proj', '*v_proj']),
             global_quant_config=dict(weight=dict(spec), input_tensors=dict(spec, is_dynamic=True), output_tensors=None, bias=None),
             layer_quant_config={'*k_proj': layer, '*v_proj': dict(layer)}, layer_type_quant_config={}, exclude=['lm_head'])
    q.update(over)
    return q


def write_checkpoint(path, *, hidden=256, layers=2, q_heads=2, kv_heads=1, head_dim=128, inter=512, vocab=512, seed=0,
                     arch='LlamaForCausalLM', quantization_config=None, extra_config=None):
    """Writes a toy HF checkpoint (config.json + model.safetensors) in the Quark MXFP4 layout: per projection `.weight` uint8
    [out][in / 2] and `.weight_scale` uint8 [out][in / 32], k_proj / v_proj with an `.output_scale` to read past; magnitudes of
    oracle.make_synthetic_weights (embeddings 0.02 N, linears 0.1 / sqrt(K) N times a per-channel factor in [0.5, 2]).  Returns
    {tensor name: numpy array} plus 'config'."""
    import torch
    from safetensors.torch import save_file

    rng = np.random.default_rng(seed)
    os.makedirs(path, exist_ok=True)
    cfg = {'architectures': [arch], 'model_type': 'llama', 'hidden_size': hidden, 'num_hidden_layers': layers,
           'num_attention_heads': q_heads, 'num_key_value_heads': kv_heads, 'head_dim': head_dim, 'intermediate_size': inter,
           'vocab_size': vocab, 'rms_norm_eps': 1e-5, 'rope_theta': 10000.0, 'max_position_embeddings': 512, 'tie_word_embeddings': False,
           'torch_dtype': 'float16', 'quantization_config': quantization_config or quant_config()}
    cfg.update(extra_config or {})
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(cfg, f)
    tensors = {}

    def dense(name, shape, std):
        tensors[name] = (rng.standard_normal(shape) * std).astype(f16)

    def qlinear(prefix, out_f, in_f):
        w = rng.standard_normal((out_f, in_f)) * (0.1 / np.sqrt(in_f)) * rng.uniform(0.5, 2.0, (out_f, 1))
        tensors[prefix + '.weight'], tensors[prefix + '.weight_scale'] = quantize_weight(w)

    dense('model.embed_tokens.weight', (vocab, hidden), 0.02)
    dense('lm_head.weight', (vocab, hidden), 0.1 / np.sqrt(hidden))
    tensors['model.norm.weight'] = (1 + 0.05 * rng.standard_normal(hidden)).astype(f16)
    for i in range(layers):
        p = f'model.layers.{i}.'
        tensors[p + 'input_layernorm.weight'] = (1 + 0.05 * rng.standard_normal(hidden)).astype(f16)
        tensors[p + 'post_attention_layernorm.weight'] = (1 + 0.05 * rng.standard_normal(hidden)).astype(f16)
        qlinear(p + 'self_attn.q_proj', q_heads * head_dim, hidden)
        qlinear(p + 'self_attn.k_proj', kv_heads * head_dim, hidden)
        qlinear(p + 'self_attn.v_proj', kv_heads * head_dim, hidden)
        qlinear(p + 'self_attn.o_proj', hidden, q_heads * head_dim)
        tensors[p + 'self_attn.k_proj.output_scale'] = np.asarray(0.02, f32)     # read past
        tensors[p + 'self_attn.v_proj.output_scale'] = np.asarray(0.03, f32)
        qlinear(p + 'mlp.gate_proj', inter, hidden)
        qlinear(p + 'mlp.up_proj', inter, hidden)
        qlinear(p + 'mlp.down_proj', hidden, inter)
    save_file({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}, os.path.join(path, 'model.safetensors'))
    out = dict(tensors)
    out['config'] = cfg
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------
def tm_weights(ck: dict, oc: o.ModelConfig) -> dict:
    """the engine-layout weights of a checkpoint written by write_checkpoint, assembled here (not by checkpoint.py): linears
    {'blocks' [N][K/2], 'scales' [N][K/32]} output-major, q / k rows permuted for the interleaved RoPE, q | k | v stacked,
    (gate_j, up_j) rows interleaved"""
    D, Hq, Hkv = oc.head_dim, oc.q_heads, oc.kv_heads

    def lin(pre, heads=None):
        d = dict(blocks=ck[pre + '.weight'], scales=ck[pre + '.weight_scale'])
        if heads:
            d = {k: np.ascontiguousarray(o.permute_qk_for_interleaved_rope(v.T, heads, D).T) for k, v in d.items()}
        return d

    def fuse(g, u):
        return {k: np.ascontiguousarray(o.interleave_w1w3(g[k].T, u[k].T).T) for k in g}

    layers = []
    for i in range(oc.layers):
        p = f'model.layers.{i}'
        a = p + '.self_attn.'
        q, k, v = lin(a + 'q_proj', Hq), lin(a + 'k_proj', Hkv), lin(a + 'v_proj')
        layers.append(dict(attn_norm=ck[p + '.input_layernorm.weight'], ffn_norm=ck[p + '.post_attention_layernorm.weight'],
                           w_qkv={kk: np.concatenate([q[kk], k[kk], v[kk]], 0) for kk in q}, wo=lin(a + 'o_proj'),
                           w1w3=fuse(lin(p + '.mlp.gate_proj'), lin(p + '.mlp.up_proj')), w2=lin(p + '.mlp.down_proj')))
    return dict(tok_embeddings=ck['model.embed_tokens.weight'], layers=layers, norm=ck['model.norm.weight'],
                output=np.ascontiguousarray(ck['lm_head.weight'].T))


def oracle_config(ck: dict, kv_bits: int) -> o.ModelConfig:
    c = ck['config']
    return o.ModelConfig(hidden=c['hidden_size'], layers=c['num_hidden_layers'], q_heads=c['num_attention_heads'],
                         kv_heads=c['num_key_value_heads'], head_dim=c['head_dim'], inter=c['intermediate_size'], vocab=c['vocab_size'],
                         rms_eps=c['rms_norm_eps'], rope=o.RopeParam(c['head_dim'], c['rope_theta'], 'default', 1.0, 1.0, 4.0, 8192),
                         kv_bits=kv_bits, weight_format='mxfp4')


def perturb_ulp(x, rng):
    """every non-zero element one fp16 ulp up or down, random signs: what the norm / SiLU operator tests allow their outputs"""
    b = np.ascontiguousarray(x, f16).view(np.int16).astype(np.int32)
    step = rng.choice([-1, 1], b.shape)
    nb = np.where((b & 0x7FFF) == 0, b, b + step)
    nb = np.where((nb & 0x7FFF) >= 0x7C00, b, nb)               # never into inf / NaN
    return nb.astype(np.int16).view(f16)


def perturb_attention(x, rng):
    """the decode-attention test's bound (tests/test_gpu_ops.py): +-(1e-2 |x| + 2e-3), random signs"""
    x32 = np.asarray(x, f16).astype(f32)
    return (x32 + rng.choice([-1.0, 1.0], x32.shape).astype(f32) * (f32(1e-2) * np.abs(x32) + f32(2e-3))).astype(f16)


class Mxfp4Model(o.OracleModel):
    """o.OracleModel with the four decoder linears MXFP4 W4A4: linear() above, activations quantised per row and group of 32 once per
    GEMM input.  perturb_seed: every GEMM input is perturbed by what the operator tests allow its producer (perturb_ulp for the norm and
    gated-SiLU outputs, perturb_attention for the attention outputs) -- the measurement of how far FP4's discontinuous activation
    codes carry such noise into the logits."""

    def __init__(self, cfg, weights, batch, max_ctx, perturb_seed=None):
        super().__init__(cfg, weights, batch, max_ctx)
        self.rng = None if perturb_seed is None else np.random.default_rng(perturb_seed)

    def lin(self, x, W, gated=False, kind='ulp'):
        if self.rng is not None:
            x = perturb_attention(x, self.rng) if kind == 'attn' else perturb_ulp(x, self.rng)
        return linear(x, W['blocks'], W['scales'], gated)

    def forward(self, ids_per_seq, decode_splits=1):
        cfg = self.cfg
        D, Hq, Hkv = cfg.head_dim, cfg.q_heads, cfg.kv_heads
        lens = [len(t) for t in ids_per_seq]
        ids = np.concatenate([np.asarray(t, np.int64) for t in ids_per_seq])
        offs = np.concatenate([[0], np.cumsum(lens)])
        resid = o.embedding_lookup(self.w['tok_embeddings'], ids)
        x = o.rmsnorm(resid, self.w['layers'][0]['attn_norm'], cfg.rms_eps)
        for li, Lw in enumerate(self.w['layers']):
            qkv = self.lin(x, Lw['w_qkv'])
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
            resid, x = o.residual_rmsnorm(resid, self.lin(attn, Lw['wo'], kind='attn'), Lw['ffn_norm'], cfg.rms_eps)
            d = self.lin(self.lin(x, Lw['w1w3'], True), Lw['w2'])
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        self.last_resid = resid
        logits = o.lm_head(x[last], self.w['output'])
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits
