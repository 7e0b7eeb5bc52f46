"""Numpy restatement of the channel-scaled FP8 linear (per-tensor and per-channel FP8 checkpoints), shared by
tests/test_host_fp8_channel.py and tests/test_gpu_fp8_channel.py.

Contract:
  weights      e4m3 codes wq [K][N] with one fp32 scale per output column, sw [N]
  activations  quantised per token over the whole row = oracle.tm_oracle.fp8_quant_rows(x, group=K):
               absmax clamped to 1e-8, sx = absmax / 448, q = e4m3_rne_sat(x * (448 / absmax)), fp32 throughout
  linear       y[m, n] = h( (sx[m] * sw[n]) * sum_k xq[m, k] * wq[k, n] ), the sum in fp32 over all of K, the product of the
               two scales formed in fp32 and applied once; gated: the gated-SiLU epilogue on the scaled fp32 values of the
               (gate_j, up_j)-interleaved columns.

Exact operands (exact_weight / exact_x): weight codes are integers in [-2, 2]; an x row is integers in [-4, 4] times 2^a with one element
at +-448 * 2^a, so 448 / absmax = 2^-a, the codes are the integers and sx = 2^a; the column scales are powers of two.  Every
partial sum of products is an integer below 2^24 (asserted), so every order of accumulation, every split of K and every k-phase
gives the same fp32 value, and scaling by powers of two keeps it.  fp16 has 30 binades: scales that are ALL distinct over 96 or
256 columns would push the outputs out of its range (to inf or 0, which compare equal whatever the kernel did), so the exponents
are a_m = (3 m mod 5) - 2 and c_n = (7 n mod 9) - 7: distinct inside every window of 5 rows / 9 columns, periods coprime to every
tile dimension (4, 32, 64, 128 columns; 32, 64 rows), so a scale taken from a wrong row, column, column group or expert shows.
For the gated form the gate columns (even n) carry non-negative codes, a code >= 1 against the +448 element and c_n in {-1, 0}:
the scaled gate accumulator is >= 56, where g / (1 + expf(-g)) is g itself in fp32, and the epilogue is one fp32 product.
"""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import tm_oracle as o

f16, f32 = np.float16, np.float32


# ---- arithmetic ---------------------------------------------------------------------------------------------------------
def quant(x):
    """per-token quantiser: (codes uint8 [M][K], sx fp32 [M])"""
    x = np.asarray(x, f16)
    q, s = o.fp8_quant_rows(x, group=x.shape[1])
    return q, np.ascontiguousarray(s[0])


def acc_f64(xq, wq):
    """sum_k xq * wq in float64 (products of two e4m3 values and their sums up to 2^53 are exact there)"""
    return o.fp8_e4m3_to_f32(xq).astype(np.float64) @ o.fp8_e4m3_to_f32(wq).astype(np.float64)


def linear(x, wq, sw, gated=False, act_quant=True):
    """the contract above; act_quant=False: dequantised weights x fp16 activations with fp32 accumulation (what a framework
    without fp8 matrix cores computes from the same checkpoint -- used for the cross-check against transformers only)"""
    sw = np.asarray(sw, f32)
    if not act_quant:
        w = o.fp8_e4m3_to_f32(wq) * sw[None, :]
        acc = (np.asarray(x, f16).astype(np.float64) @ w.astype(np.float64)).astype(f32)
    else:
        xq, sx = quant(x)
        acc = (sx[:, None] * sw[None, :]).astype(f32) * acc_f64(xq, wq).astype(f32)
    return o.gated_silu_epilogue(acc) if gated else acc.astype(f16)


def grouped(x, experts, seg, row_idx, gated=False):
    """flat rows seg[e] .. seg[e + 1] of expert e = (wq, sw) read row row_idx[f] (None: f) of x"""
    N = experts[0][0].shape[1]
    out = np.zeros((seg[-1], N // 2 if gated else N), f16)
    for e, (wq, sw) in enumerate(experts):
        rows = np.arange(seg[e], seg[e + 1])
        if rows.size:
            out[rows] = linear(x[rows if row_idx is None else row_idx[rows]], wq, sw, gated)
    return out


# ---- exactly summable operands -------------------------------------------------------------------------------------------
def row_exp(m):
    return (3 * np.asarray(m) % 5) - 2


def col_exp(n, gated=False):
    n = np.asarray(n)
    c = (7 * n % 9) - 7
    if gated:                       # gate columns: 2^-1 or 2^0 (see the module docstring); up columns: 2^-14 .. 2^-11, which keeps g * u finite in fp16
        c = np.where(n % 2 == 0, -((n // 2) % 2), -14 + (((n // 2) * 3) % 4))
    return c


def exact_weight(K, N, gated=False, seed=0):
    """(codes uint8 [K][N], sw fp32 [N], pivot column of x that meets a code >= 1 in every gate column)"""
    rng = np.random.default_rng(1000 + K * 7 + N + seed)
    w = rng.integers(-2, 3, (K, N))
    pivot = int(rng.integers(0, K))
    if gated:
        w[:, 0::2] = np.abs(w[:, 0::2])
        w[pivot, 0::2] = 1 + (np.arange(N // 2) % 2)
    sw = np.exp2(col_exp(np.arange(N) + (0 if gated else seed), gated)).astype(f32)
    return o.fp8_e4m3_from_f32(w.astype(f32)), sw, pivot


def exact_x(M, K, pivot, gated=False, seed=0):
    """fp16 [M][K]: integers in [-4, 4] (gated: [0, 4]) times 2^a_m, element `pivot` = +-448 * 2^a_m (gated: +448 * 2^a_m)"""
    rng = np.random.default_rng(2000 + M * 13 + K + seed)
    xi = rng.integers(0 if gated else -4, 5, (M, K)).astype(np.float64)
    xi[:, pivot] = 448.0 if gated else np.where(np.arange(M) % 2 == 0, 448.0, -448.0)
    if not gated:                   # the absmax in the first and in the last column as well
        xi[0::3, pivot] = rng.integers(-4, 5, len(xi[0::3]))
        xi[0::3, 0] = 448.0
        xi[1::3, pivot] = rng.integers(-4, 5, len(xi[1::3]))
        xi[1::3, K - 1] = -448.0
    a = np.abs(row_exp(np.arange(M))) if gated else row_exp(np.arange(M))    # gated: a_m >= 0 keeps the gate >= 56
    x = xi * np.exp2(a)[:, None]
    x16 = x.astype(f16)
    assert np.array_equal(x16.astype(np.float64), x)
    return x16


def assert_exactly_summable(x16, wq, sw, gated=False):
    """every partial sum is an integer below 2^24, the float64 sum does not depend on the order, the codes are the integers"""
    xq, sx = quant(x16)
    a = o.fp8_e4m3_to_f32(xq).astype(np.float64)
    w = o.fp8_e4m3_to_f32(wq).astype(np.float64)
    assert np.array_equal(a * sx[:, None].astype(np.float64), x16.astype(np.float64)), 'the activation codes are not exact'
    assert np.all(np.log2(sx) == np.round(np.log2(sx))) and np.all(np.log2(sw) == np.round(np.log2(sw)))
    assert (np.abs(a) @ np.abs(w)).max() < 2.0**24
    full = a @ w
    perm = np.random.default_rng(5).permutation(a.shape[1])
    assert np.array_equal(a[:, perm] @ w[perm], full) and np.array_equal(a[:, ::-1] @ w[::-1], full)
    if gated:
        g = (sx[:, None] * sw[None, 0::2]).astype(f32) * full[:, 0::2].astype(f32)
        assert g.min() >= 32.0
        assert np.array_equal(o.silu_f32(g).view(np.uint32), g.view(np.uint32))
    y = linear(x16, wq, sw, gated)
    assert np.isfinite(y.astype(f32)).all()
    return y


# ---- toy checkpoints -----------------------------------------------------------------------------------------------------
def quantize_weight(w_out_in, strategy):
    """a checkpoint's [out][in] weight -> (e4m3 codes [out][in] uint8, scale fp32: [] (tensor) or [out, 1] (channel)) with
    scale = absmax / 448 like AutoFP8 / llm-compressor"""
    w = np.asarray(w_out_in, f32)
    if strategy == 'tensor':
        s = np.maximum(np.abs(w).max(), 1e-8).astype(f32) / f32(448.0)
        return o.fp8_e4m3_from_f32(w / s), np.asarray(s, f32)
    s = (np.maximum(np.abs(w).max(axis=1, keepdims=True), 1e-8) / 448.0).astype(f32)
    return o.fp8_e4m3_from_f32(w / s), s


def dequantize_weight(codes, scale):
    return o.fp8_e4m3_to_f32(codes) * np.asarray(scale, f32).reshape(-1, 1) if np.ndim(scale) else o.fp8_e4m3_to_f32(codes) * f32(scale)


def quant_config(dialect, strategy='tensor', static=False, moe=False):
    if dialect == 'fp8':            # AutoFP8 / neuralmagic *-FP8: per-tensor, no weight_block_size
        return {'quant_method': 'fp8', 'activation_scheme': 'static' if static else 'dynamic', 'ignored_layers': ['lm_head']}
    assert dialect == 'compressed-tensors'
    ignore = ['lm_head'] + (['re:.*block_sparse_moe.gate'] if moe else [])
    return {'quant_method': 'compressed-tensors', 'format': 'float-quantized', 'ignore': ignore,
            'kv_cache_scheme': {'num_bits': 8, 'type': 'float', 'strategy': 'tensor', 'dynamic': False, 'symmetric': True} if static else None,
            'config_groups': {'group_0': {
                'targets': ['Linear'],
                'weights': {'num_bits': 8, 'type': 'float', 'symmetric': True, 'strategy': strategy, 'dynamic': False},
                'input_activations': {'num_bits': 8, 'type': 'float', 'symmetric': True, 'strategy': 'tensor' if static else 'token',
                                      'dynamic': not static}}}}


def write_checkpoint(path, *, hidden=256, layers=2, q_heads=2, kv_heads=1, head_dim=128, inter=512, vocab=512, experts=0, top_k=2,
                     dialect='fp8', strategy='tensor', scale_shape=None, static=False, seed=0, arch=None, qkv_bias=False):
    """Writes a toy HF checkpoint (config.json + model.safetensors) with e4m3 decoder linears (magnitudes of
    oracle.make_synthetic_weights, whose models the engine tests' bounds were set on: embeddings 0.02 N, linears 0.1 / sqrt(K) N
    times a per-channel factor in [0.5, 2], router 0.2 N) and returns
    {tensor name: numpy array} of what was written plus 'dequant': {linear prefix: fp32 [out][in]}.
    scale_shape: how a per-tensor scale is stored ('[]' | '[1]') or a per-channel one ('[N]' | '[N,1]')."""
    import torch
    from safetensors.torch import save_file

    rng = np.random.default_rng(seed)
    os.makedirs(path, exist_ok=True)
    moe = experts > 0
    arch = arch or ('MixtralForCausalLM' if moe else 'LlamaForCausalLM')
    cfg = {'architectures': [arch], 'model_type': 'mixtral' if moe else 'llama', 'hidden_size': hidden, 'num_hidden_layers': layers,
           'num_attention_heads': q_heads, 'num_key_value_heads': kv_heads, 'head_dim': head_dim, 'intermediate_size': inter,
           'vocab_size': vocab, 'rms_norm_eps': 1e-5, 'rope_theta': 10000.0, 'max_position_embeddings': 512, 'tie_word_embeddings': False,
           'torch_dtype': 'float16', 'quantization_config': quant_config(dialect, strategy, static, moe)}
    if moe:
        cfg.update(num_local_experts=experts, num_experts_per_tok=top_k)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(cfg, f)
    scale_shape = scale_shape or ('[]' if strategy == 'tensor' else '[N,1]')
    tensors, dequant = {}, {}

    def dense(name, shape, std):
        tensors[name] = (rng.standard_normal(shape) * std).astype(f16)

    def qlinear(prefix, out_f, in_f):
        w = rng.standard_normal((out_f, in_f)) * (0.1 / np.sqrt(in_f)) * rng.uniform(0.5, 2.0, (out_f, 1))
        codes, s = quantize_weight(w, strategy)
        dequant[prefix] = dequantize_weight(codes, s)
        tensors[prefix + '.weight'] = codes
        s = s.reshape({'[]': (), '[1]': (1,), '[N]': (-1,), '[N,1]': (-1, 1)}[scale_shape])
        tensors[prefix + '.weight_scale'] = np.asarray(s, f32)
        if static:                  # read past: calibrated activation / KV scales
            tensors[prefix + '.input_scale'] = np.asarray(0.0123, f32)

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
        if static:
            tensors[p + 'self_attn.k_proj.k_scale'] = np.asarray(0.02, f32)
            tensors[p + 'self_attn.v_proj.v_scale'] = np.asarray(0.03, f32)
        if moe:
            dense(p + 'block_sparse_moe.gate.weight', (experts, hidden), 0.2)
            for e in range(experts):
                qlinear(p + f'block_sparse_moe.experts.{e}.w1', inter, hidden)
                qlinear(p + f'block_sparse_moe.experts.{e}.w3', inter, hidden)
                qlinear(p + f'block_sparse_moe.experts.{e}.w2', hidden, inter)
        else:
            qlinear(p + 'mlp.gate_proj', inter, hidden)
            qlinear(p + 'mlp.up_proj', inter, hidden)
            qlinear(p + 'mlp.down_proj', hidden, inter)

    def to_torch(a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint8:
            return torch.from_numpy(a).view(torch.float8_e4m3fn)
        return torch.from_numpy(a)

    save_file({k: to_torch(v) for k, v in tensors.items()}, os.path.join(path, 'model.safetensors'))
    out = dict(tensors)
    out['dequant'] = dequant
    out['config'] = cfg
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------
def tm_weights(ck: dict, oc: o.ModelConfig) -> dict:
    """the engine-layout weights of a checkpoint written by write_checkpoint, assembled here (not by checkpoint.py): linears
    {'f8': codes [in][out], 'cs': fp32 [out]}, q / k output channels permuted for the interleaved RoPE with their scales, q | k | v
    concatenated, (gate_j, up_j) interleaved"""
    D, Hq, Hkv = oc.head_dim, oc.q_heads, oc.kv_heads
    perm = o.permute_qk_for_interleaved_rope

    def lin(pre, heads=None):
        codes = ck[pre + '.weight']
        cs = np.broadcast_to(np.asarray(ck[pre + '.weight_scale'], f32).reshape(-1), (codes.shape[0],))
        d = dict(f8=np.ascontiguousarray(codes.T), cs=np.ascontiguousarray(cs))
        return {k: perm(v, heads, D) for k, v in d.items()} if heads else d

    def fuse(g, u):
        return dict(f8=o.interleave_w1w3(g['f8'], u['f8']), cs=o.interleave_w1w3(g['cs'][None], u['cs'][None])[0])

    layers = []
    for i in range(oc.layers):
        p = f'model.layers.{i}'
        a = p + '.self_attn.'
        q, k, v = lin(a + 'q_proj', Hq), lin(a + 'k_proj', Hkv), lin(a + 'v_proj')
        L = dict(attn_norm=ck[p + '.input_layernorm.weight'], ffn_norm=ck[p + '.post_attention_layernorm.weight'],
                 w_qkv={kk: np.concatenate([q[kk], k[kk], v[kk]], -1) for kk in q}, wo=lin(a + 'o_proj'))
        if oc.moe_experts:
            m = p + '.block_sparse_moe'
            L['moe_gate'] = np.ascontiguousarray(ck[m + '.gate.weight'].T)
            L['experts'] = [dict(w1w3=fuse(lin(f'{m}.experts.{e}.w1'), lin(f'{m}.experts.{e}.w3')), w2=lin(f'{m}.experts.{e}.w2'))
                            for e in range(oc.moe_experts)]
        else:
            L['w1w3'] = fuse(lin(p + '.mlp.gate_proj'), lin(p + '.mlp.up_proj'))
            L['w2'] = lin(p + '.mlp.down_proj')
        layers.append(L)
    return dict(tok_embeddings=ck['model.embed_tokens.weight'], layers=layers, norm=ck['model.norm.weight'],
                output=np.ascontiguousarray(ck['lm_head.weight'].T))


def oracle_config(ck: dict, kv_bits: int) -> o.ModelConfig:
    c = ck['config']
    return o.ModelConfig(hidden=c['hidden_size'], layers=c['num_hidden_layers'], q_heads=c['num_attention_heads'],
                         kv_heads=c['num_key_value_heads'], head_dim=c['head_dim'], inter=c['intermediate_size'], vocab=c['vocab_size'],
                         rms_eps=c['rms_norm_eps'], rope=o.RopeParam(c['head_dim'], c['rope_theta'], 'default', 1.0, 1.0, 4.0, 8192),
                         kv_bits=kv_bits, weight_format='fp8', moe_experts=c.get('num_local_experts', 0),
                         moe_top_k=c.get('num_experts_per_tok', 0) if c.get('num_local_experts') else 0)


class ChannelModel(o.OracleModel):
    """o.OracleModel with every decoder linear and expert channel-scaled: linear() above, activations quantised per token (x once
    per GEMM input, the gated-SiLU output once per (token, expert) row).  act_quant=False: dequantised weights x fp16 activations."""

    def __init__(self, cfg, weights, batch, max_ctx, act_quant=True):
        super().__init__(cfg, weights, batch, max_ctx)
        self.act_quant = act_quant

    def lin(self, x, W, gated=False):
        return linear(x, W['f8'], W['cs'], gated, self.act_quant)

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
            resid, x = o.residual_rmsnorm(resid, self.lin(attn, Lw['wo']), Lw['ffn_norm'], cfg.rms_eps)
            if cfg.moe_experts:
                _, eids, ew = o.moe_gate(x, Lw['moe_gate'], cfg.moe_top_k, cfg.moe_norm_topk, cfg.moe_routed_scale)
                acc = np.zeros(x.shape, f32)
                for t in range(x.shape[0]):
                    for j in range(cfg.moe_top_k):
                        E_ = Lw['experts'][eids[t, j]]
                        y = self.lin(self.lin(x[t:t + 1], E_['w1w3'], True), E_['w2'])
                        acc[t] += ew[t, j] * y[0].astype(f32)
                d = acc.astype(f16)
            else:
                d = self.lin(self.lin(x, Lw['w1w3'], True), Lw['w2'])
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        self.last_resid = resid
        logits = o.lm_head(x[last], self.w['output'])
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits
