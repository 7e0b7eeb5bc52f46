"""Numpy restatement of the INT8 W8A8 linear (smooth_quant and compressed-tensors int-quantized checkpoints), shared by
tests/test_host_int8.py and tests/test_gpu_int8.py.

Contract:
  weights      int8 codes wq [K][N] with one fp32 scale per output column, sw [N] (a per-tensor scale repeated over its columns; the
               scales of a fused linear concatenated / interleaved like its columns)
  activations  one scale per token over the whole fp16 row, all in fp32:
                 absmax = max(max|x|, 1e-7f);  sx = absmax / 127.0f;  q = x / sx  (the IEEE division, not x * (127 / absmax));
                 round half AWAY from zero;  clamp to [-127, 127]
               |x / sx| reaches 127.00001 (hence the clamp), exact ties occur, and floor(q + 0.5f) in fp32 would round 0.49999997 up:
               quant() rounds in float64, where q + 0.5 is exact.
  linear       y[m, n] = h( (float(acc) * sx[m]) * sw[n] ),  acc = sum_k xq[m, k] * wq[k, n] as an int32 sum over ALL of K (exact:
               K <= 32768 keeps |acc| <= 32768 * 127 * 128 < 2^31), float() = int32 -> fp32 rounding to nearest even, the two scales
               applied in that order; h = the fp16 store, or the gated-SiLU epilogue on the scaled fp32 values of the
               (gate_j, up_j)-interleaved columns.
Integer accumulation is exact, so for every M, every split of K and every k-phase the result is the same bits: the plain linear is
compared bit for bit on RANDOM operands.  The gated epilogue's expf differs between numpy and the device, so the gated form is bit for
bit only where SiLU is the identity in fp32 (exact_weight / exact_x: gate accumulator >= 32 after scaling, 1 + expf(-g) == 1) and
within 2e-3 + 2^-8 |ref| on random operands.

Exact operands for the gated form: weight codes are integers in [-2, 2] (gate columns, even n: non-negative, and >= 1 in row `pivot`);
an x row is integers in [0, 4] times 2^a with element `pivot` = 127 * 2^a, so sx = 2^a exactly and the codes are the integers; gate
column scales are 2^-1 or 2^0: the scaled gate accumulator is >= 127 * 1 * 2^-1 = 63.5.
"""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import tm_oracle as o

f16, f32 = np.float16, np.float32
K_MAX = 32768


# ---- arithmetic ---------------------------------------------------------------------------------------------------------
def quant(x):
    """per-token quantiser: (codes int8 [M][K], sx fp32 [M])"""
    x = np.asarray(x, f16).astype(f32)
    absmax = np.maximum(np.abs(x).max(axis=1), f32(1e-7)).astype(f32)
    sx = (absmax / f32(127.0)).astype(f32)
    q = (x / sx[:, None]).astype(f32)                        # numpy's fp32 division is the IEEE one
    q64 = q.astype(np.float64)
    r = np.copysign(np.floor(np.abs(q64) + 0.5), q64)         # half away from zero; |q| + 0.5 is exact in float64
    return np.clip(r, -127, 127).astype(np.int8), sx


def acc_i64(xq, wq):
    """sum_k xq * wq as int64, checked against the contract's bound (summed in float64, where every partial sum -- an integer below
    2^31 -- is exact in any order; the host test holds it against integer sums)"""
    a = (np.asarray(xq, np.int8).astype(np.float64) @ np.asarray(wq, np.int8).astype(np.float64)).astype(np.int64)
    assert xq.shape[1] <= K_MAX and np.abs(a).max(initial=0) < 2**31
    return a


def scale(acc, sx, sw):
    """(float(acc) * sx[m]) * sw[n] in fp32"""
    a = np.asarray(acc).astype(np.int32).astype(f32)          # int32 -> fp32: round to nearest even
    return ((a * np.asarray(sx, f32)[:, None]).astype(f32) * np.asarray(sw, f32)[None, :]).astype(f32)


def linear(x, wq, sw, gated=False):
    xq, sx = quant(x)
    y = scale(acc_i64(xq, wq), sx, sw)
    return o.gated_silu_epilogue(y) if gated else y.astype(f16)


# ---- operands ---------------------------------------------------------------------------------------------------------------
def random_weight(rng, K, N):
    """codes over the whole of [-128, 127] (the corners planted) and column scales of very different size that keep outputs of
    x ~ N(0, 1) * [0.2, 4] well inside fp16"""
    wq = rng.integers(-128, 128, (K, N)).astype(np.int8)
    wq[::37, ::11] = -128
    wq[5::53, 3::7] = 127
    sw = (rng.uniform(0.25, 4.0, N) * 2e-4 / np.sqrt(K / 128)).astype(f32)
    return wq, sw


def random_x(rng, M, K):
    return (rng.standard_normal((M, K)) * rng.uniform(0.2, 4.0, (M, 1))).astype(f16)


def exact_weight(K, N, seed=0):
    """gated form (module docstring): (codes int8 [K][N], sw fp32 [N], pivot)"""
    rng = np.random.default_rng(1000 + K * 7 + N + seed)
    w = rng.integers(-2, 3, (K, N))
    pivot = int(rng.integers(0, K))
    w[:, 0::2] = np.abs(w[:, 0::2])
    w[pivot, 0::2] = 1 + (np.arange(N // 2) % 2)
    n = np.arange(N)
    c = np.where(n % 2 == 0, -((n // 2) % 2), -14 + (((n // 2) * 3) % 4))    # gate 2^-1 / 2^0; up 2^-14 .. 2^-11 keeps g * u finite in fp16
    return w.astype(np.int8), np.exp2(c).astype(f32), pivot


def exact_x(M, K, pivot, seed=0):
    """fp16 [M][K]: integers in [0, 4] times 2^a_m, a_m = |(3 m mod 5) - 2|, element `pivot` = 127 * 2^a_m"""
    rng = np.random.default_rng(2000 + M * 13 + K + seed)
    xi = rng.integers(0, 5, (M, K)).astype(np.float64)
    xi[:, pivot] = 127.0
    x = xi * np.exp2(np.abs((3 * np.arange(M) % 5) - 2))[:, None]
    x16 = x.astype(f16)
    assert np.array_equal(x16.astype(np.float64), x)
    return x16


def assert_exact_gated(x16, wq, sw):
    """the codes are the integers, sx is a power of two, SiLU is the identity on every scaled gate value; returns the reference"""
    xq, sx = quant(x16)
    assert np.array_equal(xq.astype(np.float64) * sx[:, None].astype(np.float64), x16.astype(np.float64)), 'the activation codes are not exact'
    assert np.all(np.log2(sx) == np.round(np.log2(sx)))
    g = scale(acc_i64(xq, wq), sx, sw)[:, 0::2]
    assert g.min() >= 32.0
    assert np.array_equal(o.silu_f32(g).view(np.uint32), g.view(np.uint32))
    y = linear(x16, wq, sw, True)
    assert np.isfinite(y.astype(f32)).all()
    return y


# ---- toy checkpoints -----------------------------------------------------------------------------------------------------
def quantize_weight(w_out_in, strategy):
    """a checkpoint's [out][in] weight -> (int8 codes [out][in], scale fp32: [] (tensor) or [out, 1] (channel)), scale = absmax / 127"""
    w = np.asarray(w_out_in, f32)
    amax = np.abs(w).max() if strategy == 'tensor' else np.abs(w).max(axis=1, keepdims=True)
    s = (np.maximum(amax, 1e-8) / 127.0).astype(f32)
    return np.clip(np.rint(w / s), -127, 127).astype(np.int8), s


def quant_config(dialect, strategy='channel', static=False):
    if dialect == 'smooth_quant':    # what `lmdeploy lite smooth_quant` writes (always one scale per output channel)
        return {'quant_method': 'smooth_quant', 'quant_dtype': 'int8', 'modules_to_not_convert': ['lm_head']}
    assert dialect == 'compressed-tensors'
    return {'quant_method': 'compressed-tensors', 'format': 'int-quantized', 'ignore': ['lm_head'],
            'kv_cache_scheme': {'num_bits': 8, 'type': 'float', 'strategy': 'tensor', 'dynamic': False, 'symmetric': True} if static else None,
            'config_groups': {'group_0': {
                'targets': ['Linear'],
                'weights': {'num_bits': 8, 'type': 'int', 'symmetric': True, 'strategy': strategy, 'dynamic': False},
                'input_activations': {'num_bits': 8, 'type': 'int', 'symmetric': True, 'strategy': 'tensor' if static else 'token',
                                      'dynamic': not static}}}}


SCALE_SHAPES = {'[]': (), '[1]': (1,), '[N]': (-1,), '[N,1]': (-1, 1)}


def write_checkpoint(path, *, hidden=256, layers=2, q_heads=2, kv_heads=1, head_dim=128, inter=512, vocab=512, dialect='smooth_quant',
                     strategy='channel', scale_shape=None, scale_dtype=f32, static=False, seed=0, arch='LlamaForCausalLM', experts=0):
    """Writes a toy HF checkpoint (config.json + model.safetensors) with int8 decoder linears (embeddings 0.02 N, linears
    0.1 / sqrt(K) N times a per-channel factor in [0.5, 2]; Qwen2: q / k / v biases 0.1 N) and returns {tensor name: numpy array} of
    what was written plus 'dequant': {linear prefix: fp32 [out][in] = codes * scale} and 'config'.
    smooth_quant stores `<proj>.scale` fp32 [out, 1]; compressed-tensors `<proj>.weight_scale` in `scale_shape` ('[]' | '[1]' per
    tensor, '[N]' | '[N,1]' per channel) and `scale_dtype`.  experts > 0 only writes the config of a MoE architecture (for refusals)."""
    import torch
    from safetensors.torch import save_file

    rng = np.random.default_rng(seed)
    os.makedirs(path, exist_ok=True)
    sq = dialect == 'smooth_quant'
    assert not sq or strategy == 'channel'
    qwen2 = arch == 'Qwen2ForCausalLM'
    cfg = {'architectures': [arch], 'model_type': 'qwen2' if qwen2 else 'llama', 'hidden_size': hidden, 'num_hidden_layers': layers,
           'num_attention_heads': q_heads, 'num_key_value_heads': kv_heads, 'head_dim': head_dim, 'intermediate_size': inter,
           'vocab_size': vocab, 'rms_norm_eps': 1e-5, 'rope_theta': 10000.0, 'max_position_embeddings': 512, 'tie_word_embeddings': False,
           'torch_dtype': 'float16', 'quantization_config': quant_config(dialect, strategy, static)}
    if experts:
        cfg.update(num_local_experts=experts, num_experts_per_tok=2, num_experts=experts, moe_intermediate_size=inter,
                   shared_expert_intermediate_size=0)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(cfg, f)
    scale_shape = scale_shape or ('[N,1]' if strategy == 'channel' else '[]')
    tensors, dequant = {}, {}

    def dense(name, shape, std):
        tensors[name] = (rng.standard_normal(shape) * std).astype(f16)

    def qlinear(prefix, out_f, in_f):
        w = rng.standard_normal((out_f, in_f)) * (0.1 / np.sqrt(in_f)) * rng.uniform(0.5, 2.0, (out_f, 1))
        codes, s = quantize_weight(w, strategy)
        s = np.asarray(s.astype(scale_dtype).astype(f32))    # what the reader sees after widening the stored dtype
        dequant[prefix] = codes.astype(f32) * (s.reshape(-1, 1) if s.ndim else s)
        tensors[prefix + '.weight'] = codes
        if sq:
            tensors[prefix + '.scale'] = s.reshape(-1, 1)
        else:
            tensors[prefix + '.weight_scale'] = s.reshape(SCALE_SHAPES[scale_shape]).astype(scale_dtype)
        if static:                  # read past: calibrated activation scales
            tensors[prefix + '.input_scale'] = np.asarray(0.0123, f32)

    dense('model.embed_tokens.weight', (vocab, hidden), 0.02)
    dense('lm_head.weight', (vocab, hidden), 0.1 / np.sqrt(hidden))
    tensors['model.norm.weight'] = (1 + 0.05 * rng.standard_normal(hidden)).astype(f16)
    for i in range(layers):
        p = f'model.layers.{i}.'
        tensors[p + 'input_layernorm.weight'] = (1 + 0.05 * rng.standard_normal(hidden)).astype(f16)
        tensors[p + 'post_attention_layernorm.weight'] = (1 + 0.05 * rng.standard_normal(hidden)).astype(f16)
        for n, heads in (('q', q_heads), ('k', kv_heads), ('v', kv_heads)):
            qlinear(p + f'self_attn.{n}_proj', heads * head_dim, hidden)
            if qwen2:
                dense(p + f'self_attn.{n}_proj.bias', (heads * head_dim,), 0.1)
        qlinear(p + 'self_attn.o_proj', hidden, q_heads * head_dim)
        if static:
            tensors[p + 'self_attn.k_proj.k_scale'] = np.asarray(0.02, f32)
            tensors[p + 'self_attn.v_proj.v_scale'] = np.asarray(0.03, f32)
        qlinear(p + 'mlp.gate_proj', inter, hidden)
        qlinear(p + 'mlp.up_proj', inter, hidden)
        qlinear(p + 'mlp.down_proj', hidden, inter)
    save_file({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}, os.path.join(path, 'model.safetensors'))
    out = dict(tensors)
    out['dequant'] = dequant
    out['config'] = cfg
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------
def tm_weights(ck: dict, oc: o.ModelConfig) -> dict:
    """the engine-layout weights of a checkpoint written by write_checkpoint, assembled here (not by checkpoint.py): linears
    {'i8': codes [in][out], 'cs': fp32 [out], 'deq': fp32 [in][out] from the written dequantised weights}, q / k output channels
    permuted for the interleaved RoPE, q | k | v concatenated, (gate_j, up_j) interleaved; Qwen2: 'qkv_bias' alike"""
    D, Hq, Hkv = oc.head_dim, oc.q_heads, oc.kv_heads
    perm = o.permute_qk_for_interleaved_rope

    def lin(pre, heads=None):
        codes = ck[pre + '.weight']
        s = ck[pre + ('.scale' if pre + '.scale' in ck else '.weight_scale')]
        cs = np.broadcast_to(np.asarray(s).astype(f32).reshape(-1), (codes.shape[0],))
        d = dict(i8=np.ascontiguousarray(codes.T), cs=np.ascontiguousarray(cs), deq=np.ascontiguousarray(ck['dequant'][pre].T))
        return {k: perm(v, heads, D) for k, v in d.items()} if heads else d

    def fuse(g, u):
        return {k: (o.interleave_w1w3(g[k][None], u[k][None])[0] if g[k].ndim == 1 else o.interleave_w1w3(g[k], u[k])) for k in g}

    layers = []
    for i in range(oc.layers):
        p = f'model.layers.{i}'
        a = p + '.self_attn.'
        q, k, v = lin(a + 'q_proj', Hq), lin(a + 'k_proj', Hkv), lin(a + 'v_proj')
        L = dict(attn_norm=ck[p + '.input_layernorm.weight'], ffn_norm=ck[p + '.post_attention_layernorm.weight'],
                 w_qkv={kk: np.concatenate([q[kk], k[kk], v[kk]], -1) for kk in q}, wo=lin(a + 'o_proj'),
                 w1w3=fuse(lin(p + '.mlp.gate_proj'), lin(p + '.mlp.up_proj')), w2=lin(p + '.mlp.down_proj'))
        if a + 'q_proj.bias' in ck:
            L['qkv_bias'] = np.concatenate([perm(ck[a + 'q_proj.bias'], Hq, D), perm(ck[a + 'k_proj.bias'], Hkv, D), ck[a + 'v_proj.bias']])
        layers.append(L)
    return dict(tok_embeddings=ck['model.embed_tokens.weight'], layers=layers, norm=ck['model.norm.weight'],
                output=np.ascontiguousarray(ck['lm_head.weight'].T))


def oracle_config(ck: dict, kv_bits: int) -> o.ModelConfig:
    c = ck['config']
    return o.ModelConfig(hidden=c['hidden_size'], layers=c['num_hidden_layers'], q_heads=c['num_attention_heads'],
                         kv_heads=c['num_key_value_heads'], head_dim=c['head_dim'], inter=c['intermediate_size'], vocab=c['vocab_size'],
                         rms_eps=c['rms_norm_eps'], rope=o.RopeParam(c['head_dim'], c['rope_theta'], 'default', 1.0, 1.0, 4.0, 8192),
                         kv_bits=kv_bits, weight_format='fp8')


class Int8Model(o.OracleModel):
    """o.OracleModel with every decoder linear the contract above (activations quantised per token, once per GEMM input); layers with
    'qkv_bias' add it to q, k and v in fp16 before RoPE (Qwen2)"""

    def lin(self, x, W, gated=False):
        return linear(x, W['i8'], W['cs'], gated)

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
            if 'qkv_bias' in Lw:
                qkv = o.hadd(qkv, np.asarray(Lw['qkv_bias'], f16)[None, :])
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
            d = self.lin(self.lin(x, Lw['w1w3'], True), Lw['w2'])
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        self.last_resid = resid
        logits = o.lm_head(x[last], self.w['output'])
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits
