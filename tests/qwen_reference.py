"""Qwen2 / Qwen3 dense decoders restated on the oracle's primitives (oracle.tm_oracle), for the Qwen parity tests.

The two differences from the Llama data flow sit in the attention prologue, in the reference's order:
  * Qwen3: per-head RMSNorm of q and k over head_dim with weights q_norm / k_norm [128], after the QKV GEMM
    (unified_attention_layer.cc:395,720-748; kernels/norm/rms_norm.cu:141-207) -- o.rmsnorm over the last axis;
  * Qwen2: the q / k / v projection bias, an fp16 add before RoPE (attention_universal.h:110-165 for q,
    kv_cache_utils_v2.cu:73-124 for the prefill K / V) -- o.hadd;
then RoPE (o.rope_apply / o.process_kv) as for Llama.  V gets the bias only.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import tm_oracle as o

f16, f32 = np.float16, np.float32


@dataclass
class QwenConfig(o.ModelConfig):
    attn_bias: int = 0
    qk_norm: int = 0


def head_norm(x, w, eps):
    """per-head RMSNorm: x fp16 [..., heads, D], w fp16 [D]"""
    return o.rmsnorm(x, w, eps)


def head_norm_kernel_order(x, w, eps):
    """head_norm with the device's fp32 summation order (tm_common.h: sumsq8 + group_sum<16>): 8 squares per 16-byte chunk in
    channel order, then the 16 chunk sums as a pairwise tree.  Bit-exact to the kernels; within 1 ulp of head_norm."""
    x = np.asarray(x, f16)
    xf = x.astype(f32)
    sq = (xf * xf).reshape(*x.shape[:-1], 16, 8)
    acc = np.zeros(sq.shape[:-1], f32)
    for e in range(8):
        acc = acc + sq[..., e]
    for _ in range(4):
        acc = acc[..., 0::2] + acc[..., 1::2]
    ss = acc[..., 0:1]
    inv = f32(1) / np.sqrt(ss * f32(1.0 / 128) + f32(eps))
    return o.hmul((xf * inv).astype(f16), np.asarray(w, f16))


def prologue(q, k, v, Lw, eps, norm=head_norm):
    """q [n, Hq, D], k / v [n, Hkv, D] fp16 straight from the QKV GEMM -> (q, k, v) before RoPE"""
    if 'q_norm' in Lw:
        q, k = norm(q, Lw['q_norm'], eps), norm(k, Lw['k_norm'], eps)
    if 'qkv_bias' in Lw:
        Hq, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
        b = np.asarray(Lw['qkv_bias'], f16)
        q = o.hadd(q, b[:Hq * D].reshape(Hq, D))
        k = o.hadd(k, b[Hq * D:(Hq + Hkv) * D].reshape(Hkv, D))
        v = o.hadd(v, b[(Hq + Hkv) * D:].reshape(Hkv, D))
    return q, k, v


def make_qwen_weights(cfg: QwenConfig, seed: int = 0, quantized: bool = True):
    """o.make_synthetic_weights plus the prologue tensors in the engine's layout: qkv_bias [(Hq + 2 Hkv) D] ~ 0.1 N(0,1) (the
    projections are ~0.1 N as well) and / or q_norm, k_norm [D] = 1 + 0.05 N(0,1)."""
    w = o.make_synthetic_weights(cfg, seed, quantized)
    rng = np.random.default_rng(seed + 7919)
    n = (cfg.q_heads + 2 * cfg.kv_heads) * cfg.head_dim
    for L in w['layers']:
        if cfg.attn_bias:
            L['qkv_bias'] = (0.1 * rng.standard_normal(n)).astype(f16)
        if cfg.qk_norm:
            L['q_norm'] = (1 + 0.05 * rng.standard_normal(cfg.head_dim)).astype(f16)
            L['k_norm'] = (1 + 0.05 * rng.standard_normal(cfg.head_dim)).astype(f16)
    return w


class QwenOracleModel(o.OracleModel):
    """o.OracleModel (dense FFN) with the Qwen attention prologue between the QKV GEMM and RoPE."""

    def forward(self, ids_per_seq, decode_splits=1):
        cfg = self.cfg
        assert not cfg.moe_experts
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
                q, k, v = prologue(qkv[sl, :Hq * D].reshape(n, Hq, D), qkv[sl, Hq * D:(Hq + Hkv) * D].reshape(n, Hkv, D),
                                   qkv[sl, (Hq + Hkv) * D:].reshape(n, Hkv, D), Lw, cfg.rms_eps)
                q = o.rope_apply(q, cos, sin)
                o.process_kv(self.cache, self.tables[b], li, k, v, cos, sin, hist)
                if n == 1:
                    kv = [self.cache.load_dequant(self.tables[b], li, hd, 0, hist + 1, 'decode') for hd in range(Hkv)]
                    attn[sl] = o.decode_attention(q[0], np.stack([a for a, _ in kv]), np.stack([c for _, c in kv]), self.c,
                                                  decode_splits).reshape(1, -1)
                else:
                    Kf, Vf = o.flatten_kv(self.cache, self.tables[b], li, hist + n)
                    attn[sl] = o.prefill_attention(q, Kf, Vf, hist, self.c).reshape(n, -1)
            resid, x = o.residual_rmsnorm(resid, o._linear(attn, Lw['wo'], cfg.group), Lw['ffn_norm'], cfg.rms_eps)
            d = o._linear(o._linear(x, Lw['w1w3'], cfg.group, gated=True), Lw['w2'], cfg.group)
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        self.last_resid = resid
        logits = o.lm_head(x[last], self.w['output'])
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits


QWEN2_CFG = dict(hidden=256, layers=2, q_heads=7, kv_heads=1, head_dim=128, inter=512, vocab=1024, rms_eps=1e-6,
                 rope=o.RopeParam(128, 1e6), attn_bias=1)        # group 7, q_heads * 128 != hidden
QWEN3_CFG = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, rms_eps=1e-6,
                 rope=o.RopeParam(128, 1e6), qk_norm=1)          # q_heads * 128 = 512 != hidden


def engine_vs_oracle(kind: str, kv_bits: int, use_graph: int, prompt_lens=(70, 5, 64), steps: int = 6, seed: int = 3,
                     max_prefill: int = 96, session_len: int = 256):
    """prefill + `steps` decode steps of the engine against QwenOracleModel (teacher-forced with the engine's tokens).
    Returns the worst logit difference; asserts the bounds of test_gpu_engine.test_engine_matches_oracle."""
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights
    cfg = QwenConfig(**(QWEN2_CFG if kind == 'qwen2' else QWEN3_CFG), kv_bits=kv_bits)
    w = make_qwen_weights(cfg, seed=seed)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in prompt_lens]
    eng = Engine.from_model_config(cfg, max_batch_size=len(prompts), session_len=session_len,
                                   quant_policy=0 if kv_bits == 16 else kv_bits, max_prefill_token_num=max_prefill,
                                   use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits().copy()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    eng.close()
    om = QwenOracleModel(cfg, w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    ref_logits, ref_toks = [lg], [ids]
    cur = toks[:, 0]
    for s in range(steps):
        ids, lg = om.forward([[int(t)] for t in cur])
        ref_logits.append(lg)
        ref_toks.append(ids)
        cur = toks[:, s + 1]
    worst = 0.0
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s].astype(f32))
        worst = max(worst, float(d.max()))
        assert d.max() <= 3e-2, f'{kind} step {s}: max logit diff {d.max()}'
        top2 = np.sort(ref_logits[s].astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ref_toks[s][safe]), f'{kind} step {s}: greedy tokens differ'
    return worst


def hf_qwen_tensors(rng, kind: str, H: int, Hq: int, Hkv: int, I: int, V: int, layers: int = 1, D: int = 128, bias: bool = None,
                    tie: bool = False) -> dict:
    """Random HF-layout (linears [out, in]) fp16 tensors of a Qwen2 (bias) / Qwen3 (q_norm, k_norm; bias if `bias`) decoder"""
    bias = (kind == 'qwen2') if bias is None else bias
    t = {}
    for i in range(layers):
        p = f'model.layers.{i}'
        for n, (o_, i_) in dict(q_proj=(Hq * D, H), k_proj=(Hkv * D, H), v_proj=(Hkv * D, H), o_proj=(H, Hq * D),
                                gate_proj=(I, H), up_proj=(I, H), down_proj=(H, I)).items():
            blk = 'self_attn' if n.endswith(('q_proj', 'k_proj', 'v_proj', 'o_proj')) else 'mlp'
            t[f'{p}.{blk}.{n}.weight'] = (rng.standard_normal((o_, i_)) * (0.1 / np.sqrt(i_))).astype(f16)
            if bias and n in ('q_proj', 'k_proj', 'v_proj'):
                t[f'{p}.self_attn.{n}.bias'] = (0.1 * rng.standard_normal(o_)).astype(f16)
        if kind == 'qwen3':
            t[f'{p}.self_attn.q_norm.weight'] = (1 + 0.05 * rng.standard_normal(D)).astype(f16)
            t[f'{p}.self_attn.k_norm.weight'] = (1 + 0.05 * rng.standard_normal(D)).astype(f16)
        t[f'{p}.input_layernorm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
        t[f'{p}.post_attention_layernorm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    t['model.embed_tokens.weight'] = (0.02 * rng.standard_normal((V, H))).astype(f16)
    t['model.norm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    if not tie:
        t['lm_head.weight'] = (rng.standard_normal((V, H)) * (0.1 / np.sqrt(H))).astype(f16)
    return t


def write_qwen_checkpoint(path: str, kind: str, hf: dict, H: int, Hq: int, Hkv: int, I: int, V: int, layers: int = 1,
                          awq: bool = False, tie: bool = False, bias: bool = None, extra_cfg: dict = None) -> dict:
    """config.json + generation_config.json + model.safetensors of a Qwen2 / Qwen3 checkpoint (AWQ: every projection quantised
    g128, biases and norms stay fp16).  Returns {linear prefix: (q uint8 [K, N], s, z)} of the AWQ tensors written."""
    import json
    import os

    from safetensors.numpy import save_file
    tensors, quant = {}, {}
    for k, v in hf.items():
        if awq and k.endswith('_proj.weight'):
            pre = k[:-len('.weight')]
            q, s, z, _ = o.quantize_groupwise_u4(np.ascontiguousarray(v.T), 128)
            tensors[pre + '.qweight'] = o.pack_awq_gemm(q)
            tensors[pre + '.qzeros'] = o.pack_awq_gemm(z.astype(np.uint8))
            tensors[pre + '.scales'] = s
            quant[pre] = (q, s, z)
        else:
            tensors[k] = v
    save_file(tensors, os.path.join(path, 'model.safetensors'))
    c = {'architectures': ['Qwen3ForCausalLM' if kind == 'qwen3' else 'Qwen2ForCausalLM'], 'hidden_size': H,
         'num_hidden_layers': layers, 'num_attention_heads': Hq, 'num_key_value_heads': Hkv, 'intermediate_size': I,
         'vocab_size': V, 'rms_norm_eps': 1e-6, 'rope_theta': 1000000.0, 'max_position_embeddings': 32768,
         'tie_word_embeddings': tie, 'use_sliding_window': False, 'sliding_window': 32768, 'eos_token_id': 151643,
         'head_dim': 128}       # (the small test shapes have hidden != heads * 128)
    if kind == 'qwen3':
        c.update(attention_bias=bool(bias))
    if awq:
        c['quantization_config'] = {'quant_method': 'awq', 'bits': 4, 'group_size': 128, 'zero_point': True, 'version': 'gemm'}
    c.update(extra_cfg or {})
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)
    with open(os.path.join(path, 'generation_config.json'), 'w') as f:
        json.dump({'eos_token_id': [151645, 151643], 'bos_token_id': 151643}, f)
    return quant


def tm_weights_from_hf(hf: dict, cfg: QwenConfig, quant: dict = None) -> dict:
    """The engine-layout weights of a fabricated checkpoint, assembled here (not by checkpoint.py): [in, out] linears, q / k
    output channels permuted for the interleaved RoPE (bias included), q_norm / k_norm permuted as one head."""
    D, Hq, Hkv = cfg.head_dim, cfg.q_heads, cfg.kv_heads
    perm = o.permute_qk_for_interleaved_rope

    def lin(pre, heads=None):
        if quant and pre in quant:
            q, s, z = quant[pre]
            d = dict(q=q, s=s, z=z.astype(f16))
        else:
            d = dict(w=np.ascontiguousarray(hf[pre + '.weight'].T))
        return {k: perm(v, heads, D) for k, v in d.items()} if heads else d
    layers = []
    for i in range(cfg.layers):
        p = f'model.layers.{i}'
        a = p + '.self_attn.'
        q, k, v = lin(a + 'q_proj', Hq), lin(a + 'k_proj', Hkv), lin(a + 'v_proj')
        g, u = lin(p + '.mlp.gate_proj'), lin(p + '.mlp.up_proj')
        L = dict(attn_norm=hf[p + '.input_layernorm.weight'], ffn_norm=hf[p + '.post_attention_layernorm.weight'],
                 w_qkv={kk: np.concatenate([q[kk], k[kk], v[kk]], -1) for kk in q}, wo=lin(a + 'o_proj'),
                 w1w3={kk: o.interleave_w1w3(g[kk], u[kk]) for kk in g}, w2=lin(p + '.mlp.down_proj'))
        if a + 'q_proj.bias' in hf:
            L['qkv_bias'] = np.concatenate([perm(hf[a + 'q_proj.bias'], Hq, D), perm(hf[a + 'k_proj.bias'], Hkv, D),
                                            hf[a + 'v_proj.bias']])
        if a + 'q_norm.weight' in hf:
            L['q_norm'], L['k_norm'] = perm(hf[a + 'q_norm.weight'], 1, D), perm(hf[a + 'k_norm.weight'], 1, D)
        layers.append(L)
    emb = hf['model.embed_tokens.weight']
    head = hf.get('lm_head.weight', emb)
    return dict(tok_embeddings=emb, layers=layers, norm=hf['model.norm.weight'], output=np.ascontiguousarray(head.T))
