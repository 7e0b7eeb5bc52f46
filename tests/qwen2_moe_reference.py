"""Qwen2-MoE on the oracle's primitives, for the Qwen2-MoE parity tests: the Qwen2 attention prologue (q / k / v bias) of
tests.qwen_reference, and in every layer a routed MoE (oracle.tm_oracle's gate and expert arithmetic) next to a dense FFN, the
shared expert, whose output is scaled per token by sigmoid(x . w_shared_gate) before the routed experts are added
(models/llama/unified_decoder.cc:295-318, moe_ffn_layer.cc:295-325, invokeMoeCombine kernels/gemm/moe_utils_v2.cu:1032-1105):
    d = fp16( f32(shared) * sigma64 + sum_j w_j * f32(y_j) ),  shared = w2( silu(w1 x) * (w3 x) ),
with sigma64 evaluated in float64 from the fp16 inputs and the routed terms formed as o.moe_ffn / o.moe_ffn_fp8 form them.
Plus fabricated HF checkpoints (AWQ g128 or block-128 FP8; router and shared gate unquantised) in the reference's tensor names
(lmdeploy/turbomind/models/qwen2.py:110-128)."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, replace

import numpy as np

from oracle import tm_oracle as o
from tests.qwen_moe_reference import QwenMoeOracleModel
from tests.qwen_reference import make_qwen_weights, prologue

f16, f32, f64 = np.float16, np.float32, np.float64


@dataclass
class Qwen2MoeConfig(o.ModelConfig):
    attn_bias: int = 1
    qk_norm: int = 0
    moe_shared_inter: int = 0


# Qwen1.5-MoE-A2.7B's routing (60 experts: the serial router, not a power of two; top-4 of a softmax over all experts) at H 256
QWEN2_MOE_CFG = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=128, vocab=1024, rms_eps=1e-6,
                     rope=o.RopeParam(128, 1e6), attn_bias=1, moe_experts=60, moe_top_k=4, moe_norm_topk=False, moe_shared_inter=384)


def make_qwen2_moe_weights(cfg: Qwen2MoeConfig, seed: int = 0):
    """make_qwen_weights (router, experts of width cfg.inter, qkv bias) plus, per layer, the shared expert -- the dense w1w3 / w2 of
    a model of width cfg.moe_shared_inter, drawn and quantised like every other linear -- and its gate [H] ~ 0.2 N(0, 1).
    The lm_head is the embedding table (tie_word_embeddings), scaled to the column norm the synthetic head has (0.1 / sqrt(H) per
    element against the table's 0.02): with an independent random head the 1024 logits are 0.1 N(0, 1) and the top-2 margin exceeds
    6e-2 at about one (step, sequence) pair in seven whatever the seed (measured on the CPU over seeds 1, 2, 3, 5), so the token
    comparison of the parity run would be nearly empty; through the residual stream a tied head gives the reference the margins of
    a model that has a preferred token, at the same logit scale and hence the same meaning of the 3e-2 bound."""
    w = make_qwen_weights(cfg, seed=seed)
    w['output'] = np.ascontiguousarray((w['tok_embeddings'].astype(f32) * f32(0.1 / np.sqrt(cfg.hidden) / 0.02)).astype(f16).T)
    dense = o.make_synthetic_weights(replace(cfg, moe_experts=0, moe_top_k=0, inter=cfg.moe_shared_inter), seed + 104729)
    rng = np.random.default_rng(seed + 15485863)
    for L, Ld in zip(w['layers'], dense['layers']):
        L['w1w3'], L['w2'] = Ld['w1w3'], Ld['w2']
        L['shared_gate'] = (0.2 * rng.standard_normal(cfg.hidden)).astype(f16)
    return w


def sigma64(x, gate):
    """sigmoid(x . gate) per row, in float64 from the fp16 inputs -> float64 [T]"""
    logit = np.asarray(x, f16).astype(f64) @ np.asarray(gate, f16).astype(f64)
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-logit))


def routed_f32(x, Lw, cfg):
    """sum_j w_j * f32(y_j) in fp32, term by term as o.moe_ffn (or o.moe_ffn_fp8) accumulates it -> float32 [T, H]"""
    _, ids, w = o.moe_gate(x, Lw['moe_gate'], cfg.moe_top_k, cfg.moe_norm_topk, cfg.moe_routed_scale)
    fp8 = cfg.moe_fp8_act and cfg.weight_format == 'fp8'
    if not fp8 and '_dense' not in Lw:
        Lw['_dense'] = [(o._dense_weight(E_['w1w3'], cfg.group), o._dense_weight(E_['w2'], cfg.group)) for E_ in Lw['experts']]
    T, H = x.shape
    out = np.zeros((T, H), f32)
    for t in range(T):
        for j in range(cfg.moe_top_k):
            if fp8:
                E_ = Lw['experts'][ids[t, j]]
                act = o.fp8_act_linear(x[t:t + 1], E_['w1w3']['f8'], E_['w1w3']['bs'], gated=True)
                y = o.fp8_act_linear(act, E_['w2']['f8'], E_['w2']['bs'])
            else:
                w13, w2 = Lw['_dense'][ids[t, j]]
                act = o.gated_silu_epilogue(o.gemm_f16_f32acc(x[t:t + 1], w13))
                y = o.gemm_f16_f32acc(act, w2).astype(f16)
            out[t] += w[t, j] * y[0].astype(f32)
    return out


def shared_combine(shared, x, gate, routed):
    """d = fp16( f32(shared) * sigma64 + routed ): shared fp16 [T, H], routed float32 [T, H] (routed_f32) -> fp16 [T, H]"""
    s = sigma64(x, gate)
    return (np.asarray(shared, f16).astype(f64) * s[:, None] + np.asarray(routed, f32).astype(f64)).astype(f16)


def shared_moe_ffn(x, Lw, cfg):
    """the FFN of a Qwen2-MoE layer -> fp16 [T, H]"""
    shared = o._linear(o._linear(x, Lw['w1w3'], cfg.group, gated=True), Lw['w2'], cfg.group)
    return shared_combine(shared, x, Lw['shared_gate'], routed_f32(x, Lw, cfg))


class Qwen2MoeOracleModel(QwenMoeOracleModel):
    """QwenMoeOracleModel.forward with the FFN line replaced by shared_moe_ffn"""

    def forward(self, ids_per_seq, decode_splits=1):
        cfg = self.cfg
        assert cfg.moe_experts and cfg.moe_shared_inter
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
            d = shared_moe_ffn(x, Lw, cfg)
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        self.last_resid = resid
        logits = o.lm_head(x[last], self.w['output'])
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits


PARITY_SEED = 3          # chosen on the CPU: see safe_fraction
MIN_SAFE = 2.0 / 3.0


def parity_inputs(fmt: str, kv_bits: int, seed: int = PARITY_SEED, prompt_lens=(70, 5, 64)):
    cfg = Qwen2MoeConfig(**QWEN2_MOE_CFG, kv_bits=kv_bits, weight_format=fmt, moe_fp8_act=fmt == 'fp8')
    w = make_qwen2_moe_weights(cfg, seed=seed)
    rng = np.random.default_rng(0)
    return cfg, w, [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in prompt_lens]


def safe_fraction(fmt: str, kv_bits: int, seed: int = PARITY_SEED, steps: int = 6, session_len: int = 256) -> float:
    """CPU only: the share of (step, sequence) pairs of the parity run at which the reference's top-2 margin exceeds 6e-2, with the
    reference generating greedily on its own.  The seed of the parity run was picked with this so that the token comparison of
    engine_vs_oracle_qwen2_moe covers at least two thirds of the pairs (1.0 in all three arms at seeds 1 and 3; see
    make_qwen2_moe_weights for the head)."""
    cfg, w, prompts = parity_inputs(fmt, kv_bits, seed)
    om = Qwen2MoeOracleModel(cfg, w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    safe = []
    for s in range(steps + 1):
        top2 = np.sort(lg.astype(f32), -1)[:, -2:]
        safe.append((top2[:, 1] - top2[:, 0]) > 6e-2)
        if s < steps:
            ids, lg = om.forward([[int(t)] for t in ids])
    return float(np.mean(safe))


def engine_vs_oracle_qwen2_moe(fmt: str, kv_bits: int, use_graph: int, steps: int = 6, seed: int = PARITY_SEED, max_prefill: int = 96,
                               session_len: int = 256):
    """tests.qwen_reference.engine_vs_oracle for the Qwen2-MoE geometry, its bounds: logits within 3e-2, greedy tokens equal where
    the reference's top-2 margin exceeds 6e-2 -- and at least two thirds of the (step, sequence) pairs must be such"""
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights
    cfg, w, prompts = parity_inputs(fmt, kv_bits, seed)
    eng = Engine.from_model_config(cfg, weight_type=2 if fmt == 'fp8' else 0, max_batch_size=len(prompts), session_len=session_len,
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
    om = Qwen2MoeOracleModel(cfg, w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    ref_logits, ref_toks = [lg], [ids]
    cur = toks[:, 0]
    for s in range(steps):
        ids, lg = om.forward([[int(t)] for t in cur])
        ref_logits.append(lg)
        ref_toks.append(ids)
        cur = toks[:, s + 1]
    worst, n_safe = 0.0, 0
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s].astype(f32))
        worst = max(worst, float(d.max()))
        print(f'{fmt} kv{kv_bits} graph {use_graph} step {s}: max logit diff {d.max():.4f}')
        assert d.max() <= 3e-2, f'{fmt} step {s}: max logit diff {d.max()}'
        top2 = np.sort(ref_logits[s].astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        n_safe += int(safe.sum())
        assert np.array_equal(toks[safe, s], ref_toks[s][safe]), f'{fmt} step {s}: greedy tokens differ'
    frac = n_safe / ((steps + 1) * len(prompts))
    print(f'{fmt} kv{kv_bits} graph {use_graph}: {n_safe} of {(steps + 1) * len(prompts)} (step, sequence) pairs safe')
    assert frac >= MIN_SAFE, f'only {frac:.2f} of the (step, sequence) pairs have a top-2 margin above 6e-2'
    return worst


def hf_qwen2_moe_tensors(rng, H: int, Hq: int, Hkv: int, I: int, S: int, E: int, V: int, layers: int = 2, D: int = 128) -> dict:
    """Random HF-layout (linears [out, in]) fp16 tensors of a Qwen2-MoE decoder: q / k / v bias, router mlp.gate [E, H], experts
    mlp.experts.X.{gate,up,down}_proj of width I, mlp.shared_expert.{gate,up,down}_proj of width S, mlp.shared_expert_gate [1, H]"""
    t = {}
    for i in range(layers):
        p = f'model.layers.{i}'
        for n, (o_, i_) in dict(q_proj=(Hq * D, H), k_proj=(Hkv * D, H), v_proj=(Hkv * D, H), o_proj=(H, Hq * D)).items():
            t[f'{p}.self_attn.{n}.weight'] = (rng.standard_normal((o_, i_)) * (0.1 / np.sqrt(i_))).astype(f16)
            if n != 'o_proj':
                t[f'{p}.self_attn.{n}.bias'] = (0.1 * rng.standard_normal(o_)).astype(f16)
        t[f'{p}.mlp.gate.weight'] = (0.2 * rng.standard_normal((E, H))).astype(f16)
        ffns = [(f'{p}.mlp.experts.{x}', I) for x in range(E)] + [(f'{p}.mlp.shared_expert', S)]
        for pre, width in ffns:
            for n, (o_, i_) in dict(gate_proj=(width, H), up_proj=(width, H), down_proj=(H, width)).items():
                t[f'{pre}.{n}.weight'] = (rng.standard_normal((o_, i_)) * (0.1 / np.sqrt(i_))).astype(f16)
        t[f'{p}.mlp.shared_expert_gate.weight'] = (0.2 * rng.standard_normal((1, H))).astype(f16)
        t[f'{p}.input_layernorm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
        t[f'{p}.post_attention_layernorm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    t['model.embed_tokens.weight'] = (0.02 * rng.standard_normal((V, H))).astype(f16)
    t['model.norm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    t['lm_head.weight'] = (rng.standard_normal((V, H)) * (0.1 / np.sqrt(H))).astype(f16)
    return t


def qwen2_moe_config_json(H: int, Hq: int, Hkv: int, I: int, S: int, E: int, k: int, V: int, layers: int, fmt: str, **extra) -> dict:
    c = {'architectures': ['Qwen2MoeForCausalLM'], 'hidden_size': H, 'num_hidden_layers': layers, 'num_attention_heads': Hq,
         'num_key_value_heads': Hkv, 'intermediate_size': 4 * H, 'moe_intermediate_size': I, 'shared_expert_intermediate_size': S,
         'num_experts': E, 'num_experts_per_tok': k, 'norm_topk_prob': False, 'decoder_sparse_step': 1, 'mlp_only_layers': [],
         'vocab_size': V, 'rms_norm_eps': 1e-6, 'rope_theta': 1000000.0, 'max_position_embeddings': 32768, 'tie_word_embeddings': False,
         'use_sliding_window': False, 'sliding_window': 32768, 'eos_token_id': 151643, 'head_dim': 128}
    if fmt == 'awq':
        c['quantization_config'] = {'quant_method': 'awq', 'bits': 4, 'group_size': 128, 'zero_point': True, 'version': 'gemm'}
    elif fmt == 'fp8':
        c['quantization_config'] = {'quant_method': 'fp8', 'weight_block_size': [128, 128]}
    c.update(extra)
    return c


def write_qwen2_moe_checkpoint(path: str, hf: dict, H: int, Hq: int, Hkv: int, I: int, S: int, E: int, k: int, V: int, layers: int = 2,
                               fmt: str = 'awq', extra_cfg: dict = None) -> dict:
    """config.json + generation_config.json + model.safetensors of a Qwen2-MoE checkpoint.  Every *_proj is quantised (AWQ g128:
    qweight / qzeros / scales; fp8: e4m3 weight + weight_scale_inv [out/128, in/128]); the router, the shared gate, biases, norms,
    embeddings and lm_head stay fp16.  Returns {linear prefix: engine-layout linear dict ([in, out]: q / s / z or f8 / bs)}."""
    import torch
    from safetensors.torch import save_file
    tensors, quant = {}, {}
    for name, v in hf.items():
        if name.endswith('_proj.weight'):
            pre = name[:-len('.weight')]
            wt = np.ascontiguousarray(v.T)                     # [in, out]
            if fmt == 'awq':
                q, s, z, _ = o.quantize_groupwise_u4(wt, 128)
                tensors[pre + '.qweight'] = torch.from_numpy(o.pack_awq_gemm(q))
                tensors[pre + '.qzeros'] = torch.from_numpy(o.pack_awq_gemm(z.astype(np.uint8)))
                tensors[pre + '.scales'] = torch.from_numpy(s)
                quant[pre] = dict(q=q, s=s, z=z.astype(f16))
            else:
                f8, bs = o.fp8_quantize_blockwise(wt)          # codes [in, out], scales [in/128, out/128]
                tensors[pre + '.weight'] = torch.from_numpy(np.ascontiguousarray(f8.T)).view(torch.float8_e4m3fn)
                tensors[pre + '.weight_scale_inv'] = torch.from_numpy(np.ascontiguousarray(bs.T))
                quant[pre] = dict(f8=f8, bs=bs)
        else:
            tensors[name] = torch.from_numpy(v)
    save_file(tensors, os.path.join(path, 'model.safetensors'))
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(qwen2_moe_config_json(H, Hq, Hkv, I, S, E, k, V, layers, fmt, **(extra_cfg or {})), f)
    with open(os.path.join(path, 'generation_config.json'), 'w') as f:
        json.dump({'eos_token_id': [151645, 151643], 'bos_token_id': 151643}, f)
    return quant
