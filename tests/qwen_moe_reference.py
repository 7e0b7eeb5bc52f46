"""Qwen3-MoE on the oracle's primitives, for the Qwen3-MoE parity tests: the Qwen3 attention prologue of tests.qwen_reference with
the routed expert FFN of oracle.tm_oracle (moe_ffn / moe_ffn_fp8) in every layer, plus fabricated HF checkpoints (AWQ g128 or
block-128 FP8; the router stays unquantised) in the reference's tensor names (lmdeploy/turbomind/models/qwen3.py:110-121)."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass

import numpy as np

from oracle import tm_oracle as o
from tests.qwen_reference import QwenOracleModel, make_qwen_weights, prologue

f16, f32 = np.float16, np.float32


@dataclass
class QwenMoeConfig(o.ModelConfig):
    attn_bias: int = 0
    qk_norm: int = 1


# 72 experts: above the serial router's 64 and not a power of two
QWEN3_MOE_CFG = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=128, vocab=1024, rms_eps=1e-6,
                     rope=o.RopeParam(128, 1e6), qk_norm=1, moe_experts=72, moe_top_k=8, moe_norm_topk=True)


def make_qwen_moe_weights(cfg: QwenMoeConfig, seed: int = 0):
    return make_qwen_weights(cfg, seed=seed)


class QwenMoeOracleModel(QwenOracleModel):
    """QwenOracleModel.forward with the FFN line replaced by o.moe_ffn / o.moe_ffn_fp8"""

    def forward(self, ids_per_seq, decode_splits=1):
        cfg = self.cfg
        assert cfg.moe_experts
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
            if cfg.moe_fp8_act and cfg.weight_format == 'fp8':
                exq = [((E_['w1w3']['f8'], E_['w1w3']['bs']), (E_['w2']['f8'], E_['w2']['bs'])) for E_ in Lw['experts']]
                d, _, _ = o.moe_ffn_fp8(x, Lw['moe_gate'], exq, cfg.moe_top_k, cfg.moe_norm_topk, cfg.moe_routed_scale)
            else:
                if '_dense' not in Lw:
                    Lw['_dense'] = [(o._dense_weight(E_['w1w3'], cfg.group), o._dense_weight(E_['w2'], cfg.group))
                                    for E_ in Lw['experts']]
                d, _, _ = o.moe_ffn(x, Lw['moe_gate'], Lw['_dense'], cfg.moe_top_k, cfg.moe_norm_topk, cfg.moe_routed_scale)
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        self.last_resid = resid
        logits = o.lm_head(x[last], self.w['output'])
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits


def engine_vs_oracle_moe(fmt: str, kv_bits: int, use_graph: int, prompt_lens=(70, 5, 64), steps: int = 6, seed: int = 3,
                         max_prefill: int = 96, session_len: int = 256):
    """tests.qwen_reference.engine_vs_oracle for the Qwen3-MoE geometry (E 72, top-8, qk_norm; u4 or e4m3 experts), its bounds"""
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights
    cfg = QwenMoeConfig(**QWEN3_MOE_CFG, kv_bits=kv_bits, weight_format=fmt, moe_fp8_act=fmt == 'fp8')
    w = make_qwen_moe_weights(cfg, seed=seed)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in prompt_lens]
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
    om = QwenMoeOracleModel(cfg, w, batch=len(prompts), max_ctx=session_len)
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
        assert d.max() <= 3e-2, f'{fmt} step {s}: max logit diff {d.max()}'
        top2 = np.sort(ref_logits[s].astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ref_toks[s][safe]), f'{fmt} step {s}: greedy tokens differ'
    return worst


def hf_qwen_moe_tensors(rng, H: int, Hq: int, Hkv: int, I: int, E: int, V: int, layers: int = 2, D: int = 128) -> dict:
    """Random HF-layout (linears [out, in]) fp16 tensors of a Qwen3-MoE decoder: q_norm / k_norm, router mlp.gate [E, H], experts
    mlp.experts.X.{gate_proj, up_proj, down_proj}"""
    t = {}
    for i in range(layers):
        p = f'model.layers.{i}'
        for n, (o_, i_) in dict(q_proj=(Hq * D, H), k_proj=(Hkv * D, H), v_proj=(Hkv * D, H), o_proj=(H, Hq * D)).items():
            t[f'{p}.self_attn.{n}.weight'] = (rng.standard_normal((o_, i_)) * (0.1 / np.sqrt(i_))).astype(f16)
        t[f'{p}.self_attn.q_norm.weight'] = (1 + 0.05 * rng.standard_normal(D)).astype(f16)
        t[f'{p}.self_attn.k_norm.weight'] = (1 + 0.05 * rng.standard_normal(D)).astype(f16)
        t[f'{p}.mlp.gate.weight'] = (0.2 * rng.standard_normal((E, H))).astype(f16)
        for x in range(E):
            for n, (o_, i_) in dict(gate_proj=(I, H), up_proj=(I, H), down_proj=(H, I)).items():
                t[f'{p}.mlp.experts.{x}.{n}.weight'] = (rng.standard_normal((o_, i_)) * (0.1 / np.sqrt(i_))).astype(f16)
        t[f'{p}.input_layernorm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
        t[f'{p}.post_attention_layernorm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    t['model.embed_tokens.weight'] = (0.02 * rng.standard_normal((V, H))).astype(f16)
    t['model.norm.weight'] = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    t['lm_head.weight'] = (rng.standard_normal((V, H)) * (0.1 / np.sqrt(H))).astype(f16)
    return t


def qwen_moe_config_json(H: int, Hq: int, Hkv: int, I: int, E: int, k: int, V: int, layers: int, fmt: str, **extra) -> dict:
    c = {'architectures': ['Qwen3MoeForCausalLM'], 'hidden_size': H, 'num_hidden_layers': layers, 'num_attention_heads': Hq,
         'num_key_value_heads': Hkv, 'intermediate_size': 4 * H, 'moe_intermediate_size': I, 'num_experts': E,
         'num_experts_per_tok': k, 'norm_topk_prob': True, 'decoder_sparse_step': 1, 'mlp_only_layers': [], 'vocab_size': V,
         'rms_norm_eps': 1e-6, 'rope_theta': 1000000.0, 'max_position_embeddings': 32768, 'tie_word_embeddings': False,
         'use_sliding_window': False, 'eos_token_id': 151645, 'head_dim': 128, 'attention_bias': False}
    if fmt == 'awq':
        c['quantization_config'] = {'quant_method': 'awq', 'bits': 4, 'group_size': 128, 'zero_point': True, 'version': 'gemm'}
    elif fmt == 'fp8':
        c['quantization_config'] = {'quant_method': 'fp8', 'weight_block_size': [128, 128]}
    c.update(extra)
    return c


def write_qwen_moe_checkpoint(path: str, hf: dict, H: int, Hq: int, Hkv: int, I: int, E: int, k: int, V: int, layers: int = 2,
                              fmt: str = 'awq', extra_cfg: dict = None) -> dict:
    """config.json + model.safetensors of a Qwen3-MoE checkpoint.  Every *_proj is quantised (AWQ g128: qweight / qzeros / scales;
    fp8: e4m3 weight + weight_scale_inv [out/128, in/128]); the router, norms, embeddings and lm_head stay fp16.
    Returns {linear prefix: engine-layout linear dict ([in, out]: q / s / z or f8 / bs)} of what was written."""
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
        json.dump(qwen_moe_config_json(H, Hq, Hkv, I, E, k, V, layers, fmt, **(extra_cfg or {})), f)
    with open(os.path.join(path, 'generation_config.json'), 'w') as f:
        json.dump({'eos_token_id': [151645, 151643], 'bos_token_id': 151643}, f)
    return quant
