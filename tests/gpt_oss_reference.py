"""gpt-oss (GptOssForCausalLM) restated in the engine's arithmetic at the model's own, UNPADDED width, and the toy checkpoints the
gpt-oss tests share.

The model is composed from what the repository already restates, nothing is new arithmetic:
  * attention      tests.attention_window_reference (per-layer sliding window, sinks) behind tests.qwen_reference.prologue (q / k / v
                   bias in fp16 before RoPE), RoPE from a packed YaRN table (tests.rope_scaling_reference.table_packed layout);
  * o_proj bias    oracle.residual_rmsnorm's bias term: r = h(h(r + wo_out) + bias);
  * MoE block      tests.mxfp4_reference.block_forward (router bias, softmax over the top-k, clamped activation, expert biases) on the
                   dequantised MXFP4 experts, or on the fp16 experts as they are.
Its weights are read back from the engine's SLOTS (loader.export_weights of checkpoint.load_hf_weights) with the zero padding cut
off, so a comparison with transformers covers the reader, the q / k permutation, the expert mapping and the padding at once.

The toy: hidden 192 (-> 256 padded), inter 320 (-> 384), 2 layers [sliding, full], window 8, 4 / 2 heads of 64, 4 experts top-2,
vocab 512, YaRN factor 4 over an original 32 with `truncate: false`.  Every parameter is a bf16 value and every expert weight an
MXFP4 value (e2m1 code x 2^k), so the fp32 transformers model, the bf16 `save_pretrained` checkpoint, the published-layout MXFP4
checkpoint and the engine's fp16 slots all hold the SAME numbers.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass

import numpy as np

from oracle import tm_oracle as o
from tests import attention_window_reference as AW
from tests import mxfp4_reference as MX
from tests.qwen_reference import prologue

f16, f32, f64 = np.float16, np.float32, np.float64

TOY = dict(hidden_size=192, intermediate_size=320, num_hidden_layers=2, layer_types=['sliding_attention', 'full_attention'],
           sliding_window=8, num_attention_heads=4, num_key_value_heads=2, head_dim=64, num_local_experts=4, num_experts_per_tok=2,
           vocab_size=512, max_position_embeddings=128, rms_norm_eps=1e-5, tie_word_embeddings=False, attention_bias=True,
           rope_parameters=dict(rope_type='yarn', rope_theta=150000.0, factor=4.0, beta_fast=32.0, beta_slow=1.0, truncate=False,
                                original_max_position_embeddings=32))
H, I, E, V, LAYERS = 192, 320, 4, 512, 2


@dataclass
class GptOssConfig(AW.WindowConfig):
    attn_bias: int = 1
    attn_out_bias: int = 1
    moe_expert_format: int = 3
    moe_act: int = 1
    moe_bias: int = 1
    rope_table: np.ndarray = None      # fp16 [rows][D / 2][2]: replaces the oracle's RoPE table look-up (YaRN)


# ---- the toy model and its two checkpoints ------------------------------------------------------------------------------------------
def build_toy(seed: int):
    """-> (transformers GptOssForCausalLM in fp32 with eager attention, the experts' MXFP4 images {name: (blocks, scales)})"""
    import torch
    from transformers import GptOssConfig as HfConfig
    from transformers import GptOssForCausalLM
    cfg = HfConfig(**TOY)
    cfg._attn_implementation = 'eager'
    torch.manual_seed(seed)
    model = GptOssForCausalLM(cfg).float().eval()
    rng = np.random.default_rng(seed)
    images = {}
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('experts.gate_up_proj') or name.endswith('experts.down_proj'):
                K, N = p.shape[1], p.shape[2]
                lins = [MX.random_linear(rng, K, N, scale_byte=122 if N == 2 * I else 121) for _ in range(E)]
                images[name] = (np.stack([l['blocks'] for l in lins]), np.stack([l['scales'] for l in lins]))
                w = np.stack([MX.dequant(**l) for l in lins]).astype(f32)          # [E][K][N]
            elif name.endswith('layernorm.weight') or name.endswith('norm.weight'):
                w = 1 + 0.05 * rng.standard_normal(p.shape)
            elif name.endswith('sinks'):
                w = rng.uniform(-2.0, 4.0, p.shape)
            elif name.endswith('router.bias'):
                w = 0.5 * rng.standard_normal(p.shape)
            elif name.endswith('gate_up_proj_bias'):
                w = 0.25 * rng.standard_normal(p.shape)
            elif name.endswith('bias'):
                w = 0.1 * rng.standard_normal(p.shape)
            elif name.endswith('embed_tokens.weight'):
                w = 0.5 * rng.standard_normal(p.shape)
            elif name.endswith('router.weight'):
                w = 0.2 * rng.standard_normal(p.shape)
            else:       # q / k / v / o projections, lm_head: [out, in]
                w = rng.standard_normal(p.shape) / math.sqrt(p.shape[-1])
            p.copy_(torch.from_numpy(np.asarray(w, f32)).bfloat16().float())
    return model, images


def write_save_pretrained(model, path: str):
    """the unquantised form: transformers' own writer on a bf16 copy (lossless: every parameter is a bf16 value)"""
    import copy

    import torch
    copy.deepcopy(model).to(torch.bfloat16).save_pretrained(path, safe_serialization=True)


def write_published(model, images: dict, path: str):
    """the published layout: experts as `*_blocks` uint8 [E, N, K/32, 16] / `*_scales` uint8 [E, N, K/32] (+ `*_bias`), bf16
    elsewhere, config.json in the older `rope_scaling` + `rope_theta` spelling with quantization_config.quant_method = mxfp4"""
    import torch
    from safetensors.torch import save_file
    tensors = {}
    for name, p in model.named_parameters():
        if name in images:
            b, s = images[name]
            tensors[name + '_blocks'] = torch.from_numpy(np.ascontiguousarray(b.reshape(*b.shape[:2], -1, 16)))
            tensors[name + '_scales'] = torch.from_numpy(np.ascontiguousarray(s))
        else:
            tensors[name] = p.detach().to(torch.bfloat16).contiguous()
    os.makedirs(path, exist_ok=True)
    save_file(tensors, os.path.join(path, 'model.safetensors'))
    c = {k: v for k, v in TOY.items() if k != 'rope_parameters'}
    rp = dict(TOY['rope_parameters'])
    c.update(architectures=['GptOssForCausalLM'], model_type='gpt_oss', torch_dtype='bfloat16', rope_theta=rp.pop('rope_theta'),
             rope_scaling=rp, swiglu_limit=7.0, quantization_config=dict(quant_method='mxfp4', modules_to_not_convert=[]))
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)


def hf_logits(model, ids) -> np.ndarray:
    """fp32 logits [len(ids), V] of one sequence"""
    import torch
    with torch.no_grad():
        return model(torch.tensor([list(ids)]), use_cache=False).logits[0].float().numpy()


# ---- engine slots -> the reference's weights --------------------------------------------------------------------------------------
def yarn_table(rope, rows: int) -> np.ndarray:
    """checkpoint.RopeConfig (yarn, gpt-oss form) -> packed fp16 table through the library's own host builder"""
    import ctypes

    from lmdeploy_amd import _ffi
    p = _ffi.RopeParam(dim=rope.dim, base=rope.base, type=3, factor=rope.factor, low_freq_factor=1.0, high_freq_factor=4.0,
                       original_max_position=0, max_position_embeddings=rope.max_position_embeddings, yarn_beta_fast=rope.beta_fast,
                       yarn_beta_slow=rope.beta_slow, yarn_attention_factor=rope.attention_factor, yarn_truncate=int(rope.truncate))
    tab = np.zeros((rows, rope.dim // 2, 2), f16)
    _ffi.check(_ffi.load().tm_rope_table_ex(tab.ctypes.data, rows, ctypes.byref(p)))
    return tab


def weights_from_slots(slots: dict, mc) -> dict:
    """the engine's slots of a gpt-oss model (checkpoint.ModelConfig mc) -> this module's weights at width mc.hidden / mc.inter:
    every pad is cut off, after a check that it holds what pad_model_weights promises"""
    Hm, Im = mc.hidden, mc.inter

    def cut(a, *n):
        a = np.asarray(a)
        keep = tuple(slice(0, k) for k in n)
        rest = a.copy()
        rest[keep] = 0
        assert not rest.view(np.uint8 if a.dtype == np.uint8 else a.dtype).any(), 'a pad holds something other than +0'
        return np.ascontiguousarray(a[keep])

    def expert(q):
        if q + '.w1w3.blocks' in slots:
            w13 = cut(MX.dequant(slots[q + '.w1w3.blocks'], slots[q + '.w1w3.scales']), Hm, 2 * Im)
            w2 = cut(MX.dequant(slots[q + '.w2.blocks'], slots[q + '.w2.scales']), Im, Hm)
        else:
            w13, w2 = cut(slots[q + '.w1w3.weight'], Hm, 2 * Im), cut(slots[q + '.w2.weight'], Im, Hm)
        return dict(w13=w13, w2=w2, b13=cut(slots[q + '.w1w3.bias'], 2 * Im), b2=cut(slots[q + '.w2.bias'], Hm))

    layers = []
    for li in range(mc.layers):
        p = f'layers.{li}'
        nq = slots[p + '.attention.w_qkv.weight'].shape[1]
        layers.append(dict(
            attn_norm=cut(slots[p + '.attention_norm.weight'], Hm), ffn_norm=cut(slots[p + '.ffn_norm.weight'], Hm),
            w_qkv=dict(w=cut(slots[p + '.attention.w_qkv.weight'], Hm, nq)), qkv_bias=slots[p + '.attention.w_qkv.bias'],
            wo=dict(w=cut(slots[p + '.attention.wo.weight'], slots[p + '.attention.wo.weight'].shape[0], Hm)),
            wo_bias=cut(slots[p + '.attention.wo.bias'], Hm), sinks=slots[p + '.attention.sinks'],
            moe_gate=cut(slots[p + '.moe_ffn.gate.weight'], Hm, mc.moe_experts), moe_gate_bias=slots[p + '.moe_ffn.gate.bias'],
            experts=[expert(f'{p}.moe_ffn.experts.{x}') for x in range(mc.moe_experts)]))
    return dict(tok_embeddings=cut(slots['tok_embeddings.weight'], mc.vocab, Hm), layers=layers, norm=cut(slots['norm.weight'], Hm),
                output=cut(slots['output.weight'], Hm, mc.vocab))


def oracle_config(mc, kv_bits: int, rows: int) -> GptOssConfig:
    return GptOssConfig(hidden=mc.hidden, layers=mc.layers, q_heads=mc.q_heads, kv_heads=mc.kv_heads, head_dim=mc.head_dim,
                        inter=mc.inter, vocab=mc.vocab, rms_eps=mc.rms_eps, rope=o.RopeParam(mc.head_dim, mc.rope.base),
                        kv_bits=kv_bits, weight_format='f16', moe_experts=mc.moe_experts, moe_top_k=mc.moe_top_k, moe_norm_topk=True,
                        layer_windows=tuple(mc.layer_windows), attn_sinks=1, moe_expert_format=mc.moe_expert_format,
                        rope_table=yarn_table(mc.rope, rows))


MUTATIONS = ('gate_up', 'no_o_bias', 'no_qkv_bias', 'no_sinks', 'no_window', 'no_router_bias')


class GptOssOracleModel(AW.WindowOracleModel):
    """the whole model; `mut` (one of MUTATIONS) breaks one thing, for the tests that show the comparison notices"""

    def forward(self, ids_per_seq, decode_splits=1, mut=None):
        cfg = self.cfg
        D, Hq, Hkv = cfg.head_dim, cfg.q_heads, cfg.kv_heads
        tab = cfg.rope_table
        lens = [len(t) for t in ids_per_seq]
        ids = np.concatenate([np.asarray(t, np.int64) for t in ids_per_seq])
        offs = np.concatenate([[0], np.cumsum(lens)])
        resid = o.embedding_lookup(self.w['tok_embeddings'], ids)
        x = o.rmsnorm(resid, self.w['layers'][0]['attn_norm'], cfg.rms_eps)
        for li, Lw in enumerate(self.w['layers']):
            W = 0 if mut == 'no_window' else self.layer_window(li)
            sinks = None if mut == 'no_sinks' else Lw['sinks']
            pro = {} if mut == 'no_qkv_bias' else Lw
            qkv = o._linear(x, Lw['w_qkv'], cfg.group)
            attn = np.zeros((len(ids), Hq * D), f16)
            for b, n in enumerate(lens):
                if n == 0:
                    continue
                sl = slice(offs[b], offs[b + 1])
                hist = self.seq_len[b]
                pos = np.arange(hist, hist + n)
                cos, sin = tab[pos, :, 0], tab[pos, :, 1]
                q, k, v = prologue(qkv[sl, :Hq * D].reshape(n, Hq, D), qkv[sl, Hq * D:(Hq + Hkv) * D].reshape(n, Hkv, D),
                                   qkv[sl, (Hq + Hkv) * D:].reshape(n, Hkv, D), pro, cfg.rms_eps)
                q = o.rope_apply(q, cos, sin)
                o.process_kv(self.cache, self.tables[b], li, k, v, cos, sin, hist)
                if n == 1:
                    kv = [self.cache.load_dequant(self.tables[b], li, hd, 0, hist + 1, 'decode') for hd in range(Hkv)]
                    attn[sl] = AW.window_decode(q[0], np.stack([a for a, _ in kv]), np.stack([c for _, c in kv]), W, self.c,
                                                sinks).reshape(1, -1)
                else:
                    Kf, Vf = o.flatten_kv(self.cache, self.tables[b], li, hist + n)
                    attn[sl] = AW.window_prefill(q, Kf, Vf, hist, W, self.c, sinks).reshape(n, -1)
            resid, x = o.residual_rmsnorm(resid, o._linear(attn, Lw['wo'], cfg.group), Lw['ffn_norm'], cfg.rms_eps,
                                          None if mut == 'no_o_bias' else Lw['wo_bias'])
            d, _, _ = MX.block_forward(x, Lw['moe_gate'], Lw['moe_gate_bias'], Lw['experts'], cfg.moe_top_k, True, 1.0,
                                       mut=mut if mut in ('gate_up', 'no_router_bias') else None)
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        self.last_resid = resid
        self.all_logits = o.lm_head(x, self.w['output'])        # every row (the transformers comparison reads all 20)
        last = np.array([offs[b + 1] - 1 for b in range(len(lens)) if lens[b] > 0])
        logits = self.all_logits[last]
        for b, n in enumerate(lens):
            self.seq_len[b] += n
        return o.greedy(logits), logits


def load_through_reader(path: str):
    """read_config + load_hf_weights + export_weights -> (checkpoint.ModelConfig, slots)"""
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.loader import export_weights
    mc = checkpoint.read_config(path)
    return mc, export_weights(mc, checkpoint.load_hf_weights(path, mc))


_TOYS = {}


def toy(seed: int = 0):
    """the toy of `seed`, built and written once per process -> dict(model, images, save_pretrained=dir, published=dir)"""
    if seed not in _TOYS:
        import atexit
        import shutil
        import tempfile
        root = tempfile.mkdtemp(prefix='gpt_oss_toy_')
        atexit.register(shutil.rmtree, root, ignore_errors=True)
        model, images = build_toy(seed)
        t = dict(model=model, images=images, save_pretrained=os.path.join(root, 'save_pretrained'),
                 published=os.path.join(root, 'published'))
        write_save_pretrained(model, t['save_pretrained'])
        write_published(model, images, t['published'])
        _TOYS[seed] = t
    return _TOYS[seed]
