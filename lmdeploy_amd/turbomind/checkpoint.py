"""HF checkpoint -> logical TM-layout weights (the on-disk side of the boundary).

Host-side mirror of the reference loader for Llama / InternLM2 / Mixtral / Qwen2 / Qwen3 / Qwen2-MoE / Qwen3-MoE with W4A16 weights (AWQ
g128; GPTQ g128, symmetric, no act-order; compressed-tensors `pack-quantized` g128 or -- dense models -- g32: the W4 table below),
FP8 (e4m3: 128x128 block scales, `.weight_scale_inv`; or one scale per tensor / per output channel, `.weight_scale` -- AutoFP8
`quant_method: "fp8"` without weight_block_size and compressed-tensors `float-quantized`; their static `input_scale` / `k_scale` /
`v_scale` tensors are read past: activations are quantised per token, the KV cache follows quant_policy), INT8 W8A8 (int8 codes with
one scale per tensor / output channel: `quant_method: "smooth_quant"` with `.scale`, compressed-tensors `int-quantized` with
`.weight_scale`; dense models; the INT8 table below) or fp16 / bf16 weights
(dense linears and MoE experts alike), and for gpt-oss
(GptOssForCausalLM: MXFP4 experts as published, or the bf16 experts transformers' save_pretrained writes; served zero-padded):
  * source models                    lmdeploy/turbomind/models/llama.py:45-101, internlm2.py:34-87, mixtral.py:57-106,
                                     qwen2.py, qwen3.py (q/k/v bias; per-head q/k norm, reordered like one head;
                                     Qwen3-MoE: mlp.gate router + mlp.experts.X.{gate,up,down}_proj, qwen3.py:110-121;
                                     Qwen2-MoE adds mlp.shared_expert.* and mlp.shared_expert_gate, qwen2.py:110-128)
  * FP8 normalize / dequant          lmdeploy/turbomind/weight_format.py:349-384 (HF [out, in] -> [in, out], scales alike)
  * AWQ normalize (unpack order)     lmdeploy/turbomind/weight_format.py:200-234
  * GPTQ / compressed-tensors        lmdeploy/turbomind/weight_format.py:250-346 (sequential nibbles; zeros + 1; [N, K/8] -> [K, N])
  * RoPE q/k channel permutation     lmdeploy/turbomind/models/utils.py:306-373 (weight, scales and zeros alike)
  * QKV fusion / w1w3 interleave     lmdeploy/turbomind/builders/attention.py:65-108, ffn.py:31-65,138-170
  * config -> engine model config    lmdeploy/turbomind/converter.py:154-259
HF linears are [out, in]; TM layout is [in, out] (= AWQ's native [K, N/8] packing for quantised tensors).
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, field
from glob import glob

import numpy as np

from .loader import (interleave_gate_up, pad_model_weights, permute_qk_for_interleaved_rope, unpack_awq_gemm, unpack_u4_cols,
                     unpack_u4_rows)


@dataclass
class RopeConfig:
    dim: int = 128
    base: float = 10000.0
    type: str = 'default'
    factor: float = 1.0
    low_freq_factor: float = 1.0
    high_freq_factor: float = 4.0
    original_max_position_embeddings: int = 8192
    # yarn: the length the correction range is taken over; dynamic: prompts longer than this take a base of their own.  Both hold
    # the MODEL's max_position_embeddings (what the reference's copy_rope_config hands to the engine, also for yarn checkpoints that
    # carry original_max_position_embeddings: that key only sets the factor)
    max_position_embeddings: int = 0
    beta_fast: float = 32.0
    beta_slow: float = 1.0
    attention_factor: float = 1.0
    # yarn: True = the correction range is rounded outwards (the reference; transformers' default), False = it stays fractional
    # (transformers' `truncate: false`: gpt-oss)
    truncate: bool = True


@dataclass
class ModelConfig:
    hidden: int
    layers: int
    q_heads: int
    kv_heads: int
    head_dim: int
    inter: int
    vocab: int
    rms_eps: float = 1e-5
    rope: RopeConfig = field(default_factory=RopeConfig)
    group: int = 128
    arch: str = 'llama'
    quantized: bool = True
    weight_format: str = 'u4'          # 'u4' (AWQ) | 'fp8' (block 128x128, or one scale per channel: fp8_scale_mode) | 'f16' | 'mxfp4' (W4A4)
                                       # | 'int8' (W8A8: one scale per output channel, activations per token)
    fp8_scale_mode: int = 0            # weight_format 'fp8': 0 = 128x128 block scales, 1 = channel (per-tensor / per-channel checkpoints)
    moe_experts: int = 0               # Mixtral: num_local_experts
    moe_top_k: int = 0                 # num_experts_per_tok
    moe_norm_topk: bool = True
    moe_routed_scale: float = 1.0
    eos_token_id: int | list | None = None
    max_position_embeddings: int = 8192
    attn_bias: int = 0                 # Qwen2 (and Qwen3 with attention_bias): q / k / v projections carry a bias
    qk_norm: int = 0                   # Qwen3: per-head RMSNorm of q and k before RoPE
    moe_shared_inter: int = 0          # Qwen2-MoE: width of the shared expert (a dense FFN behind a sigmoid gate in every MoE layer)
    tie_word_embeddings: bool = False
    window: int = 0                    # Mistral / Mixtral `sliding_window`: a query sees the last `window` keys (0 = all)
    moe_expert_format: int = 0         # 0: the experts follow weight_format; 3: MXFP4 experts (gpt-oss) next to fp16 / u4 attention
    moe_act: int = 0                   # 0: silu(gate) * up; 1: gpt-oss, clamped gate * sigmoid(1.702 gate) * (1 + up)
    moe_bias: int = 0                  # gpt-oss: router bias [E] and per-expert biases on w1w3 / w2
    attn_out_bias: int = 0             # gpt-oss: the o projection carries a bias
    attn_sinks: int = 0                # gpt-oss: one sink logit per q head joins every softmax
    layer_windows: list | None = None  # gpt-oss: one sliding window per layer (0 = full attention), from `layer_types`
    w4_dialect: str = 'awq'            # weight_format 'u4': how the checkpoint packs its 4-bit linears: 'awq' | 'gptq' | 'compressed-tensors'
    w4_zero_offset: int = 1            # GPTQ: what is added to a stored qzeros nibble (1: the v1 form; 0: gptq_v2)
    mrope_section: tuple | None = None  # Qwen2-VL / Qwen2.5-VL: frequency pairs rotated by the t / h / w coordinate (sum = head_dim / 2)

    @property
    def group_size(self) -> int:
        """the u4 quantisation group along K: 128, or 32 (compressed-tensors pack-quantized; dense models, a kernel of its own)"""
        return self.group


def check_kv_quant_policy(cfg, quant_policy: int, tp: int = 1, what: str = 'this model'):
    """quant_policy 42 (TurboQuant KV cache: a 128-wide Hadamard rotation per row, decode attention in the rotated domain) serves
    head_dim 128 with full attention on one rank; NotImplementedError with the reason for anything else.  Every other policy passes."""
    if int(quant_policy) != 42:
        return
    if cfg.head_dim != 128:
        raise NotImplementedError(f'quant_policy=42 (TurboQuant KV) with {what} of head_dim {cfg.head_dim}: the rotation and its '
                                  f'kernels are built for head_dim 128')
    windows = [int(w) for w in (getattr(cfg, 'layer_windows', None) or [])]
    if int(getattr(cfg, 'window', 0) or 0) > 0 or any(w > 0 for w in windows) or getattr(cfg, 'attn_sinks', 0):
        raise NotImplementedError(f'quant_policy=42 (TurboQuant KV) with {what}, which has a sliding window or attention sinks: '
                                  f'the TurboQuant decode attention serves full attention only')
    if tp > 1:
        raise NotImplementedError('quant_policy=42 (TurboQuant KV) with tp > 1: built for tp = 1')


def check_speculative(cfg, quant_policy: int, tp: int = 1, what: str = 'this model'):
    """Speculative decoding (prompt lookup) serves full-attention text models on one rank with quant_policy 0 / 4 / 8;
    NotImplementedError with the reason for anything else -- before any GPU work, like check_kv_quant_policy."""
    if tp > 1:
        raise NotImplementedError('speculative decoding with tp > 1 is not built')
    if int(quant_policy) == 42:
        raise NotImplementedError('speculative decoding with quant_policy=42 (TurboQuant KV) is not built')
    windows = [int(w) for w in (getattr(cfg, 'layer_windows', None) or [])]
    if int(getattr(cfg, 'window', 0) or 0) > 0 or any(w > 0 for w in windows) or getattr(cfg, 'attn_sinks', 0):
        raise NotImplementedError(f'speculative decoding with {what}, which has a sliding window or attention sinks, is not built: the '
                                  f'verify attention serves full attention only')
    if getattr(cfg, 'mrope_section', None):
        raise NotImplementedError(f'speculative decoding with {what}, which has M-RoPE sections (a multimodal model), is not built')


# Qwen decoders: the Llama layout plus the attention prologue.  Exact names: Qwen3-MoE (the Qwen3 prologue with a routed expert FFN
# in every layer) and Qwen2-MoE (the Qwen2 prologue; routed experts plus a shared expert behind a sigmoid gate in every layer)
QWEN_ARCHS = ('Qwen2ForCausalLM', 'Qwen3ForCausalLM', 'Qwen3MoeForCausalLM', 'Qwen2MoeForCausalLM')
QWEN2_ARCHS = ('Qwen2ForCausalLM', 'Qwen2MoeForCausalLM')
QWEN3_MOE_KEYS = ('num_experts', 'num_experts_per_tok', 'moe_intermediate_size')
QWEN2_MOE_KEYS = QWEN3_MOE_KEYS + ('shared_expert_intermediate_size',)

# Everything the reader knows about how a Qwen2-VL / Qwen2.5-VL checkpoint is laid out, in one place.  The language model is a Qwen2
# decoder (the Qwen2 reader, every weight format it serves); the vision tower stays with PyTorch (lmdeploy_amd/vl.py) and its tensors
# are never read here.  The nested form -- language config under `text_config`, weights under `model.language_model.` -- is what the
# installed transformers writes and is tested against it.  The published form (Qwen/Qwen2-VL-*: language config at the top level of
# config.json, weights under `model.` with `visual.*` next to them) was written down from memory of those checkpoints and could not be
# checked against one: a correction is one edit here.
QWEN_VL = dict(
    archs=('Qwen2VLForConditionalGeneration', 'Qwen2_5_VLForConditionalGeneration'),
    refused_prefixes=('Qwen3VL',),                            # interleaved M-RoPE and deep-stack features: not built
    text_config='text_config',                                # nested language config (absent: the top level holds it)
    language_prefixes=('model.language_model.', 'model.'),    # tried in this order; `<prefix>embed_tokens.weight` decides
    vision_prefixes=('model.visual.', 'visual.'),             # skipped
    rope_keys=('rope_parameters', 'rope_scaling'),            # transformers 5 / 4
    rope_types=('default', 'mrope', None),
    section='mrope_section',
)


def _qwen_vl_language_config(arch: str, c: dict) -> dict:
    """config.json of a Qwen2-VL / Qwen2.5-VL checkpoint -> the config of its language model in the Qwen2 reader's terms (plus
    `mrope_section`), or NotImplementedError naming what is not served"""
    V = QWEN_VL
    text = dict(c.get(V['text_config']) or {})
    lc = dict(c, **text)                      # nested keys win; the published form has everything at the top level
    for k in (V['text_config'], 'vision_config'):
        lc.pop(k, None)
    rp = None
    for key in V['rope_keys']:
        rp = text.get(key) or c.get(key)
        if rp:
            break
    if not isinstance(rp, dict) or V['section'] not in rp:
        raise NotImplementedError(f'{arch}: config.json lacks {V["section"]} (under {" / ".join(V["rope_keys"])})')
    t = rp.get('rope_type', rp.get('type'))
    if t not in V['rope_types']:
        raise NotImplementedError(f'{arch} with rope type {t}: M-RoPE is built for the default frequencies only (yarn / dynamic are not)')
    D = lc.get('head_dim') or lc['hidden_size'] // lc['num_attention_heads']
    if D != 128:
        raise NotImplementedError(f'{arch} with head_dim {D}: M-RoPE is built for head_dim 128')
    sec = rp[V['section']]
    ok = isinstance(sec, (list, tuple)) and len(sec) == 3 and all(isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in sec)
    if not ok or sum(sec) != D // 2:
        raise NotImplementedError(f'{arch} with mrope_section {sec!r}: three non-negative integers that sum to head_dim / 2 = {D // 2} '
                                  f'are required')
    if 'rope_theta' in rp:
        lc['rope_theta'] = rp['rope_theta']
    lc.pop('rope_scaling', None)              # the frequencies are the default ones: nothing left for the RoPE-scaling branch
    lc.pop('rope_parameters', None)
    lc['architectures'] = ['Qwen2ForCausalLM']
    lc['mrope_section'] = tuple(int(v) for v in sec)
    return lc


def _qwen3_moe_fields(arch: str, c: dict, quantized: bool, keys: tuple = QWEN3_MOE_KEYS) -> dict:
    """the MoE fields of a Qwen3MoeForCausalLM (or, with QWEN2_MOE_KEYS, Qwen2MoeForCausalLM) config, or NotImplementedError with the
    reason.  The geometry keys must be in config.json: a library default would describe some other checkpoint."""
    missing = [k for k in keys if c.get(k) is None]
    if missing:
        raise NotImplementedError(f'{arch}: config.json lacks {", ".join(missing)}')
    E, k = int(c['num_experts']), int(c['num_experts_per_tok'])
    if c.get('mlp_only_layers'):
        raise NotImplementedError(f'{arch} with mlp_only_layers {c["mlp_only_layers"]}: dense layers among the sparse ones are not '
                                  f'implemented (the MoE switch is model-wide)')
    if int(c.get('decoder_sparse_step', 1)) != 1:
        raise NotImplementedError(f'{arch} with decoder_sparse_step {c["decoder_sparse_step"]}: every layer must be sparse (the MoE '
                                  f'switch is model-wide)')
    if not 1 <= E <= 256 or not 1 <= k <= 8 or k > E:
        raise NotImplementedError(f'{arch} with num_experts {E}, num_experts_per_tok {k}: the router serves up to 256 experts, top-8')
    if not quantized:
        # unquantised experts run as fp16 (a bf16 tensor is narrowed like the dense linears).  The config must say that the checkpoint is
        # fp16 / bf16 -- as every published one does (`torch_dtype`, `dtype` in newer exports): a config.json with neither a
        # quantization_config nor a 16-bit dtype describes float32 experts, or a quantised export whose quantization_config was lost
        dt = str(c.get('torch_dtype', c.get('dtype'))).replace('torch.', '')
        if dt not in ('float16', 'bfloat16'):
            raise NotImplementedError(f'{arch} without a quantization_config and with torch_dtype {dt}: unquantised experts are served '
                                      f'from float16 / bfloat16 checkpoints (config.json must say so); quantised experts need their '
                                      f'quantization_config (AWQ or block-128 FP8)')
    shared = int(c['shared_expert_intermediate_size']) if 'shared_expert_intermediate_size' in keys else 0
    if shared < 0 or shared % 128:
        raise NotImplementedError(f'{arch} with shared_expert_intermediate_size {shared}: the shared expert\'s width must be a '
                                  f'multiple of 128')
    return dict(inter=int(c['moe_intermediate_size']), moe_experts=E, moe_top_k=k,
                moe_norm_topk=bool(c.get('norm_topk_prob', False)), moe_routed_scale=1.0, moe_shared_inter=shared)


def _yarn_mscale(scale: float, mscale: float = 1.0) -> float:
    return 1.0 if scale <= 1 else 0.1 * mscale * math.log(scale) + 1.0


def _scaled_rope(t: str, rs: dict, D: int, base: float, max_pos: int) -> RopeConfig:
    """rope_scaling `dynamic` / `yarn` of a Llama / InternLM config as the reference parses it (lmdeploy/turbomind/models/utils.py:76-187)"""
    factor = float(rs.get('factor', 0.0))
    if t == 'dynamic':
        return RopeConfig(D, base, 'dynamic', factor, max_position_embeddings=max_pos)
    af = rs.get('attention_factor')
    if af is None:
        ms, ms_all = rs.get('mscale'), rs.get('mscale_all_dim')
        af = _yarn_mscale(factor, ms) / _yarn_mscale(factor, ms_all) if ms is not None and ms_all is not None else _yarn_mscale(factor)
    if 'original_max_position_embeddings' in rs:
        factor = max_pos / rs['original_max_position_embeddings']
    return RopeConfig(D, base, 'yarn', float(factor), max_position_embeddings=max_pos, beta_fast=float(rs.get('beta_fast', 32.0)),
                      beta_slow=float(rs.get('beta_slow', 1.0)), attention_factor=float(af))


def _merged_eos(c: dict, model_path: str):
    """eos ids: config.json + generation_config.json (GenerationConfig.update_from_hf_gen_cfg, lmdeploy/messages.py:176-199)"""
    eos = c.get('eos_token_id')
    gpath = os.path.join(model_path, 'generation_config.json')
    if os.path.exists(gpath):
        with open(gpath) as f:
            ge = json.load(f).get('eos_token_id')
        if ge is not None:
            merged = list(eos if isinstance(eos, (list, tuple)) else ([] if eos is None else [eos]))
            merged += [t for t in (ge if isinstance(ge, (list, tuple)) else [ge]) if t not in merged]
            eos = merged if len(merged) > 1 else merged[0]
    return eos


def _read_gpt_oss(arch: str, c: dict, model_path: str, tp: int) -> ModelConfig:
    """GptOssForCausalLM (transformers/models/gpt_oss): head_dim 64 attention with q / k / v / o biases and sinks, sliding and full
    layers alternating as `layer_types` says, YaRN with a fractional correction range, an MoE block with MXFP4 (published) or bf16
    (save_pretrained) experts, router and expert biases and the clamped activation.  hidden_size / intermediate_size that are no
    multiple of 128 (2880) stay as published here: the loader pads the tensors and make_model_config hands the engine the padded
    sizes."""
    H = c.get('hidden_size')
    rs = c.get('rope_parameters') or c.get('rope_scaling')
    have = dict(c, rope_settings=rs if rs and (c.get('rope_parameters') or c.get('rope_theta') is not None) else None)
    missing = [k for k in ('layer_types', 'sliding_window', 'rope_settings') if have.get(k) is None]
    if missing:
        names = ', '.join('rope_scaling + rope_theta (or rope_parameters)' if k == 'rope_settings' else k for k in missing)
        raise NotImplementedError(f'{arch}: config.json lacks {names} -- which layers slide, over how many tokens and under which RoPE '
                                  f'cannot be known without them (a library default would describe some other checkpoint).  '
                                  f'hidden_size {H} (% 128 != 0 for gpt-oss: 2880 = 22.5 x 128) is served zero-padded to the next '
                                  f'multiple of 128 and the o_proj bias is loaded, for a complete config only')
    if tp > 1:
        raise NotImplementedError(f'{arch} with tp = {tp}: the zero-padded norm, the o_proj bias and the MXFP4 experts are built for '
                                  f'tp = 1 only')
    q = c.get('quantization_config')
    if q is not None and q.get('quant_method') != 'mxfp4':
        raise NotImplementedError(f'{arch} with quantization_config {q}: the experts are served as MXFP4 (quant_method "mxfp4", the '
                                  f'published form) or unquantised (no quantization_config)')
    if float(c.get('swiglu_limit', 7.0)) != 7.0:
        raise NotImplementedError(f'{arch} with swiglu_limit {c["swiglu_limit"]}: the expert activation clamps at 7')
    if q is None:
        dt = str(c.get('torch_dtype', c.get('dtype'))).replace('torch.', '')
        if dt not in ('float16', 'bfloat16'):
            raise NotImplementedError(f'{arch} without a quantization_config and with torch_dtype {dt}: unquantised experts are served '
                                      f'from float16 / bfloat16 checkpoints (config.json must say so)')
    if not c.get('attention_bias', True):
        raise NotImplementedError(f'{arch} with attention_bias false: the reader loads the q / k / v / o biases of every layer')
    heads, layers = c['num_attention_heads'], c['num_hidden_layers']
    D = c.get('head_dim') or H // heads
    if D not in (64, 128) or heads * D % 128:
        raise NotImplementedError(f'{arch} with {heads} attention heads of head_dim {D}: head_dim must be 64 or 128 and '
                                  f'num_attention_heads * head_dim a multiple of 128')
    E, k = int(c.get('num_local_experts') or 0), int(c.get('num_experts_per_tok') or 0)
    if not 1 <= E <= 256 or not 1 <= k <= 8 or k > E:
        raise NotImplementedError(f'{arch} with num_local_experts {E}, num_experts_per_tok {k}: the router serves up to 256 experts, top-8')
    types, sw = list(c['layer_types']), c['sliding_window']
    if len(types) != layers or any(t not in ('sliding_attention', 'full_attention') for t in types):
        raise NotImplementedError(f'{arch}: layer_types {types} must name sliding_attention or full_attention for each of the {layers} layers')
    if isinstance(sw, bool) or not isinstance(sw, int) or sw <= 0:
        raise ValueError(f'{arch}: sliding_window {sw!r} must be a positive integer')
    base = rs.get('rope_theta', c.get('rope_theta'))
    if base is None:
        raise NotImplementedError(f'{arch}: config.json lacks rope_theta')
    max_pos = int(c.get('max_position_embeddings', 0))
    t = rs.get('rope_type', rs.get('type'))
    if t == 'yarn':
        if 'original_max_position_embeddings' not in rs or max_pos <= 0:
            raise NotImplementedError(f'{arch}: YaRN needs original_max_position_embeddings and max_position_embeddings')
        # factor and attention factor as for Llama / InternLM; the correction range is taken over the ORIGINAL length and left
        # fractional under `truncate: false`, as transformers computes it (the reference's parse does neither)
        rope = _scaled_rope('yarn', rs, D, float(base), max_pos)
        rope.max_position_embeddings = int(rs['original_max_position_embeddings'])
        rope.truncate = bool(rs.get('truncate', True))
    elif t in (None, 'default'):
        rope = RopeConfig(dim=D, base=float(base))
    else:
        raise NotImplementedError(f'{arch}: rope type {t}')
    return ModelConfig(hidden=H, layers=layers, q_heads=heads, kv_heads=c.get('num_key_value_heads', heads), head_dim=D,
                       inter=c['intermediate_size'], vocab=c['vocab_size'], rms_eps=float(c.get('rms_norm_eps', 1e-5)), rope=rope,
                       arch='gpt_oss', quantized=False, weight_format='f16', moe_experts=E, moe_top_k=k, moe_norm_topk=True,
                       eos_token_id=_merged_eos(c, model_path), max_position_embeddings=max_pos or 8192, attn_bias=1, attn_out_bias=1,
                       attn_sinks=1, layer_windows=[int(sw) if t_ == 'sliding_attention' else 0 for t_ in types],
                       moe_expert_format=3 if q is not None else 0, moe_act=1, moe_bias=1,
                       tie_word_embeddings=bool(c.get('tie_word_embeddings', False)))


# router gates a compressed-tensors `ignore` list may name next to lm_head (they are read as fp16 anyway)
_CT_IGNORE_OK = ('lm_head', 're:.*lm_head', 're:.*block_sparse_moe.gate', 're:.*mlp.gate$', 're:.*mlp.shared_expert_gate$')


# The two INT8 W8A8 dialects (int8 weights with one scale per tensor / output channel, int8 activations quantised per token), every key
# and accepted value in one place.  smooth_quant is what `lmdeploy lite smooth_quant` writes (lite/apis/smooth_quant.py:121-126, tensors
# as pytorch/models/q_modules.py:97-98 declares them).  The compressed-tensors names (llm-compressor's *-quantized.w8a8 exports) were
# written down from memory and could not be checked against a published checkpoint, like the QUARK table: a correction is one edit here.
INT8 = {
    'smooth_quant': dict(
        dtype_key='quant_dtype', dtype='int8',           # float8_e4m3fn / float8_e5m2 (the reference's fp8 smooth-quant) are refused by name
        skip_key='modules_to_not_convert', skip_ok=('lm_head',),
        scale_suffix='.scale',                           # fp32 [out, 1] next to .weight int8 [out][in]
    ),
    'compressed-tensors': dict(
        format='int-quantized',
        weights=(('num_bits', (8,)), ('type', ('int',)), ('symmetric', (True,)), ('strategy', ('tensor', 'channel'))),
        input_activations=(('num_bits', (8,)), ('type', ('int',)), ('symmetric', (True, None)), ('strategy', ('token', 'tensor'))),
        scale_suffix='.weight_scale',                    # any float dtype, [out, 1] / [out] / [] / [1], next to .weight int8 [out][in]
    ),
}
# what `format` of a compressed-tensors config selects: the element type both sides must name, and whether activations may be absent
_CT_FORMATS = {
    'float-quantized': dict(weights=(('num_bits', (8,)), ('type', ('float',)), ('symmetric', (True,)), ('strategy', ('tensor', 'channel'))),
                            input_activations=(('num_bits', (8,)), ('type', ('float',)), ('strategy', ('token', 'tensor'))),
                            weight_only_ok=True, codes='e4m3'),
    'int-quantized': dict(weights=INT8['compressed-tensors']['weights'], input_activations=INT8['compressed-tensors']['input_activations'],
                          weight_only_ok=False, codes='int8'),
}


# The two further W4A16 dialects next to AWQ (u4 codes [K,N], fp16 scales [K/g,N], zeros [K/g,N] once read), every key and accepted value in
# one place.  GPTQ: the config keys are those of transformers' GPTQConfig (bits, group_size, sym, desc_act; `checkpoint_format` in
# AutoGPTQ / older transformers, `format` in newer ones, "gptq_v2" = zeros stored without the -1), checked against the installed
# transformers by tests/test_host_w4_formats.py; the tensor names and layouts are the reference's reader (GPTQFormat,
# lmdeploy/turbomind/weight_format.py:250-291).  compressed-tensors: the compressed_tensors package was not available to check
# against, so the names come from the reference's reader (CompressedTensorFormat, weight_format.py:294-346; converter.py:190-201) and
# could not be checked against the library or a published checkpoint: a correction is one edit here.
W4 = {
    'gptq': dict(
        method='gptq',
        config=(('bits', 4, (4,)), ('group_size', 128, (128,)), ('sym', True, (True,)), ('desc_act', False, (False,))),   # key, default, accepted
        v2_keys=('checkpoint_format', 'format'), v2='gptq_v2',
        qweight='.qweight',                              # int32 [K/8][N], nibble i of word r = row 8r+i
        scales='.scales',                                # fp16 [K/g][N]
        qzeros='.qzeros',                                # int32 [K/g][N/8], nibble j of word c = column 8c+j; zero = stored + 1 (v2: + 0)
        g_idx='.g_idx',                                  # int32 [K], must be k // g (anything else is act-order)
    ),
    'compressed-tensors': dict(
        method='compressed-tensors', format='pack-quantized',
        weights=(('strategy', ('group',)), ('group_size', (32, 128)), ('dynamic', (False, None)), ('actorder', (None, False))),
        weight='.weight_packed',                         # int32 [N][K/8], nibble j of word c = input channel 8c+j; the code is the nibble
        scales='.weight_scale',                          # fp16 / bf16 [N][K/g]
        zeros='.weight_zero_point',                      # asymmetric only: int32 [N/8][K/g], nibble i of word r = output channel 8r+i
        shape='.weight_shape',                           # [2] = (N, K)
        symmetric_zero=8,
    ),
}


def _is_moe(arch: str) -> bool:
    return 'Mixtral' in arch or 'Moe' in arch or 'MoE' in arch


def _check_gptq(q: dict) -> int:
    """quantization_config of a GPTQ export (W4['gptq']): the reference's conditions (converter.py:183-185 and the group sizes of
    converter.py:86-92).  Returns the offset of the stored zeros."""
    G = W4['gptq']
    for key, default, ok in G['config']:
        if q.get(key, default) not in ok:
            raise NotImplementedError(f'gptq quantization_config: {key} = {q.get(key)!r} is not served ({" | ".join(map(repr, ok))}'
                                      f'{": act-order permutes the groups along K" if key == "desc_act" else ""})')
    return 0 if any(q.get(k) == G['v2'] for k in G['v2_keys']) else 1


def _check_pack_quantized(q: dict) -> int:
    """quantization_config of a compressed-tensors `pack-quantized` export (W4['compressed-tensors']): ONE config group of 4-bit int
    group weights (group 128 or 32, static, no act-order) without input activations.  Returns the group size.  A pack-quantized config
    that is not 4-bit int weight-only is refused under `format`, as before."""
    C = W4['compressed-tensors']

    def no(key, val, want):
        return NotImplementedError(f'compressed-tensors quantization_config: {key} = {val!r} is not served ({want})')
    groups = q.get('config_groups') or {}
    if len(groups) != 1:
        raise no('config_groups', sorted(groups), 'exactly one config group')
    (gname, g), = groups.items()
    w = g.get('weights') or {}
    if w.get('num_bits') != 4 or w.get('type') != 'int' or g.get('input_activations') is not None \
            or g.get('format', C['format']) != C['format']:
        raise no('format', q.get('format'), '"pack-quantized" holds 4-bit int group weights without input activations (W4A16); 8-bit '
                 'weights come as "float-quantized": e4m3 weights with .weight_scale, or "int-quantized": int8 W8A8')
    for key, ok in C['weights']:
        if w.get(key) not in ok:
            raise no(f'config_groups.{gname}.weights.{key}', w.get(key), ' | '.join('absent' if x is None else repr(x) for x in ok))
    for name in q.get('ignore') or []:
        if name not in _CT_IGNORE_OK and not name.endswith('lm_head'):
            raise no('ignore', name, 'only lm_head and router gates may stay unquantised: every decoder linear is 4-bit')
    return int(w['group_size'])


def _refuse_int8_moe(arch: str, method: str):
    if _is_moe(arch):
        raise NotImplementedError(f'{arch} with quant_method "{method}" (INT8 W8A8): served for dense models only (int8 experts are not '
                                  f'built)')


def _check_compressed_tensors(q: dict) -> str:
    """quantization_config of llm-compressor's 8-bit exports -> 'float-quantized' (FP8: e4m3 weights) or 'int-quantized' (INT8 W8A8, the
    INT8 table): ONE config group, 8-bit symmetric weights of the format's type with a per-tensor or per-channel scale, input activations
    of the same type per token / per tensor (static scales are read past; float: may be absent; int: symmetric).  Anything else is
    refused with the offending key."""
    def no(key, val, want):
        return NotImplementedError(f'compressed-tensors quantization_config: {key} = {val!r} is not served ({want})')
    fmt = _CT_FORMATS.get(q.get('format'))
    if fmt is None:
        raise no('format', q.get('format'), 'only "float-quantized": e4m3 weights with .weight_scale, or "int-quantized": int8 W8A8')
    groups = q.get('config_groups') or {}
    if len(groups) != 1:
        raise no('config_groups', sorted(groups), 'exactly one config group')
    (gname, g), = groups.items()
    w = g.get('weights') or {}
    for key, ok in fmt['weights']:
        if w.get(key) not in ok:
            raise no(f'config_groups.{gname}.weights.{key}', w.get(key), ' | '.join(map(repr, ok)))
    a = g.get('input_activations')
    if a is None and not fmt['weight_only_ok']:
        raise no(f'config_groups.{gname}.input_activations', a, 'int8 weights are served with int8 activations (W8A8) only')
    if a is not None:
        for key, ok in fmt['input_activations']:
            if a.get(key) not in ok:
                raise no(f'config_groups.{gname}.input_activations.{key}', a.get(key), ' | '.join(repr(x) for x in ok if x is not None))
    for name in q.get('ignore') or []:
        if name not in _CT_IGNORE_OK and not name.endswith('lm_head'):
            raise no('ignore', name, f'only lm_head and router gates may stay unquantised: every decoder linear is {fmt["codes"]}')
    return q.get('format')


def _check_smooth_quant(q: dict):
    """quantization_config of `lmdeploy lite smooth_quant` (INT8['smooth_quant']): int8 only, nothing but lm_head left unconverted"""
    S = INT8['smooth_quant']
    if q.get(S['dtype_key'], S['dtype']) != S['dtype']:
        raise NotImplementedError(f'smooth_quant quantization_config: {S["dtype_key"]} = {q.get(S["dtype_key"])!r} is not served (only '
                                  f'"int8": the fp8 smooth-quant form is not built)')
    for name in q.get(S['skip_key']) or []:
        if name not in S['skip_ok']:
            raise NotImplementedError(f'smooth_quant quantization_config: {S["skip_key"]} = {name!r} is not served (only lm_head may stay '
                                      f'unconverted: every decoder linear is int8)')


# Every key of a Quark MXFP4 export this reader depends on, in one place.  The layout was written down from memory of Quark's exports
# and of how other engines read them and could not be checked against a published checkpoint: a correction is one edit here.
QUARK = dict(
    method='quark',                                  # quantization_config.quant_method
    global_cfg='global_quant_config',                # the config every linear follows ...
    layer_cfg='layer_quant_config',                  # ... unless a per-layer entry (glob pattern -> config) changes it
    exclude='exclude',                               # layers left unquantised
    weight='weight', inputs='input_tensors', outputs='output_tensors',
    spec=dict(dtype='fp4', qscheme='per_group', group_size=32, scale_format='e8m0'),   # what weight and input_tensors must say
    dynamic='is_dynamic',                            # False for the weights, True for the input activations
    weight_suffix='.weight',                         # uint8 [out][in / 2], k = 2j in the low nibble
    scale_suffix='.weight_scale',                    # uint8 [out][in / 32], e8m0
    exclude_ok=('lm_head', '*lm_head', 're:.*lm_head'),
    decoder_linears=('q_proj', 'k_proj', 'v_proj', 'o_proj', 'gate_proj', 'up_proj', 'down_proj'),
    kv_outputs=('k_proj', 'v_proj'),                 # layer_quant_config entries that only add output_tensors (KV-cache scales): read past
)


def _check_quark(q: dict, arch: str):
    """quantization_config of an AMD Quark MXFP4 W4A4 export (the QUARK table): fp4 per-group weights (group 32, e8m0 scales, not
    dynamic) and the same for the input activations, dynamic.  Anything else is refused with the offending key."""
    Q = QUARK

    def no(key, val, want):
        return NotImplementedError(f'quark quantization_config: {key} = {val!r} is not served ({want})')
    if _is_moe(arch):
        raise NotImplementedError(f'{arch} with quant_method "quark": MXFP4 W4A4 is served for dense models only (mixture-of-experts '
                                  f'architectures are not built)')
    g = q.get(Q['global_cfg'])
    if not isinstance(g, dict):
        raise no(Q['global_cfg'], g, 'the global MXFP4 config is required')

    def check(where, spec, dynamic):
        if not isinstance(spec, dict):
            raise no(where, spec, 'an fp4 per-group config is required')
        for key, want in Q['spec'].items():
            if spec.get(key) != want:
                raise no(f'{where}.{key}', spec.get(key), repr(want))
        if bool(spec.get(Q['dynamic'], False)) != dynamic:
            raise no(f'{where}.{Q["dynamic"]}', spec.get(Q['dynamic']), repr(dynamic))
    check(f'{Q["global_cfg"]}.{Q["weight"]}', g.get(Q['weight']), False)
    check(f'{Q["global_cfg"]}.{Q["inputs"]}', g.get(Q['inputs']), True)
    # (global output_tensors, KV-cache scales: read past -- the cache follows quant_policy)
    for name in q.get(Q['exclude']) or []:
        if name not in Q['exclude_ok'] and not name.endswith('lm_head'):
            raise no(Q['exclude'], name, 'only lm_head may stay unquantised: every decoder linear is MXFP4')
    for pat, lc in (q.get(Q['layer_cfg']) or {}).items():
        lc = lc or {}
        same = all(lc.get(k) in (None, g.get(k)) for k in (Q['weight'], Q['inputs']))
        if same and pat.rstrip('*').rstrip('.').endswith(Q['kv_outputs']):
            continue                                 # k_proj / v_proj with output_tensors only: KV-cache scales, read past
        if any(n in pat for n in Q['decoder_linears']) or not same:
            raise no(f'{Q["layer_cfg"]}[{pat!r}]', lc, 'a per-layer config that changes a decoder linear is not built')


def read_config(model_path: str, tp: int = 1) -> ModelConfig:
    with open(os.path.join(model_path, 'config.json')) as f:
        c = json.load(f)
    arch = (c.get('architectures') or ['LlamaForCausalLM'])[0]
    if arch == 'GptOssForCausalLM':
        return _read_gpt_oss(arch, c, model_path, tp)
    if arch.startswith(QWEN_VL['refused_prefixes']):
        raise NotImplementedError(f'architecture {arch}: Qwen3-VL (interleaved M-RoPE, deep-stack visual features) is not built; the '
                                  f'vision-language models served are Qwen2-VL and Qwen2.5-VL')
    mrope_section = None
    if arch in QWEN_VL['archs']:
        c = _qwen_vl_language_config(arch, c)
        mrope_section = c['mrope_section']
        if c.get('use_sliding_window'):
            raise NotImplementedError(f'{arch} with use_sliding_window: sliding-window attention is not implemented')
        arch = 'Qwen2ForCausalLM'
    kind = 'internlm2' if 'InternLM2' in arch else 'llama'
    qwen = arch in QWEN_ARCHS
    internlm3 = arch == 'InternLM3ForCausalLM'      # a plain Llama (the reference: supported_models.py) -- without projection biases
    if internlm3 and (c.get('bias') or c.get('qkv_bias')):
        raise NotImplementedError(f'{arch} with bias {c.get("bias")} / qkv_bias {c.get("qkv_bias")}: the Llama reader carries no '
                                  f'projection biases')
    if kind == 'llama' and not qwen and not internlm3 and not any(a in arch for a in ('Llama', 'Mistral', 'Mixtral')):
        raise NotImplementedError(f'architecture {arch}: the MI355X hot path covers Llama / InternLM2 / InternLM3 / Mixtral / Qwen2 / '
                                  f'Qwen3 decoders, Qwen2-MoE and Qwen3-MoE')
    H = c['hidden_size']
    heads = c['num_attention_heads']
    D = c.get('head_dim') or H // heads
    attn_bias = qk_norm = 0
    if qwen:
        kind = 'qwen2' if arch in QWEN2_ARCHS else 'qwen3'
        if c.get('use_sliding_window'):
            raise NotImplementedError(f'{arch} with use_sliding_window: sliding-window attention is not implemented')
        if D != 128:
            raise NotImplementedError(f'{arch} with head_dim {D}: the attention kernels need head_dim 128')
        attn_bias = 1 if kind == 'qwen2' else int(bool(c.get('attention_bias', False)))
        qk_norm = 1 if kind == 'qwen3' else 0
    else:
        # the Llama reader (Llama / Mistral / Mixtral / InternLM): attention and KV-cache kernels exist for head_dim 64 and 128
        if D not in (64, 128):
            raise NotImplementedError(f'{arch} with head_dim {D}: the attention kernels support head_dim 64 and 128')
        if heads * D % 128:
            raise NotImplementedError(f'{arch} with {heads} attention heads of head_dim {D}: num_attention_heads * head_dim = '
                                      f'{heads * D} must be a multiple of 128 (the K dimension of the o projection)')
    window = 0
    if 'Mistral' in arch or 'Mixtral' in arch:      # sliding_window: null, absent or 0 = full attention (Mistral-7B-v0.1: 4096)
        sw = c.get('sliding_window')
        if sw is not None:
            if isinstance(sw, bool) or not isinstance(sw, int) or sw < 0:
                raise ValueError(f'{arch}: sliding_window {sw!r} must be a non-negative integer or null')
            window = sw
    q = c.get('quantization_config')
    wfmt, fp8_mode, w4, group, zero_offset = 'f16', 0, 'awq', 128, 1
    if q is not None:
        if q.get('quant_method') == QUARK['method']:
            _check_quark(q, arch)
            if tp != 1:
                raise NotImplementedError(f'{arch} with quant_method "quark" (MXFP4 W4A4) and tp = {tp}: not built (run with tp = 1)')
            wfmt = 'mxfp4'
        elif q.get('quant_method') == 'compressed-tensors' and q.get('format') == W4['compressed-tensors']['format']:
            wfmt, w4, group = 'u4', 'compressed-tensors', _check_pack_quantized(q)
            if group != 128 and _is_moe(arch):
                raise NotImplementedError(f'{arch} with compressed-tensors weights.group_size = {group}: the group-{group} kernel serves '
                                          f'dense models only (mixture-of-experts models need group_size 128)')
        elif q.get('quant_method') == 'compressed-tensors':
            if _check_compressed_tensors(q) == INT8['compressed-tensors']['format']:
                _refuse_int8_moe(arch, 'compressed-tensors')
                wfmt = 'int8'
            else:
                wfmt, fp8_mode = 'fp8', 1
        elif q.get('quant_method') == 'smooth_quant':
            _check_smooth_quant(q)
            _refuse_int8_moe(arch, 'smooth_quant')
            wfmt = 'int8'
        elif q.get('quant_method') == 'fp8' and q.get('weight_block_size') is None:
            # AutoFP8 / neuralmagic *-FP8: one scale per tensor (`.weight_scale`).  head_dim 64 is fine: no scale block straddles a head
            for name in q.get('ignored_layers') or []:
                if not name.endswith(('lm_head', '.gate')):
                    raise NotImplementedError(f'fp8 quantization_config: ignored_layers = {name!r} is not served (only lm_head and '
                                              f'router gates may stay unquantised: every decoder linear is e4m3)')
            wfmt, fp8_mode = 'fp8', 1
        elif q.get('quant_method') == 'fp8':     # converter.py:186-187; block size fixed at 128 (converter.py:82,90)
            if list(q.get('weight_block_size')) != [128, 128]:
                raise NotImplementedError(f'quantization_config {q}: fp8 needs 128x128 weight blocks (weight_block_size), or none at '
                                          f'all (one scale per tensor)')
            if D == 64:
                raise NotImplementedError(f'{arch} with fp8 weights and head_dim 64: the 128-column scale blocks of the q / k / v '
                                          f'projections straddle heads; fp8 needs head_dim 128')
            wfmt = 'fp8'
        elif q.get('quant_method') == W4['gptq']['method']:
            wfmt, w4, zero_offset = 'u4', 'gptq', _check_gptq(q)
        elif q.get('quant_method') != 'awq' or q.get('bits', 4) != 4 or q.get('group_size', 128) != 128:
            raise NotImplementedError(f'quantization_config {q}: only AWQ 4-bit group 128, GPTQ 4-bit group 128 (symmetric, no '
                                      f'act-order), compressed-tensors pack-quantized 4-bit (group 128 or 32), block-128 FP8, per-tensor '
                                      f'FP8, compressed-tensors float-quantized FP8 (lmdeploy/turbomind/converter.py:82-92), Quark MXFP4 '
                                      f'or INT8 W8A8 (smooth_quant, compressed-tensors int-quantized)')
        else:
            wfmt = 'u4'
    rope = RopeConfig(dim=D, base=float(c.get('rope_theta', 10000.0)))
    rs = c.get('rope_scaling')
    if rs:
        t = rs.get('rope_type', rs.get('type'))
        if t == 'llama3':
            rope = RopeConfig(D, rope.base, 'llama3', float(rs['factor']), float(rs.get('low_freq_factor', 1.0)),
                              float(rs.get('high_freq_factor', 4.0)), int(rs.get('original_max_position_embeddings', 8192)))
        elif t == 'linear':
            rope = RopeConfig(D, rope.base, 'linear', float(rs['factor']))
        elif t in ('dynamic', 'yarn') and not qwen:
            rope = _scaled_rope(t, rs, D, rope.base, int(c.get('max_position_embeddings', 0)))
        elif t not in (None, 'default'):
            raise NotImplementedError(f'rope_scaling type {t}')
    eos = _merged_eos(c, model_path)
    c = dict(c, eos_token_id=eos)
    if arch == 'Qwen3MoeForCausalLM':
        moe = _qwen3_moe_fields(arch, c, q is not None)
    elif arch == 'Qwen2MoeForCausalLM':
        moe = _qwen3_moe_fields(arch, c, q is not None, QWEN2_MOE_KEYS)
    else:
        moe = dict(inter=c['intermediate_size'], moe_experts=int(c.get('num_local_experts', 0) or 0) if 'Mixtral' in arch else 0,
                   moe_top_k=int(c.get('num_experts_per_tok', 0) or 0) if 'Mixtral' in arch else 0)
    return ModelConfig(hidden=H, layers=c['num_hidden_layers'], q_heads=heads,
                       kv_heads=c.get('num_key_value_heads', heads), head_dim=D,
                       vocab=c['vocab_size'], rms_eps=float(c.get('rms_norm_eps', 1e-5)), rope=rope, arch=kind,
                       quantized=q is not None, eos_token_id=c.get('eos_token_id'),
                       max_position_embeddings=int(c.get('max_position_embeddings', 8192)), weight_format=wfmt, fp8_scale_mode=fp8_mode,
                       **moe, group=group, w4_dialect=w4, w4_zero_offset=zero_offset,
                       attn_bias=attn_bias, qk_norm=qk_norm, window=window, tie_word_embeddings=bool(c.get('tie_word_embeddings', False)),
                       mrope_section=mrope_section)


def gpt_oss_expert_slots(tensors: dict, layer: int) -> dict:
    """The MoE block of layer `layer` of a published gpt-oss checkpoint -> this engine's weight slots (a pure function of numpy arrays).
    tensors (names as published, transformers' GptOssExperts under the MXFP4 integration):
      model.layers.{i}.mlp.experts.gate_up_proj_blocks uint8 [E, 2I, H/32, 16]   16 bytes = 32 e2m1 codes, low nibble = even k
      ...gate_up_proj_scales uint8 [E, 2I, H/32]      ...gate_up_proj_bias [E, 2I]     rows (gate_j, up_j)-interleaved, even = gate:
                                                                                        this engine's w1w3 column order as published
      ...down_proj_blocks uint8 [E, H, I/32, 16]      ...down_proj_scales [E, H, I/32] ...down_proj_bias [E, H]
      model.layers.{i}.mlp.router.weight [E, H]       ...router.bias [E]
    Blocks and scales keep their bytes: [N, K/32, 16] is [N, K/2] row-major, the layout tm_moe_set_expert takes."""
    m = f'model.layers.{layer}.mlp'
    gu_b, gu_s, gu_bias = (np.asarray(tensors[f'{m}.experts.gate_up_proj_{n}']) for n in ('blocks', 'scales', 'bias'))
    dn_b, dn_s, dn_bias = (np.asarray(tensors[f'{m}.experts.down_proj_{n}']) for n in ('blocks', 'scales', 'bias'))
    rw, rb = np.asarray(tensors[f'{m}.router.weight']), np.asarray(tensors[f'{m}.router.bias'])
    E, N13, G, sixteen = gu_b.shape
    H, I = G * 32, N13 // 2
    if gu_b.dtype != np.uint8 or gu_s.dtype != np.uint8 or dn_b.dtype != np.uint8 or dn_s.dtype != np.uint8 or sixteen != 16:
        raise ValueError(f'{m}.experts: blocks / scales must be uint8 with 16-byte blocks')
    if gu_s.shape != (E, N13, G) or gu_bias.shape != (E, N13) or dn_b.shape != (E, H, I // 32, 16) or dn_s.shape != (E, H, I // 32) \
            or dn_bias.shape != (E, H) or rw.shape != (E, H) or rb.shape != (E,) or N13 % 2 or I % 32:
        raise ValueError(f'{m}: tensor shapes do not describe {E} experts of hidden {H}, width {I}')
    p = f'layers.{layer}.moe_ffn'
    slots = {p + '.gate.weight': np.ascontiguousarray(rw.astype(np.float16).T),
             p + '.gate.bias': np.ascontiguousarray(rb, dtype=np.float32)}
    for x in range(E):
        q = f'{p}.experts.{x}'
        slots[q + '.w1w3.blocks'] = np.ascontiguousarray(gu_b[x].reshape(N13, H // 2))
        slots[q + '.w1w3.scales'] = np.ascontiguousarray(gu_s[x])
        slots[q + '.w1w3.bias'] = np.ascontiguousarray(gu_bias[x], dtype=np.float16)
        slots[q + '.w2.blocks'] = np.ascontiguousarray(dn_b[x].reshape(H, I // 2))
        slots[q + '.w2.scales'] = np.ascontiguousarray(dn_s[x])
        slots[q + '.w2.bias'] = np.ascontiguousarray(dn_bias[x], dtype=np.float16)
    return slots


def gpt_oss_expert_slots_f16(tensors: dict, layer: int) -> dict:
    """gpt_oss_expert_slots for the unquantised form (what transformers' save_pretrained writes, bf16 or fp16):
      model.layers.{i}.mlp.experts.gate_up_proj [E, H, 2I]   input-major, columns (gate_j, up_j)-interleaved: w1w3 [K][N] as stored
      ...gate_up_proj_bias [E, 2I]     ...down_proj [E, I, H]     ...down_proj_bias [E, H]     router as published
    -> fp16 "...w1w3.weight" [H][2I] / "...w2.weight" [I][H] slots next to the same bias and router slots."""
    m = f'model.layers.{layer}.mlp'
    gu, gu_bias = np.asarray(tensors[f'{m}.experts.gate_up_proj']), np.asarray(tensors[f'{m}.experts.gate_up_proj_bias'])
    dn, dn_bias = np.asarray(tensors[f'{m}.experts.down_proj']), np.asarray(tensors[f'{m}.experts.down_proj_bias'])
    rw, rb = np.asarray(tensors[f'{m}.router.weight']), np.asarray(tensors[f'{m}.router.bias'])
    E, H, N13 = gu.shape
    I = N13 // 2
    if N13 % 2 or gu_bias.shape != (E, N13) or dn.shape != (E, I, H) or dn_bias.shape != (E, H) or rw.shape != (E, H) or rb.shape != (E,):
        raise ValueError(f'{m}: tensor shapes do not describe {E} experts of hidden {H}, width {I}')
    p = f'layers.{layer}.moe_ffn'
    slots = {p + '.gate.weight': np.ascontiguousarray(rw.astype(np.float16).T),
             p + '.gate.bias': np.ascontiguousarray(rb, dtype=np.float32)}
    for x in range(E):
        q = f'{p}.experts.{x}'
        slots[q + '.w1w3.weight'] = np.ascontiguousarray(gu[x], dtype=np.float16)
        slots[q + '.w1w3.bias'] = np.ascontiguousarray(gu_bias[x], dtype=np.float16)
        slots[q + '.w2.weight'] = np.ascontiguousarray(dn[x], dtype=np.float16)
        slots[q + '.w2.bias'] = np.ascontiguousarray(dn_bias[x], dtype=np.float16)
    return slots


def _load_gpt_oss(t: '_Tensors', cfg: ModelConfig) -> dict:
    """GptOssForCausalLM -> the weights of export_weights, zero-padded to multiples of 128 (loader.pad_model_weights)"""
    D, Hq, Hkv = cfg.head_dim, cfg.q_heads, cfg.kv_heads
    layers = []
    for i in range(cfg.layers):
        p = f'model.layers.{i}'
        a = p + '.self_attn.'
        q, k, v, wo = (_linear(t, a + n, False) for n in ('q_proj', 'k_proj', 'v_proj', 'o_proj'))
        q = _map(q, lambda w: permute_qk_for_interleaved_rope(w, Hq, D))
        k = _map(k, lambda w: permute_qk_for_interleaved_rope(w, Hkv, D))
        qkv_bias = np.concatenate([permute_qk_for_interleaved_rope(t.get(a + 'q_proj.bias').astype(np.float16), Hq, D),
                                   permute_qk_for_interleaved_rope(t.get(a + 'k_proj.bias').astype(np.float16), Hkv, D),
                                   t.get(a + 'v_proj.bias').astype(np.float16)])
        m = p + '.mlp'
        mx = cfg.moe_expert_format == 3
        names = [f'{m}.router.weight', f'{m}.router.bias'] + [
            f'{m}.experts.{w}{sfx}' for w in ('gate_up_proj', 'down_proj') for sfx in (('_blocks', '_scales', '_bias') if mx else ('', '_bias'))]
        missing = [n for n in names if n not in t]
        if missing:
            raise FileNotFoundError(f'gpt-oss checkpoint ({"MXFP4" if mx else "unquantised"} experts per config.json) lacks {missing[0]}')
        slots = (gpt_oss_expert_slots if mx else gpt_oss_expert_slots_f16)({n: t.get(n) for n in names}, i)
        s = f'layers.{i}.moe_ffn'
        if slots[s + '.gate.weight'].shape != (cfg.hidden, cfg.moe_experts):
            raise ValueError(f'{m}: the tensors describe a router of {slots[s + ".gate.weight"].shape}, config.json says '
                             f'({cfg.hidden}, {cfg.moe_experts})')
        experts = []
        for x in range(cfg.moe_experts):
            e = f'{s}.experts.{x}'
            lin = (lambda w: dict(blocks=slots[f'{e}.{w}.blocks'], scales=slots[f'{e}.{w}.scales'])) if mx else \
                (lambda w: dict(w=slots[f'{e}.{w}.weight']))
            experts.append(dict(w1w3=lin('w1w3'), w2=lin('w2'), w1w3_bias=slots[e + '.w1w3.bias'], w2_bias=slots[e + '.w2.bias']))
        layers.append(dict(attn_norm=t.get(p + '.input_layernorm.weight').astype(np.float16),
                           ffn_norm=t.get(p + '.post_attention_layernorm.weight').astype(np.float16), w_qkv=_cat([q, k, v]), wo=wo,
                           qkv_bias=qkv_bias, wo_bias=t.get(a + 'o_proj.bias').astype(np.float16),
                           sinks=t.get(a + 'sinks').astype(np.float16), moe_gate=slots[s + '.gate.weight'],
                           moe_gate_bias=slots[s + '.gate.bias'], experts=experts))
    emb = t.get('model.embed_tokens.weight')
    head = emb if (cfg.tie_word_embeddings or 'lm_head.weight' not in t) else t.get('lm_head.weight')
    w = dict(tok_embeddings=emb.astype(np.float16), layers=layers, norm=t.get('model.norm.weight').astype(np.float16),
             output=np.ascontiguousarray(head.astype(np.float16).T))
    return pad_model_weights(w, cfg.hidden, cfg.inter)


class _Tensors:
    """Lazy name -> numpy lookup over every *.safetensors shard of a checkpoint."""

    def __init__(self, model_path: str):
        from safetensors import safe_open
        self._files = []
        self._index = {}
        for fn in sorted(glob(os.path.join(model_path, '*.safetensors'))):
            f = safe_open(fn, framework='pt')      # numpy has neither bf16 nor fp8
            self._files.append(f)
            for k in f.keys():
                self._index[k] = f
        if not self._index:
            raise FileNotFoundError(f'no *.safetensors under {model_path}')

    def __contains__(self, k):
        return k in self._index

    def get(self, k) -> np.ndarray:
        """numpy view of a tensor: bf16 -> float32 (exact), fp8 -> its uint8 codes, everything else as stored"""
        import torch
        t = self._index[k].get_tensor(k)
        if t.dtype == torch.bfloat16:
            t = t.float()
        elif t.dtype in (torch.float8_e4m3fn, getattr(torch, 'float8_e8m0fnu', torch.float8_e4m3fn)):
            t = t.view(torch.uint8)
        return t.numpy().copy()     # own the memory: the tensor is a view into the file mapping


def _linear_gptq(t: '_Tensors', prefix: str, group: int, zero_offset: int) -> dict:
    """a GPTQ linear (W4['gptq']; GPTQFormat.normalize, weight_format.py:269-282) -> {'q','s','z'} like an AWQ one"""
    G = W4['gptq']
    qw, sc, qz = (t.get(prefix + G[n]) for n in ('qweight', 'scales', 'qzeros'))
    if qw.ndim != 2 or sc.ndim != 2 or qw.shape[1] != sc.shape[1] or qw.shape[0] * 8 != sc.shape[0] * group:
        raise ValueError(f'{prefix}{G["qweight"]}: expected GPTQ int32 [K/8][N] next to scales [K/{group}][N], got {tuple(qw.shape)} and '
                         f'{tuple(sc.shape)}')
    K, N = qw.shape[0] * 8, qw.shape[1]
    if qz.shape != (K // group, N // 8):
        raise ValueError(f'{prefix}{G["qzeros"]}: expected int32 [{K // group}][{N // 8}], got {tuple(qz.shape)}')
    if (prefix + G['g_idx']) in t:
        g_idx = t.get(prefix + G['g_idx']).reshape(-1)
        if g_idx.shape != (K,) or not np.array_equal(g_idx, np.arange(K) // group):
            raise NotImplementedError(f'{prefix}{G["g_idx"]}: not k // {group} -- an act-order (desc_act) checkpoint permutes the '
                                      f'groups along K, which is not served')
    z = unpack_u4_cols(qz).astype(np.int16) + zero_offset
    if z.max() > 15:
        raise ValueError(f'{prefix}{G["qzeros"]}: a stored zero of 15 + {zero_offset} leaves [0, 15] (a gptq_v2 checkpoint says so in '
                         f'checkpoint_format / format)')
    return dict(q=unpack_u4_rows(qw), s=sc.astype(np.float16), z=z.astype(np.float16))


def _linear_pack_quantized(t: '_Tensors', prefix: str, group: int) -> dict:
    """a compressed-tensors pack-quantized linear (W4['compressed-tensors']; CompressedTensorFormat.normalize, weight_format.py:310-321:
    unpack along the input dim, transpose to [K][N]; symmetric weights get zeros of 8) -> {'q','s','z'} like an AWQ one"""
    C = W4['compressed-tensors']
    wp, sc = t.get(prefix + C['weight']), t.get(prefix + C['scales'])
    if wp.ndim != 2 or sc.ndim != 2 or wp.shape[0] != sc.shape[0] or wp.shape[1] * 8 != sc.shape[1] * group:
        raise ValueError(f'{prefix}{C["weight"]}: expected int32 [N][K/8] next to {C["scales"]} [N][K/{group}], got {tuple(wp.shape)} and '
                         f'{tuple(sc.shape)}')
    N, K = wp.shape[0], wp.shape[1] * 8
    if (prefix + C['shape']) in t and tuple(int(x) for x in t.get(prefix + C['shape']).reshape(-1)) != (N, K):
        raise ValueError(f'{prefix}{C["shape"]}: {t.get(prefix + C["shape"]).reshape(-1).tolist()} is not (N, K) = ({N}, {K}) of '
                         f'{C["weight"]}')
    s = np.ascontiguousarray(sc.astype(np.float16).T)
    if (prefix + C['zeros']) in t:
        zp = t.get(prefix + C['zeros'])
        if zp.shape != (N // 8, K // group):
            raise ValueError(f'{prefix}{C["zeros"]}: expected int32 [{N // 8}][{K // group}], got {tuple(zp.shape)}')
        z = np.ascontiguousarray(unpack_u4_rows(zp).T).astype(np.float16)
    else:
        z = np.full(s.shape, C['symmetric_zero'], np.float16)
    return dict(q=np.ascontiguousarray(unpack_u4_cols(wp).T), s=s, z=z)


def _linear(t: _Tensors, prefix: str, quantized: bool) -> dict:
    """-> {'q','s','z'} (uint8 [K,N], fp16 [K/g,N] x2: AWQ, GPTQ and compressed-tensors pack-quantized alike), {'f8','bs'} (e4m3 codes [K,N], fp32 block scales
    [K/128, ceil(N/128)]), {'f8','cs'} (e4m3 codes [K,N], one fp32 scale per output channel [N]), {'i8','cs'} (int8 codes [K,N] with
    the same scales: both INT8 dialects) or {'w'} fp16 [K,N]."""
    w4 = getattr(t, 'w4', None) or {}
    if quantized and w4.get('dialect') == 'gptq' and (prefix + W4['gptq']['qweight']) in t:
        return _linear_gptq(t, prefix, w4['group'], w4['zero_offset'])
    if quantized and (prefix + W4['compressed-tensors']['weight']) in t:      # (its .weight_scale is not the 8-bit forms' below)
        return _linear_pack_quantized(t, prefix, w4.get('group', 128))
    if quantized and (prefix + QUARK['scale_suffix']) in t and t.get(prefix + QUARK['scale_suffix']).dtype == np.uint8:
        # Quark MXFP4 (e8m0 scale bytes; the FP8 forms below carry float scales): the checkpoint layout IS the engine's (output-major)
        w, s = t.get(prefix + QUARK['weight_suffix']), t.get(prefix + QUARK['scale_suffix'])
        if w.dtype != np.uint8 or w.ndim != 2 or s.shape != (w.shape[0], w.shape[1] // 16):
            raise ValueError(f'{prefix}: expected {QUARK["weight_suffix"]} uint8 [out][in / 2] and {QUARK["scale_suffix"]} uint8 '
                             f'[out][in / 32], got {w.dtype} {tuple(w.shape)} and {s.dtype} {tuple(s.shape)}')
        if (s == 255).any():
            raise ValueError(f'{prefix}{QUARK["scale_suffix"]}: scale byte 255 (the e8m0 NaN) is not accepted')
        return dict(blocks=np.ascontiguousarray(w), scales=np.ascontiguousarray(s))
    sq = prefix + INT8['smooth_quant']['scale_suffix']
    if quantized and ((prefix + '.weight_scale') in t or sq in t):  # per-tensor ([] / [1]) or per-channel ([N] / [N, 1]) scale
        sname = sq if sq in t else prefix + '.weight_scale'
        w = t.get(prefix + '.weight')
        if w.dtype not in (np.uint8, np.int8) or (sname == sq and w.dtype != np.int8):
            raise ValueError(f'{prefix}.weight: expected float8_e4m3fn or int8 codes next to {sname.rsplit(".", 1)[1]}, got {w.dtype}')
        N = w.shape[0]
        s = t.get(sname).astype(np.float32)
        if s.shape not in ((), (1,), (N,), (N, 1)):
            raise ValueError(f'{sname}: shape {tuple(s.shape)} is neither a per-tensor ([] / [1]) nor a per-channel '
                             f'([{N}] / [{N}, 1]) scale')
        # (.input_scale / .k_scale / .v_scale of static checkpoints are not read)
        return {'i8' if w.dtype == np.int8 else 'f8': np.ascontiguousarray(w.T),
                'cs': np.ascontiguousarray(np.broadcast_to(s.reshape(-1), (N,)))}
    if quantized and (prefix + '.weight_scale_inv') in t:       # FP8Format.normalize: transpose weight and scales
        w = t.get(prefix + '.weight')
        assert w.dtype == np.uint8, f'{prefix}.weight: expected float8_e4m3fn / uint8 codes, got {w.dtype}'
        return dict(f8=np.ascontiguousarray(w.T), bs=np.ascontiguousarray(t.get(prefix + '.weight_scale_inv').astype(np.float32).T))
    if quantized and (prefix + '.qweight') in t:
        qw, sc = t.get(prefix + '.qweight'), t.get(prefix + '.scales')
        if qw.ndim != 2 or sc.ndim != 2 or qw.shape[1] * 8 != sc.shape[1]:
            raise ValueError(f'{prefix}.qweight: expected AWQ int32 [K][N/8] next to scales [K/g][N], got {tuple(qw.shape)} and '
                             f'{tuple(sc.shape)}')
        return dict(q=unpack_awq_gemm(t.get(prefix + '.qweight')),
                    s=t.get(prefix + '.scales').astype(np.float16),
                    z=unpack_awq_gemm(t.get(prefix + '.qzeros')).astype(np.float16))
    return dict(w=np.ascontiguousarray(t.get(prefix + '.weight').astype(np.float16).T))


def _cat(parts: list) -> dict:
    if 'blocks' in parts[0]:                                    # MXFP4, output-major: stack the rows
        return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}
    return {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]}


def _map(lin: dict, fn) -> dict:
    """apply a per-output-channel permutation; fp8 block scales cover whole heads (128 channels) and stay put (channel scales
    'cs' move with their columns)"""
    if 'blocks' in lin:                                         # MXFP4, output-major: the permutation moves rows
        return {k: np.ascontiguousarray(fn(v.T).T) for k, v in lin.items()}
    return {k: (v if k == 'bs' else fn(v)) for k, v in lin.items()}


def _fuse_w1w3(w1: dict, w3: dict) -> dict:
    """(gate_j, up_j) column interleave (builders/ffn.py:31-34).  fp8: codes interleaved, the scale row becomes
    [w1 blocks | w3 blocks] -- the engine's layout for *.w1w3.scales (include/tm_mi355x.h, tm_moe_set_expert)."""
    if 'blocks' in w1:                                          # MXFP4, output-major: rows (2j, 2j + 1) = (gate_j, up_j)
        return {k: np.ascontiguousarray(interleave_gate_up(w1[k].T, w3[k].T).T) for k in w1}
    if 'f8' in w1 and 'bs' in w1:
        assert w1['f8'].shape[1] % 128 == 0, 'fp8 w1/w3: intermediate size must be a multiple of the 128-column block'
        return dict(f8=interleave_gate_up(w1['f8'], w3['f8']), bs=np.concatenate([w1['bs'], w3['bs']], axis=1), gated=True)
    return {kk: interleave_gate_up(w1[kk], w3[kk]) for kk in w1}


def load_hf_weights(model_path: str, cfg: ModelConfig) -> dict:
    t = _Tensors(model_path)
    if cfg.arch == 'gpt_oss':
        return _load_gpt_oss(t, cfg)
    # `.qweight` is AWQ's and GPTQ's alike: the 4-bit dialect comes from the quantization_config, not from the key
    t.w4 = dict(dialect=getattr(cfg, 'w4_dialect', 'awq'), group=cfg.group, zero_offset=getattr(cfg, 'w4_zero_offset', 1))
    if cfg.group != 128 and cfg.moe_experts:
        raise NotImplementedError(f'group_size {cfg.group} with moe_experts {cfg.moe_experts}: the group-{cfg.group} kernel serves dense '
                                  f'models only')
    D, Hq, Hkv = cfg.head_dim, cfg.q_heads, cfg.kv_heads
    layers = []
    llama_names = cfg.arch != 'internlm2'        # Llama / Mixtral / Qwen2 / Qwen3
    root = 'model.'
    if getattr(cfg, 'mrope_section', None):      # Qwen2-VL: the language model's prefix (QWEN_VL); the vision tensors are never read
        found = [pfx for pfx in QWEN_VL['language_prefixes'] if pfx + 'embed_tokens.weight' in t]
        if not found:
            raise ValueError(f'{model_path}: no embed_tokens.weight under any of {QWEN_VL["language_prefixes"]}')
        root = found[0]
    for i in range(cfg.layers):
        extra = {}
        if llama_names:
            p = f'{root}layers.{i}'
            q = _linear(t, p + '.self_attn.q_proj', cfg.quantized)
            k = _linear(t, p + '.self_attn.k_proj', cfg.quantized)
            v = _linear(t, p + '.self_attn.v_proj', cfg.quantized)
            wo = _linear(t, p + '.self_attn.o_proj', cfg.quantized)
            moe = None
            if cfg.moe_experts:      # router [E, H] (unquantised also in AWQ checkpoints) -> fp16 [H][E]; per-expert w1 / w3 / w2
                # (AWQ, FP8 or, in the checkpoints as published, fp16 / bf16 -> fp16 [K][N] like the dense linears)
                # Mixtral (models/mixtral.py:73-106): block_sparse_moe.experts.X.w1 / w3 / w2; Qwen3-MoE (models/qwen3.py:110-121) and
                # Qwen2-MoE (models/qwen2.py:110-128): mlp.experts.X.gate_proj / up_proj / down_proj
                m, names = ((p + '.mlp', ('gate_proj', 'up_proj', 'down_proj')) if cfg.arch in ('qwen2', 'qwen3')
                            else (p + '.block_sparse_moe', ('w1', 'w3', 'w2')))
                moe = dict(moe_gate=np.ascontiguousarray(t.get(m + '.gate.weight').astype(np.float16).T), experts=[])
                for x in range(cfg.moe_experts):
                    e1, e3, e2 = (_linear(t, f'{m}.experts.{x}.{n}', cfg.quantized) for n in names)
                    moe['experts'].append(dict(w1w3=_fuse_w1w3(e1, e3), w2=e2))
                if getattr(cfg, 'moe_shared_inter', 0):
                    # Qwen2-MoE: the shared expert is a dense FFN (the engine's feed_forward slots), its gate an unquantised [1, H] row
                    sg = m + '.shared_expert_gate'
                    if (sg + '.qweight') in t or (sg + '.weight_scale_inv') in t or (sg + W4['compressed-tensors']['weight']) in t:
                        raise NotImplementedError(f'{sg}: a quantised shared-expert gate is not implemented (the gate is read as '
                                                  f'fp16 / bf16 [1, hidden])')
                    s1, s3, s2 = (_linear(t, f'{m}.shared_expert.{n}', cfg.quantized) for n in names)
                    gate = t.get(sg + '.weight')
                    if gate.dtype == np.uint8 or gate.size != cfg.hidden:
                        raise NotImplementedError(f'{sg}.weight: expected fp16 / bf16 [1, {cfg.hidden}], got {gate.dtype} '
                                                  f'{tuple(gate.shape)}')
                    moe.update(w1w3=_fuse_w1w3(s1, s3), w2=s2, shared_gate=np.ascontiguousarray(gate.astype(np.float16).reshape(-1)))
                w1 = w3 = w2 = None
            else:
                w1 = _linear(t, p + '.mlp.gate_proj', cfg.quantized)
                w3 = _linear(t, p + '.mlp.up_proj', cfg.quantized)
                w2 = _linear(t, p + '.mlp.down_proj', cfg.quantized)
            n1 = t.get(p + '.input_layernorm.weight')
            n2 = t.get(p + '.post_attention_layernorm.weight')
            if getattr(cfg, 'attn_bias', 0):      # fp16 [Hq*D | Hkv*D | Hkv*D], q / k channel-permuted like the weights (qwen2.py)
                a = p + '.self_attn.'
                extra['qkv_bias'] = np.concatenate([
                    permute_qk_for_interleaved_rope(t.get(a + 'q_proj.bias').astype(np.float16), Hq, D),
                    permute_qk_for_interleaved_rope(t.get(a + 'k_proj.bias').astype(np.float16), Hkv, D),
                    t.get(a + 'v_proj.bias').astype(np.float16)])
            if getattr(cfg, 'qk_norm', 0):        # [D] each, reordered as one head (qwen3.py: self.norm(pfx + 'q_norm', reorder))
                for n in ('q_norm', 'k_norm'):
                    extra[n] = permute_qk_for_interleaved_rope(t.get(f'{p}.self_attn.{n}.weight').astype(np.float16), 1, D)
        else:   # internlm2: fused wqkv, per kv group [q_0..q_{g-1}, k, v] (models/internlm2.py:34-87)
            p = f'model.layers.{i}'
            moe = None
            wqkv = _linear(t, p + '.attention.wqkv', cfg.quantized)
            g = Hq // Hkv

            def split(x):
                lead = x.shape[:-1]
                x = x.reshape(*lead, Hkv, g + 2, D)
                return (x[..., :g, :].reshape(*lead, Hq * D), x[..., g, :].reshape(*lead, Hkv * D),
                        x[..., g + 1, :].reshape(*lead, Hkv * D))
            parts = {k_: split(v_) for k_, v_ in wqkv.items()}
            q = {k_: parts[k_][0] for k_ in parts}
            k = {k_: parts[k_][1] for k_ in parts}
            v = {k_: parts[k_][2] for k_ in parts}
            wo = _linear(t, p + '.attention.wo', cfg.quantized)
            w1 = _linear(t, p + '.feed_forward.w1', cfg.quantized)
            w3 = _linear(t, p + '.feed_forward.w3', cfg.quantized)
            w2 = _linear(t, p + '.feed_forward.w2', cfg.quantized)
            n1 = t.get(p + '.attention_norm.weight')
            n2 = t.get(p + '.ffn_norm.weight')
        if ('i8' in wo) != (getattr(cfg, 'weight_format', None) == 'int8'):       # the tensors must be what the quantization_config announced
            raise ValueError(f'{p}: the o projection holds {"int8" if "i8" in wo else "no int8"} codes but the quantization_config '
                             f'describes weight format {getattr(cfg, "weight_format", None)!r}')
        q = _map(q, lambda a: permute_qk_for_interleaved_rope(a, Hq, D))
        k = _map(k, lambda a: permute_qk_for_interleaved_rope(a, Hkv, D))
        ffn = moe if moe is not None else dict(w1w3=_fuse_w1w3(w1, w3), w2=w2)
        layers.append(dict(attn_norm=n1.astype(np.float16), ffn_norm=n2.astype(np.float16), w_qkv=_cat([q, k, v]), wo=wo, **ffn,
                           **extra))
    if llama_names:
        emb = t.get(root + 'embed_tokens.weight')
        norm = t.get(root + 'norm.weight')
        tied = getattr(cfg, 'tie_word_embeddings', False) or 'lm_head.weight' not in t
        head = emb if tied else t.get('lm_head.weight')
    else:
        emb = t.get('model.tok_embeddings.weight')
        norm = t.get('model.norm.weight')
        head = t.get('output.weight')
    return dict(tok_embeddings=emb.astype(np.float16), layers=layers, norm=norm.astype(np.float16),
                output=np.ascontiguousarray(head.astype(np.float16).T))
