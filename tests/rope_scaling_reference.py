"""numpy restatement of the two RoPE recipes the oracle does not carry -- YaRN and dynamic NTK -- in the oracle's own deterministic
form (fp32 products, exp2 / sin / cos in float64 on those fp32 values, rounded fp32 -> fp16), plus a helper that runs the oracle one
sequence at a time.  Sources restated (arithmetic only):
  * parser                lmdeploy/turbomind/models/utils.py:64-187 (attention_factor from attention_factor | mscale / mscale_all_dim |
                          0.1 ln(factor) + 1; factor = max_position_embeddings / original when the latter is given; copy_rope_config hands
                          the MODEL's max_position_embeddings to the engine)
  * kernel parameters     src/turbomind/models/attention_weight.cc:37-93 (correction range, ramp_inv_factor_div_2 / _mul_min)
  * frequencies           src/turbomind/kernels/attention/rotary_embedding.h:21-36,74-110,169-181
  * per-sequence base     src/turbomind/models/llama/unified_attention_layer.cc:228-243
Sequences do not interact, so a per-sequence base is a per-sequence default RoPE: OracleModel(batch=1) with RopeParam(dim, base_b).
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from oracle import tm_oracle as o

f16, f32, f64 = np.float16, np.float32, np.float64


def yarn_mscale(scale: float, mscale: float = 1.0) -> float:
    return 1.0 if scale <= 1 else 0.1 * mscale * math.log(scale) + 1.0


def yarn_attention_factor(rs: dict) -> float:
    """attention_factor of a rope_scaling dict, from the factor AS WRITTEN (before original_max_position_embeddings replaces it)"""
    if rs.get('attention_factor') is not None:
        return float(rs['attention_factor'])
    factor = rs.get('factor', 0.0)
    if rs.get('mscale') is not None and rs.get('mscale_all_dim') is not None:
        return float(yarn_mscale(factor, rs['mscale']) / yarn_mscale(factor, rs['mscale_all_dim']))
    return yarn_mscale(factor)


def default_freq(dim: int, base: float) -> np.ndarray:
    i = np.arange(0, dim, 2, dtype=f32)
    scale_factor = f32(-math.log2(float(f32(base))) / dim)
    return np.exp2((i * scale_factor).astype(f32).astype(f64)).astype(f32)


def yarn_correction_range(dim: int, base: float, max_pos: int, beta_fast: float, beta_slow: float):
    base = float(f32(base))

    def corr(rot):
        return (dim * math.log(max_pos / (float(f32(rot)) * 2.0 * math.pi))) / (2.0 * math.log(base))
    low = max(f32(math.floor(corr(beta_fast))), f32(0))
    high = min(f32(math.ceil(corr(beta_slow))), f32(dim - 1))
    if low == high:
        high = f32(high + f32(0.001))
    return f32(low), f32(high)


def yarn_inv_freq(dim: int, base: float, factor: float, max_pos: int, beta_fast: float = 32.0, beta_slow: float = 1.0) -> np.ndarray:
    """inv_freq = freq - freq * alpha * (1 - 1 / factor), alpha the clamped ramp between the correction dimensions"""
    freq = default_freq(dim, base)
    low, high = yarn_correction_range(dim, base, max_pos, beta_fast, beta_slow)
    span = float(f32(high - low))
    div_2 = f32(1.0 / span / 2.0)
    mul_min = f32(1.0 / span * float(low))
    inv_factor = f32(1.0 / float(f32(factor))) if factor != 0 else f32(1)
    i = np.arange(0, dim, 2, dtype=f32)
    alpha = np.clip(((i * div_2).astype(f32) - mul_min).astype(f32), f32(0), f32(1)).astype(f32)
    return (freq - ((freq * alpha).astype(f32) * (f32(1) - inv_factor)).astype(f32)).astype(f32)


def dynamic_base(base: float, factor: float, dim: int, max_pos: int, prompt_len: int) -> float:
    """the sequence's base in float64"""
    if factor > 1 and prompt_len > max_pos:
        s = factor * prompt_len / max_pos - (factor - 1)
        return base * s ** (dim / (dim - 2.0))
    return float(base)


def table(inv_freq: np.ndarray, positions, attention_factor: float = 1.0):
    """(cos, sin) fp16 [len(positions), dim / 2] for arbitrary inverse frequencies; the factor multiplies in fp32 before the cast"""
    ang = (np.asarray(positions, f32)[:, None] * np.asarray(inv_freq, f32)[None, :]).astype(f32).astype(f64)
    af = f32(attention_factor)
    return ((np.cos(ang).astype(f32) * af).astype(f32).astype(f16), (np.sin(ang).astype(f32) * af).astype(f32).astype(f16))


def table_packed(inv_freq: np.ndarray, max_pos: int, attention_factor: float = 1.0) -> np.ndarray:
    """the engine's layout: fp16 [max_pos][dim / 2][2]"""
    c, s = table(inv_freq, np.arange(max_pos), attention_factor)
    return np.stack([c, s], axis=-1)


class PerSequenceOracle:
    """The oracle model run one sequence at a time, every sequence with a RoPE of its own: `ropes[b]` is an o.RopeParam (e.g.
    RopeParam(dim, base_b) for dynamic NTK) or a packed table fp16 [rows][dim / 2][2] that replaces the oracle's table look-up for
    that sequence (YaRN).  forward() has OracleModel.forward's interface; `models[b].cache / .tables[0]` hold sequence b's KV."""

    def __init__(self, cfg, weights, ropes, max_ctx: int):
        self.models, self.tabs = [], []
        for r in ropes:
            tab = None if isinstance(r, o.RopeParam) else np.asarray(r, f16)
            rp = r if tab is None else o.RopeParam(cfg.rope.dim, cfg.rope.base)
            self.models.append(o.OracleModel(dataclasses.replace(cfg, rope=rp), weights, batch=1, max_ctx=max_ctx))
            self.tabs.append(tab)

    def forward(self, ids_per_seq):
        ids, logits = [], []
        for m, tab, t in zip(self.models, self.tabs, ids_per_seq):
            saved = o.rope_cos_sin
            if tab is not None:
                o.rope_cos_sin = lambda p, pos, _t=tab: (_t[np.asarray(pos), :, 0], _t[np.asarray(pos), :, 1])
            try:
                i, lg = m.forward([t])
            finally:
                o.rope_cos_sin = saved
            ids.append(i[0])
            logits.append(lg[0])
        return np.asarray(ids), np.stack(logits)
