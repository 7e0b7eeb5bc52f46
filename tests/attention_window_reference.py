"""Sliding-window attention and attention sinks restated on the oracle's primitives (oracle.tm_oracle), for the sliding-window tests.

  * window W: the query at absolute position p sees the keys t with 0 <= p - t < W, i.e. the last min(p + 1, W) tokens, itself
    included (the reference's mask, mainloop_sm80.h:558-566; HF Mistral / gpt-oss).  Windowed attention IS full attention over the
    cropped context K[:, n - W:], V[:, n - W:], so the arithmetic is o.decode_attention on the crop; prefill is that row by row.
  * sinks: one natural-log logit per query head that joins the softmax denominator and contributes no value
    (attention_universal.h:529-535).  Restated as a float64 softmax with one extra column per head whose value row is zero.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import tm_oracle as o

f16, f32, f64 = np.float16, np.float32, np.float64


def crop(K, V, n: int, window: int):
    """the keys / values the query at position n - 1 sees: K, V [Hkv, >= n, D] -> [Hkv, min(n, window), D]"""
    lo = max(n - window, 0) if window > 0 else 0
    return K[:, lo:n], V[:, lo:n]


def sink_attention(q, K, V, sinks, softmax_scale=None):
    """q fp16 [Hq, D], K / V fp16 [Hkv, ctx, D], sinks [Hq] -> fp16 [Hq, D]: float64 softmax over [scores | sink], the sink's value 0"""
    Hq, D = q.shape
    G = Hq // K.shape[0]
    scale = (1.0 / math.sqrt(D)) if softmax_scale is None else softmax_scale
    out = np.zeros((Hq, D), f64)
    for hq in range(Hq):
        g = hq // G
        s = np.concatenate([(K[g].astype(f64) @ q[hq].astype(f64)) * scale, [f64(sinks[hq])]])
        p = np.exp(s - s.max())
        p /= p.sum()
        out[hq] = p[:-1] @ V[g].astype(f64)
    return out.astype(f16)


def window_decode(q, K, V, window: int = 0, softmax_scale=None, sinks=None):
    """decode attention of the query at position ctx - 1 over K / V [Hkv, ctx, D] with a window (0 = none) and optional sinks"""
    Kc, Vc = crop(K, V, K.shape[1], window)
    if sinks is None:
        return o.decode_attention(q, Kc, Vc, softmax_scale, 1)
    return sink_attention(q, Kc, Vc, sinks, softmax_scale)


def window_prefill(q, K, V, history: int = 0, window: int = 0, softmax_scale=None, sinks=None):
    """q fp16 [T, Hq, D] on top of `history` cached tokens, K / V fp16 [Hkv, history + T, D]: window_decode row by row"""
    T, Hq, D = q.shape
    out = np.zeros((T, Hq, D), f16)
    for i in range(T):
        n = history + i + 1
        out[i] = window_decode(q[i], K[:, :n], V[:, :n], window, softmax_scale, sinks)
    return out


@dataclass
class WindowConfig(o.ModelConfig):
    window: int = 0                    # every layer's window (0 = none)
    layer_windows: tuple = None        # per layer, replaces `window`
    attn_sinks: int = 0                # layers carry 'sinks' [q_heads]


def make_window_weights(cfg: WindowConfig, seed: int = 0, quantized: bool = True):
    """o.make_synthetic_weights plus, with cfg.attn_sinks, 'sinks' [q_heads] uniform in [-2, 4] per layer"""
    w = o.make_synthetic_weights(cfg, seed, quantized)
    rng = np.random.default_rng(seed + 104729)
    if cfg.attn_sinks:
        for L in w['layers']:
            L['sinks'] = rng.uniform(-2.0, 4.0, cfg.q_heads).astype(f16)
    return w


class WindowOracleModel(o.OracleModel):
    """o.OracleModel (dense FFN) whose attention sees, per layer, the cropped context and the layer's sinks"""

    def layer_window(self, li: int) -> int:
        lw = getattr(self.cfg, 'layer_windows', None)
        return int(lw[li]) if lw is not None else int(getattr(self.cfg, 'window', 0))

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
            W, sinks = self.layer_window(li), Lw.get('sinks')
            qkv = o._linear(x, Lw['w_qkv'], cfg.group)
            attn = np.zeros((len(ids), Hq * D), f16)
            for b, n in enumerate(lens):
                if n == 0:
                    continue
                sl = slice(offs[b], offs[b + 1])
                hist = self.seq_len[b]
                cos, sin = o.rope_cos_sin(cfg.rope, np.arange(hist, hist + n))
                q = o.rope_apply(qkv[sl, :Hq * D].reshape(n, Hq, D), cos, sin)
                o.process_kv(self.cache, self.tables[b], li, qkv[sl, Hq * D:(Hq + Hkv) * D].reshape(n, Hkv, D),
                             qkv[sl, (Hq + Hkv) * D:].reshape(n, Hkv, D), cos, sin, hist)
                if n == 1:
                    kv = [self.cache.load_dequant(self.tables[b], li, hd, 0, hist + 1, 'decode') for hd in range(Hkv)]
                    attn[sl] = window_decode(q[0], np.stack([a for a, _ in kv]), np.stack([c for _, c in kv]), W, self.c,
                                             sinks).reshape(1, -1)
                else:
                    Kf, Vf = o.flatten_kv(self.cache, self.tables[b], li, hist + n)
                    attn[sl] = window_prefill(q, Kf, Vf, hist, W, self.c, sinks).reshape(n, -1)
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
