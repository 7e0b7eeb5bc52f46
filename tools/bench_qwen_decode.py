#!/usr/bin/env python
"""Decode step of synthetic Qwen-shaped models with the attention prologue on and off: batch 64, context ~1k, int8 KV, u4
weights, graph replay.  Qwen2.5-7B (3584 / 28 q x 4 kv heads / 18944 / 152064, q/k/v bias) and Qwen3-8B (4096 / 32 x 8 /
12288 / 151936, per-head q/k RMSNorm); "off" is the same shape with both flags 0 (the Llama path).  Arms alternate per round.
    python tools/bench_qwen_decode.py [--rounds 2] [--steps 64] [--models qwen2_7b,qwen3_8b] [--arms on,off]
One JSON line per run on stdout, then a summary (median ms per decode step per model and arm)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd.turbomind.engine import Engine  # noqa: E402
from oracle import tm_oracle as o  # noqa: E402

MODELS = {
    'qwen2_7b': (dict(hidden=3584, layers=28, q_heads=28, kv_heads=4, head_dim=128, inter=18944, vocab=152064, rms_eps=1e-6),
                 dict(attn_bias=1, qk_norm=0)),
    'qwen3_8b': (dict(hidden=4096, layers=36, q_heads=32, kv_heads=8, head_dim=128, inter=12288, vocab=151936, rms_eps=1e-6),
                 dict(attn_bias=0, qk_norm=1)),
}


def run(model: str, arm: str, batch: int, ctx: int, warmup: int, steps: int) -> dict:
    import torch
    shape, flags = MODELS[model]
    cfg = o.ModelConfig(**shape, rope=o.RopeParam(128, 1e6), kv_bits=8)   # make_model_config reads the two flags by getattr
    cfg.attn_bias, cfg.qk_norm = (flags['attn_bias'], flags['qk_norm']) if arm == 'on' else (0, 0)
    eng = Engine.from_model_config(cfg, max_batch_size=batch, session_len=ctx + warmup + steps + 8, quant_policy=8,
                                   max_prefill_token_num=8192, use_graph=1)
    eng.init_synthetic(seed=1)
    eng.start()
    rng = np.random.default_rng(0)
    eng.prefill([rng.integers(0, cfg.vocab, ctx).astype(np.int32) for _ in range(batch)], max_new_tokens=warmup + steps + 1)
    eng.decode(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.decode(steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    eng.close()
    return dict(model=model, arm=arm, attn_bias=cfg.attn_bias, qk_norm=cfg.qk_norm, batch=batch, ctx=ctx, steps=steps,
                ms_per_step=round(ms, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='qwen2_7b,qwen3_8b')
    ap.add_argument('--arms', default='on,off')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ctx', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--steps', type=int, default=64)
    a = ap.parse_args()
    res = []
    arms = a.arms.split(',')
    for r in range(a.rounds):
        for m in a.models.split(','):
            for arm in (arms if r % 2 == 0 else arms[::-1]):
                res.append(run(m, arm, a.batch, a.ctx, a.warmup, a.steps))
                print(json.dumps(dict(res[-1], round=r)), flush=True)
    for m in a.models.split(','):
        row = {arm: float(np.median([x['ms_per_step'] for x in res if x['model'] == m and x['arm'] == arm])) for arm in arms}
        if 'on' in row and 'off' in row:
            row['on_vs_off_pct'] = round(100 * (row['on'] / row['off'] - 1), 2)
        print(json.dumps(dict(summary=m, **row)), flush=True)


if __name__ == '__main__':
    main()
