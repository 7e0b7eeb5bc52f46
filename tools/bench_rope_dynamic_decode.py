#!/usr/bin/env python
"""What dynamic-NTK RoPE costs: the decode step of a synthetic InternLM2-20B-shaped model (6144 / 48 q x 8 kv heads / 16384 / 92544, u4
weights, int8 KV, graph replay) at batch 64, context ~1k, three ways --
  tables   rope_type 4, factor 2, max_position_embeddings 512: every sequence has a table of its own, unfused decode prologue
  fused    the same engine with rope_type 0: one table, the fused decode prologue (today's path)
  unfused  rope_type 0 with TM_FUSE_QKV=0: one table, unfused prologue -- what `tables` should equal
Arms alternate per round (one engine per run).  `--table-cost`: HIP-event time of building one table of 32769 and 65537 rows next to
the prefill time of a prompt that long (batch 1).
    python tools/bench_rope_dynamic_decode.py [--rounds 3] [--steps 64] [--arms tables,fused,unfused] [--table-cost]
One JSON line per run on stdout, then a summary (median ms per decode step and tokens/s per arm)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402
from lmdeploy_amd.turbomind import checkpoint  # noqa: E402
from lmdeploy_amd.turbomind.engine import Engine  # noqa: E402
from oracle import tm_oracle as o  # noqa: E402

BASE = 1e6


def make_cfg(dynamic: bool, max_pos_emb: int):
    cfg = o.ModelConfig(**o.INTERNLM2_20B, rope=o.RopeParam(128, BASE), kv_bits=8)
    if dynamic:
        cfg.rope = checkpoint.RopeConfig(128, BASE, 'dynamic', 2.0, max_position_embeddings=max_pos_emb)
    return cfg


def run(arm: str, batch: int, ctx: int, warmup: int, steps: int) -> dict:
    import torch
    cfg = make_cfg(arm == 'tables', 512)
    if arm == 'unfused':
        os.environ['TM_FUSE_QKV'] = '0'     # read when the batch is admitted
    try:
        eng = Engine.from_model_config(cfg, max_batch_size=batch, session_len=ctx + warmup + steps + 8, quant_policy=8,
                                       max_prefill_token_num=8192, use_graph=1)
        eng.init_synthetic(seed=1)
        eng.start()
        info = eng.rope_info()
        rng = np.random.default_rng(0)
        eng.prefill([rng.integers(0, cfg.vocab, ctx).astype(np.int32) for _ in range(batch)], max_new_tokens=warmup + steps + 1)
        eng.decode(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.decode(steps)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        eng.close()
    finally:
        os.environ.pop('TM_FUSE_QKV', None)
    return dict(arm=arm, batch=batch, ctx=ctx, steps=steps, per_seq_tables=info['per_seq_tables'], table_bytes=info['table_bytes'],
                ms_per_step=round(ms, 4), tok_per_s=round(batch * 1e3 / ms, 1))


def table_cost(reps: int) -> list:
    import torch
    lib = _ffi.load()
    out = []
    cfg = make_cfg(False, 0)
    eng = Engine.from_model_config(cfg, max_batch_size=1, session_len=65536 + 8, quant_policy=8, max_prefill_token_num=8192, use_graph=0)
    eng.init_synthetic(seed=1)
    eng.start()
    rng = np.random.default_rng(0)
    for max_pos in (32769, 65537):
        p = _ffi.RopeParam(dim=128, base=3.5e6, type=4, factor=2.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position=0,
                           max_position_embeddings=32768, yarn_beta_fast=32.0, yarn_beta_slow=1.0, yarn_attention_factor=1.0)
        buf = torch.empty((max_pos, 64, 2), dtype=torch.float16, device='cuda')
        st = torch.cuda.current_stream().cuda_stream
        ms = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _ffi.check(lib.tm_rope_table_device(buf.data_ptr(), max_pos, ctypes.byref(p), st))
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        n = max_pos - 1
        prompt = rng.integers(0, cfg.vocab, n).astype(np.int32)
        pf = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.prefill([prompt], max_new_tokens=2)
            eng.sync()
            pf.append((time.perf_counter() - t0) * 1e3)
            eng.release()
        out.append(dict(table_rows=max_pos, table_ms_first=round(ms[0], 4), table_ms_median=round(float(np.median(ms[1:])), 4),
                        prefill_tokens=n, prefill_ms=round(min(pf), 1)))
        print(json.dumps(out[-1]), flush=True)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arms', default='tables,fused,unfused')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ctx', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--table-cost', action='store_true')
    ap.add_argument('--table-reps', type=int, default=5)
    a = ap.parse_args()
    arms = [x for x in a.arms.split(',') if x]
    res = []
    for r in range(a.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            res.append(run(arm, a.batch, a.ctx, a.warmup, a.steps))
            print(json.dumps(dict(res[-1], round=r)), flush=True)
    for arm in arms:
        ms = [x['ms_per_step'] for x in res if x['arm'] == arm]
        if ms:
            med = float(np.median(ms))
            print(json.dumps(dict(summary=arm, ms_per_step_median=round(med, 4), ms_min=min(ms), ms_max=max(ms),
                                  tok_per_s=round(a.batch * 1e3 / med, 1))), flush=True)
    if a.table_cost:
        table_cost(a.table_reps)


if __name__ == '__main__':
    main()
