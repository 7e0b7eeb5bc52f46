#!/usr/bin/env python
"""Prompt scoring against a plain prefill of the same inputs, Llama-3-8B W4A16 + int8 KV shapes, synthetic weights:
tm_engine_score (lm_head over every prompt row + per-row cross-entropy) vs tm_engine_prefill(max_new_tokens=1) + release
(lm_head over the last row of each prompt).  Prints one JSON line: mean seconds per call of each, their ratio, scored tokens/s.
The per-kernel split (lm_head GEMM, CE kernel) comes from a separate run under `rocprofv3 --kernel-trace --stats -- python ...`.
  python tools/bench_ppl.py [--inputs 64] [--len 1024] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import LLAMA3_8B, _Cfg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs', type=int, default=64)
    ap.add_argument('--len', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-prefill', type=int, default=8192)
    args = ap.parse_args()
    from lmdeploy_amd.turbomind.engine import Engine
    eng = Engine.from_model_config(_Cfg(dict(LLAMA3_8B)), max_batch_size=args.inputs, session_len=args.len + 64, quant_policy=8,
                                   max_prefill_token_num=args.max_prefill)
    eng.init_synthetic(seed=0)
    eng.start()
    rng = np.random.default_rng(0)
    seqs = [rng.integers(0, LLAMA3_8B['vocab'], args.len).astype(np.int32) for _ in range(args.inputs)]

    def prefill():
        eng.prefill(seqs, max_new_tokens=1)
        eng.sync()
        eng.release()

    def score():
        return eng.score(seqs)

    prefill()      # warm-up: lazy module loads, scoring scratch
    nll = score()
    t_pf, t_sc = [], []
    for _ in range(args.reps):     # interleaved, so that clock / thermal drift hits both arms alike
        t0 = time.perf_counter()
        prefill()
        t_pf.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        score()
        t_sc.append(time.perf_counter() - t0)
    eng.close()
    pf, sc = float(np.median(t_pf)), float(np.median(t_sc))
    scored = args.inputs * (args.len - 1)
    mean_nll = float(np.mean([np.mean(x, dtype=np.float64) for x in nll]))
    print(json.dumps(dict(metric='score_vs_prefill', inputs=args.inputs, len=args.len, max_prefill_token_num=args.max_prefill,
                          reps=args.reps, prefill_s=round(pf, 4), score_s=round(sc, 4), ratio=round(sc / pf, 4),
                          scored_tok_per_s=round(scored / sc, 1), prefill_tok_per_s=round(args.inputs * args.len / pf, 1),
                          prefill_s_all=[round(x, 4) for x in t_pf], score_s_all=[round(x, 4) for x in t_sc],
                          mean_nll=round(mean_nll, 4), nll_finite=bool(all(np.isfinite(x).all() for x in nll)))))


if __name__ == '__main__':
    main()
