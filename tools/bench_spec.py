#!/usr/bin/env python
"""What a speculative step costs next to a plain decode step (synthetic Llama-3-8B geometry, W4A16, int8 KV, context ~1k).

    python tools/bench_spec.py [--batches 1,8,64] [--ks 1,3,7] [--ctx 1000] [--steps 50] [--warmup 6] [--rounds 2]
        per batch, ONE engine: the plain arm (tm_engine_decode, graph replay) and one speculative arm per k (tm_engine_decode_spec,
        graph replay) alternate round by round in this process; device events on the engine stream around `steps` steps after
        `warmup`.  Prints one JSON line per (batch, arm, round) and a summary per batch: median ms per step, r_k = t_spec(k) /
        t_plain, and the break-even acceptance r_k - 1 (accepted drafts per step above which a speculative step emits more tokens per
        millisecond than plain steps).  The prompts are random tokens: a speculative step has a fixed shape, so its time does not
        depend on what is accepted; the acceptance of real text cannot be measured with synthetic weights.
    python tools/bench_spec.py --kernels [--batch 64] [--ctx 1024] [--rows 4] [--iters 20]
        launches of the verify attention (`rows` query rows per sequence) and of the MFMA decode attention over the same random
        cache, for `rocprofv3 --kernel-trace --stats -- python tools/bench_spec.py --kernels` in a run of its own (kernel names:
        verify_attention_i8_mfma_kernel / decode_attention_i8_mfma_kernel and their reduce kernels).
    python tools/bench_spec.py --trace-arm plain|k3 [--batch 8]
        a few steps of one arm and nothing else, for a kernel trace of a whole step."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402
from lmdeploy_amd.turbomind.engine import Engine  # noqa: E402
from oracle import tm_oracle as o  # noqa: E402

LLAMA3_8B = dict(hidden=4096, layers=32, q_heads=32, kv_heads=8, head_dim=128, inter=14336, vocab=128256)


def make_engine(batch, ctx, room):
    cfg = o.ModelConfig(**LLAMA3_8B, rope=o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192), kv_bits=8)
    eng = Engine.from_model_config(cfg, max_batch_size=batch, session_len=ctx + room + 16, quant_policy=8,
                                   max_prefill_token_num=8192, use_graph=1)
    eng.init_synthetic(seed=1)
    eng.start()
    return eng, cfg


def time_arm(eng, cfg, batch, ctx, k, warmup, steps):
    """ms per step of one arm: k = 0 plain decode steps, k > 0 speculative steps; a fresh prefill of the same prompts every time"""
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, ctx).astype(np.int32) for _ in range(batch)]
    eng.set_speculative(k, 3, 1)
    eng.prefill(prompts, max_new_tokens=(warmup + steps) * (k + 1) + 2)
    run = eng.decode_spec if k else eng.decode
    run(warmup)                                    # the eager first step and the capture are in here
    eng.sync()
    stream = torch.cuda.ExternalStream(eng.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    run(steps)
    e1.record(stream)
    eng.sync()
    ms = e0.elapsed_time(e1) / steps
    emitted = None
    if k:
        _, counts = eng.fetch_spec()
        emitted = float(np.mean(counts - 1)) / (warmup + steps)      # tokens per step and sequence (random prompts: close to 1)
    eng.release()
    return ms, emitted


def bench_steps(a):
    ks = [int(v) for v in a.ks.split(',')]
    for batch in [int(v) for v in a.batches.split(',')]:
        eng, cfg = make_engine(batch, a.ctx, (a.warmup + a.steps) * (max(ks) + 1) + max(ks) + 2)
        res = {}
        try:
            for rnd in range(a.rounds):
                arms = [0] + ks
                for k in (arms if rnd % 2 == 0 else arms[::-1]):
                    ms, emitted = time_arm(eng, cfg, batch, a.ctx, k, a.warmup, a.steps)
                    res.setdefault(k, []).append(ms)
                    print(json.dumps(dict(batch=batch, ctx=a.ctx, arm='plain' if k == 0 else f'spec_k{k}', round=rnd, steps=a.steps,
                                          ms_per_step=round(ms, 4), rows=batch * (k + 1),
                                          **({'tokens_per_step_and_sequence': round(emitted, 3)} if k else {}))), flush=True)
        finally:
            eng.close()
        plain = float(np.median(res[0]))
        summ = dict(summary=True, batch=batch, ctx=a.ctx, plain_ms=round(plain, 4), plain_spread_pct=round(100 * (max(res[0]) / min(res[0]) - 1), 2))
        for k in ks:
            t = float(np.median(res[k]))
            summ[f'spec_k{k}_ms'] = round(t, 4)
            summ[f'r_{k}'] = round(t / plain, 3)
            summ[f'break_even_accepted_per_step_k{k}'] = round(t / plain - 1, 3)
        print(json.dumps(summ), flush=True)


def bench_kernels(a):
    tm = _ffi.load()
    B, Hq, Hkv, D, bits, ctx, rows = a.batch, 32, 8, 128, 8, a.ctx, a.rows
    lsz = tm.tm_kv_layer_size(Hkv, D, 64, bits)
    nblk = (ctx + rows + 63) // 64
    pool = torch.randint(0, 255, (B * nblk, lsz), dtype=torch.uint8, device='cuda')
    nparam = Hkv * 2 * 64 * 4
    prm = torch.empty((B * nblk, nparam // 2), dtype=torch.float16, device='cuda').uniform_(0.01, 0.05)
    pool[:, lsz - nparam:] = prm.view(torch.uint8)
    ptrs = (pool.data_ptr() + torch.randperm(B * nblk).to(torch.int64) * lsz).cuda()
    cu_blk = torch.arange(0, (B + 1) * nblk, nblk, dtype=torch.int32, device='cuda')
    view = _ffi.KvCache(ptrs.data_ptr(), cu_blk.data_ptr(), 0, Hkv, D, 64, bits)
    st = torch.cuda.current_stream().cuda_stream
    q = torch.randn((B * rows, Hq * D), device='cuda').half()
    out = torch.empty((B * rows, Hq * D), device='cuda').half()
    cu_q = torch.arange(0, (B + 1) * rows, rows, dtype=torch.int32, device='cuda')
    klen_v = torch.full((B,), ctx + rows, dtype=torch.int32, device='cuda')      # the forward's rows are in the cache
    klen_d = torch.full((B,), ctx + 1, dtype=torch.int32, device='cuda')
    for splits in [int(s) for s in a.splits.split(',')]:
        ws = torch.empty(max(1, tm.tm_verify_attention_workspace(B * rows, Hq, splits)), dtype=torch.uint8, device='cuda')
        for _ in range(a.iters):
            _ffi.check(tm.tm_decode_attention(out.data_ptr(), q.data_ptr(), Hq * D, klen_d.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(), view, st))
            _ffi.check(tm.tm_verify_attention(out.data_ptr(), q.data_ptr(), Hq * D, cu_q.data_ptr(), klen_v.data_ptr(), B, Hq, 0.0, splits,
                                              ws.data_ptr(), view, st))
    torch.cuda.synchronize()
    print(f'{a.iters} launches each of decode attention (ctx {ctx + 1}) and verify attention ({rows} rows, ctx {ctx + rows}) at batch {B}, '
          f'32 q / 8 kv heads, int8 KV, splits {a.splits}: kernel times are in the profiler\'s trace', flush=True)


def trace_arm(a):
    k = 0 if a.trace_arm == 'plain' else int(a.trace_arm[1:])
    eng, cfg = make_engine(a.batch, a.ctx, 64 * 8)
    try:
        ms, _ = time_arm(eng, cfg, a.batch, a.ctx, k, 2, 8)
        print(json.dumps(dict(batch=a.batch, arm=a.trace_arm, ms_per_step_under_the_profiler=round(ms, 4))), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,64')
    ap.add_argument('--ks', default='1,3,7')
    ap.add_argument('--ctx', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--trace-arm', default='')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rows', type=int, default=4)
    ap.add_argument('--splits', default='1,4')
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_spec.py needs a GPU: there is no CPU fallback and no number without one')
    if a.kernels:
        return bench_kernels(a)
    if a.trace_arm:
        return trace_arm(a)
    bench_steps(a)


if __name__ == '__main__':
    main()
