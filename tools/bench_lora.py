#!/usr/bin/env python
"""What multi-LoRA serving costs on Llama-3-8B's shapes at batch 64 (synthetic W4A16 weights, int8 KV, context ~1k).

    python tools/bench_lora.py [--ranks 16,64] [--batch 64] [--ctx 1000] [--steps 50] [--warmup 6] [--rounds 3] [--iters 200]
        per rank, (1) device-event time per tm_lora_apply at the three linears (w_qkv: three segments, wo, w2) with one adapter on every
        row and with 8 adapters interleaved, the plan kernel timed on its own; (2) the captured decode step in four arms that alternate
        round by round in this process: `base` = an engine with no adapter loaded (the schedule without the feature), and on a second
        engine with 8 adapters loaded `none` (no row selects one: the unfused schedule + launches whose workgroups leave at once), `one`
        (every row the same adapter) and `eight` (rows interleaved over 8).  One JSON line per measurement, medians in the summary:
        none - base = what the unfused schedule costs, one / eight - none = what the delta launches add."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402
from lmdeploy_amd.turbomind import checkpoint  # noqa: E402
from lmdeploy_amd.turbomind.engine import Engine  # noqa: E402
from oracle import tm_oracle as o  # noqa: E402

LLAMA3_8B = dict(hidden=4096, layers=32, q_heads=32, kv_heads=8, head_dim=128, inter=14336, vocab=128256)
H, KQ, KKV, INTER = 4096, 4096, 1024, 14336
LINEARS = {_ffi.LORA_QKV: (H, [KQ, KKV, KKV]), _ffi.LORA_WO: (KQ, [H]), _ffi.LORA_W2: (INTER, [H])}


def operands(rank, seed=0):
    """{kind: (A, B, ranks)} of one random adapter (the same arrays serve every layer and slot: only the time matters here)"""
    rng = np.random.default_rng(seed)
    return {kind: checkpoint.lora_operands([(rng.standard_normal((rank, K), dtype=np.float32) / np.sqrt(K),
                                             rng.standard_normal((n, rank), dtype=np.float32) * 0.01) for n in cols], cols, 1.0)
            for kind, (K, cols) in LINEARS.items()}


def bench_apply(rank, M, iters):
    tm, ops = _ffi.load(), operands(rank)
    ws = torch.zeros(tm.tm_lora_plan_workspace(M), dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(10):
            fn()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for arm, ids in (('one', np.zeros(M, np.int32)), ('eight', (np.arange(M) % 8).astype(np.int32))):
        d_ids = torch.from_numpy(ids).cuda()
        plan = lambda: _ffi.check(tm.tm_lora_plan(ws.data_ptr(), d_ids.data_ptr(), None, M, 8, st))     # noqa: E731
        print(json.dumps(dict(what='tm_lora_plan', rank=rank, M=M, arm=arm, us=round(timed(plan), 2))), flush=True)
        for kind, (K, cols) in LINEARS.items():
            A, B, ranks = ops[kind]
            N, ends, tab = sum(cols), np.cumsum(cols), C.c_void_p()
            _ffi.check(tm.tm_lora_table_create(C.byref(tab), K, N, len(cols), (C.c_int * len(cols))(*(ends - cols)), (C.c_int * len(cols))(*ends), 8))
            for s in range(8):
                _ffi.check(tm.tm_lora_table_set(tab, s, A.ctypes.data, B.ctypes.data, (C.c_int * len(cols))(*ranks), B.shape[1]))
            x = torch.randn(M, K, device='cuda', dtype=torch.float16)
            y = torch.zeros(M, N, device='cuda', dtype=torch.float16)
            us = timed(lambda: _ffi.check(tm.tm_lora_apply(tab, x.data_ptr(), K, y.data_ptr(), N, M, ws.data_ptr(), st)))
            print(json.dumps(dict(what='tm_lora_apply', linear=('w_qkv', 'wo', 'w2')[kind], rank=rank, M=M, K=K, N=N, arm=arm, us=round(us, 2))),
                  flush=True)
            tm.tm_lora_table_destroy(tab)


def make_engine(batch, ctx, room):
    cfg = o.ModelConfig(**LLAMA3_8B, rope=o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192), kv_bits=8)
    eng = Engine.from_model_config(cfg, max_batch_size=batch, session_len=ctx + room + 16, quant_policy=8, max_prefill_token_num=8192,
                                   cache_blocks=batch * ((ctx + room + 16) // 64 + 2), use_graph=1)
    eng.init_synthetic(seed=1)
    eng.start()
    return eng, cfg


def time_steps(eng, cfg, batch, ctx, slots, warmup, steps):
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, ctx).astype(np.int32) for _ in range(batch)]
    if slots is not None:
        eng.set_adapters(slots)
    eng.prefill(prompts, max_new_tokens=warmup + steps + 2)
    eng.decode(warmup)                              # the eager first step and the capture are in here
    eng.sync()
    stream = torch.cuda.ExternalStream(eng.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    eng.decode(steps)
    e1.record(stream)
    eng.sync()
    eng.release()
    return e0.elapsed_time(e1) / steps


def bench_steps(a, rank, base, lora, cfg):
    ops = operands(rank)
    for slot in range(8):
        for layer in range(cfg.layers):
            for kind, (A, B, ranks) in ops.items():
                lora.load_adapter(slot, layer, kind, A, B, ranks)
    arms = dict(base=(base, None), none=(lora, [-1] * a.batch), one=(lora, [0] * a.batch), eight=(lora, [b % 8 for b in range(a.batch)]))
    res = {k: [] for k in arms}
    for rnd in range(a.rounds):
        for name, (eng, slots) in arms.items():
            ms = time_steps(eng, cfg, a.batch, a.ctx, slots, a.warmup, a.steps)
            res[name].append(ms)
            print(json.dumps(dict(what='decode_step', rank=rank, batch=a.batch, arm=name, round=rnd, ms_per_step=round(ms, 4))), flush=True)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps(dict(what='summary', rank=rank, batch=a.batch, median_ms=med, unfused_schedule_ms=round(med['none'] - med['base'], 4),
                          delta_one_ms=round(med['one'] - med['none'], 4), delta_eight_ms=round(med['eight'] - med['none'], 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (('--ranks', '16,64'), ('--batch', 64), ('--ctx', 1000), ('--steps', 50), ('--warmup', 6), ('--rounds', 3), ('--iters', 200)):
        ap.add_argument(name, type=type(default), default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_lora.py needs a GPU'
    for rank in [int(r) for r in a.ranks.split(',')]:
        bench_apply(rank, a.batch, a.iters)
    base, cfg = make_engine(a.batch, a.ctx, a.warmup + a.steps + 2)
    lora, _ = make_engine(a.batch, a.ctx, a.warmup + a.steps + 2)
    for rank in [int(r) for r in a.ranks.split(',')]:
        bench_steps(a, rank, base, lora, cfg)
    base.close()
    lora.close()


if __name__ == '__main__':
    main()
