#!/usr/bin/env python
"""What M-RoPE and image embeddings cost, at the Qwen2-VL-7B geometry (28 q / 4 kv heads of 128, hidden 3584, int8 KV).

  python tools/bench_mrope.py [--store] [--embedding] [--engine] [--rounds 5] [--iters 20]

--store      tm_kv_rope_store_mrope (coordinates of an image grid, sections 16 / 24 / 24) against tm_kv_rope_store_qk (bias on, as
             Qwen2 has it) for 8192 prefill rows (8 sequences of 1024) and for 64 decode rows (no coordinates, a delta array).
--embedding  tm_embedding_mixed (half of the rows from the request's buffer) against tm_embedding, 8192 rows of 3584.
--engine     one decode step (graph replay, batch 64, context 1024) of a synthetic W4A16 engine of that geometry with sections (the delta
             array of zeros: the fused prologue's pos_delta arm) against the same engine without.
No section given: all three.  The variants are timed interleaved, round after round, in this one process (a median of --iters launches
each, device events around the launches; the median and minimum over the rounds are printed).  Without a GPU the tool fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi, vl  # noqa: E402

HQ, HKV, HIDDEN, SECTIONS = 28, 4, 3584, (16, 24, 24)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return median([a.elapsed_time(b) for a, b in ev]) * 1e3       # us


def compare(name, arms, a):
    for fn in arms.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, a.iters))
    base = None
    for k in arms:
        med = median(res[k])
        base = base or med
        print(f'{name} {k:28s}: median {med:8.1f} us  min {min(res[k]):8.1f} us  ({med / base:.3f} of the first)', flush=True)


def bench_store(tm, a):
    st = torch.cuda.current_stream().cuda_stream
    lsz = tm.tm_kv_layer_size(HKV, 128, 64, 8)
    tab = np.zeros((2049, 64, 2), np.float16)
    _ffi.check(tm.tm_rope_table(tab.ctypes.data, 2049, 128, 1e6, 0, 1.0, 1.0, 4.0, 8192))
    tab_d = torch.from_numpy(tab).cuda()
    bias = (0.1 * torch.randn((HQ + 2 * HKV) * 128, device='cuda')).half()
    for what, B, new, hist in (('prefill 8 x 1024 rows', 8, 1024, 0), ('decode 64 rows', 64, 1, 1023)):
        T, nblk = B * new, (hist + new + 63) // 64
        qkv = torch.randn((T, (HQ + 2 * HKV) * 128), device='cuda').half()
        cu_q = torch.arange(0, T + 1, new, dtype=torch.int32, device='cuda')
        klen = torch.full((B,), hist + new, dtype=torch.int32, device='cuda')
        pool = torch.zeros((B * nblk, lsz), dtype=torch.uint8, device='cuda')
        ptrs = (pool.data_ptr() + torch.randperm(B * nblk).to(torch.int64) * lsz).cuda()
        cu_b = torch.arange(0, (B + 1) * nblk, nblk, dtype=torch.int32, device='cuda')
        cache = _ffi.KvCache(ptrs.data_ptr(), cu_b.data_ptr(), 0, HKV, 128, 64, 8)
        head = (qkv.data_ptr(), HQ, cu_q.data_ptr(), klen.data_ptr(), B, T, tab_d.data_ptr(), 2049)
        tail = (bias.data_ptr(), None, None, 0.0, cache, st)
        delta = torch.zeros(B, dtype=torch.int32, device='cuda')
        arms = {'plain (tm_kv_rope_store_qk)': lambda: _ffi.check(tm.tm_kv_rope_store_qk(*head, *tail))}
        if new > 1:      # every sequence: 16 text tokens, a 56 x 64 image (28 x 32 = 896 tokens), 112 text tokens
            ids = np.array([1] * 16 + [0] * 896 + [1] * 112)
            pos, _ = vl.mrope_positions(ids, [[1, 56, 64]], 0, 2)
            coords = torch.from_numpy(np.ascontiguousarray(np.tile(pos.T, (B, 1)))).cuda()
            arms['mrope, coordinates'] = lambda: _ffi.check(tm.tm_kv_rope_store_mrope(*head, coords.data_ptr(), None, *SECTIONS, *tail))
        arms['mrope, delta array'] = lambda: _ffi.check(tm.tm_kv_rope_store_mrope(*head, None, delta.data_ptr(), *SECTIONS, *tail))
        compare(f'store {what}:', arms, a)


def bench_embedding(tm, a):
    st = torch.cuda.current_stream().cuda_stream
    T, vocab = 8192, 152064
    table = torch.randn((vocab, HIDDEN), device='cuda').half()
    rows = torch.randn((T // 2, HIDDEN), device='cuda').half()
    ids = torch.randint(0, vocab, (T,), dtype=torch.int32, device='cuda')
    index = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    index[T // 4:T // 4 + T // 2] = torch.arange(T // 2, dtype=torch.int32, device='cuda')
    out = torch.empty((T, HIDDEN), dtype=torch.float16, device='cuda')
    compare('embedding 8192 x 3584:', {
        'tm_embedding': lambda: _ffi.check(tm.tm_embedding(out.data_ptr(), table.data_ptr(), ids.data_ptr(), T, HIDDEN, vocab, st)),
        'tm_embedding_mixed, half': lambda: _ffi.check(tm.tm_embedding_mixed(out.data_ptr(), table.data_ptr(), ids.data_ptr(), rows.data_ptr(),
                                                                             index.data_ptr(), T, HIDDEN, vocab, st))}, a)


def bench_engine(tm, a):
    from lmdeploy_amd.turbomind.engine import Engine

    class Rope:
        dim, base, type, factor = 128, 1e6, 'default', 1.0
        low_freq_factor, high_freq_factor, original_max_position_embeddings = 1.0, 4.0, 8192

    class Cfg:
        hidden, layers, q_heads, kv_heads, head_dim, inter, vocab = HIDDEN, 28, HQ, HKV, 128, 18944, 152064
        rms_eps, group, rope, attn_bias = 1e-6, 128, Rope(), 1

    B, ctx, steps = 64, 1024, 64
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, 1000, ctx).astype(np.int32) for _ in range(B)]
    res = {}
    for rnd in range(a.rounds):
        for name, sections in (('without sections', None), ('with sections', SECTIONS)):
            cfg = Cfg()
            cfg.mrope_section = sections
            eng = Engine.from_model_config(cfg, max_batch_size=B, session_len=ctx + steps + 8, quant_policy=8, cache_max_entry_count=0.5)
            eng.init_synthetic(seed=0)
            eng.start()
            eng.prefill(prompts, max_new_tokens=steps + 4)
            eng.decode(3)          # eager step + capture + one replay
            eng.sync()
            t0 = time.perf_counter()
            eng.decode(steps)
            eng.sync()
            res.setdefault(name, []).append((time.perf_counter() - t0) / steps * 1e6)
            eng.close()
    for name, xs in res.items():
        print(f'engine decode step, batch {B}, context {ctx}, {name:17s}: median {median(xs):8.1f} us  min {min(xs):8.1f} us  '
              f'({median(xs) / median(res["without sections"]):.4f} of the engine without)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    for f in ('store', 'embedding', 'engine'):
        ap.add_argument('--' + f, action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mrope.py needs a GPU'
    tm = _ffi.load()
    every = not (a.store or a.embedding or a.engine)
    if a.store or every:
        bench_store(tm, a)
    if a.embedding or every:
        bench_embedding(tm, a)
    if a.engine or every:
        bench_engine(tm, a)


if __name__ == '__main__':
    main()
