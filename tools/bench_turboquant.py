#!/usr/bin/env python
"""TurboQuant KV cache (quant_policy 42) next to int4 and int8 at the Llama-3-8B geometry (32 q / 8 kv heads of 128, batch 64).

  python tools/bench_turboquant.py [--attention] [--store] [--engine] [--ctx 1024,4096,16384] [--rounds 5] [--iters 20]

--attention  decode-attention time per launch for KV bits 42 / 4 / 8 on random cache contents: the variants are timed interleaved,
             round after round, in this one process (a median of --iters launches each; the median and minimum over the rounds are
             printed), over several layers of the pool so that consecutive launches read cold bytes.  Next to each time: the bytes the
             launch must read (codes + norms of every cached token) over 8 TB/s, as a fraction of the time.
--store      tm_kv_rope_store and tm_flatten_kv (transposed V) time per token, bits 42 against 4.
--engine     decode tok/s of the synthetic Llama-3-8B W4A16 model at quant_policy 4 and 42, and the KV blocks the pool gets when memory
             bounds it (--pool: only those).
No section given: all three.  Everything is measured with device events around launches, or a host clock around work that ends in a
device synchronise; without a GPU the tool fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402

HBM = 8e12      # bytes / s
ROW = {42: 64 + 32 + 8, 4: 2 * (64 + 4), 8: 2 * (128 + 4), 16: 2 * 256}     # bytes per token and kv head at head_dim 128


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    return median([a.elapsed_time(b) for a, b in ev]) * 1e3       # us


class Pool:
    """random cache blocks with finite fp16 norms / (scale, zero) pairs; `layers` layers so that launches rotate over cold bytes"""

    def __init__(self, tm, B, Hkv, ctx, bits, layers):
        self.lsz = tm.tm_kv_layer_size(Hkv, 128, 64, bits)
        self.nblk = (ctx + 63) // 64
        self.B, self.Hkv, self.bits, self.layers = B, Hkv, bits, layers
        self.pool = torch.randint(0, 255, (B * self.nblk, layers, self.lsz), dtype=torch.uint8, device='cuda')
        if bits != 16:
            nparam = Hkv * 2 * 64 * 4
            prm = torch.empty((B * self.nblk, layers, nparam // 2), dtype=torch.float16, device='cuda').uniform_(0.01, 0.05)
            self.pool[:, :, self.lsz - nparam:] = prm.view(torch.uint8).view(B * self.nblk, layers, nparam)
        perm = torch.randperm(B * self.nblk)
        self.ptrs = (self.pool.data_ptr() + perm.to(torch.int64) * layers * self.lsz).cuda()
        self.cu = torch.arange(0, (B + 1) * self.nblk, self.nblk, dtype=torch.int32, device='cuda')

    def view(self, i):
        return _ffi.KvCache(self.ptrs.data_ptr(), self.cu.data_ptr(), (i % self.layers) * self.lsz, self.Hkv, 128, 64, self.bits)


def bench_attention(tm, a):
    B, Hq, Hkv = a.batch, 32, 8
    st = torch.cuda.current_stream().cuda_stream
    q = torch.randn((B, Hq * 128), device='cuda').half()
    out = torch.empty((B, Hq * 128), device='cuda').half()
    for ctx in [int(c) for c in a.ctx.split(',')]:
        klen = torch.full((B,), ctx, dtype=torch.int32, device='cuda')
        arms = {}
        for bits in (42, 4, 8):
            for splits in (1, 2, 4):
                arms[(bits, splits)] = None
        pools = {bits: Pool(tm, B, Hkv, ctx, bits, a.layers) for bits in (42, 4, 8)}
        ws = torch.empty(max(1, tm.tm_decode_attention_workspace(B, Hq, 4)), dtype=torch.uint8, device='cuda')

        def launch(bits, splits, i):
            _ffi.check(tm.tm_decode_attention(out.data_ptr(), q.data_ptr(), Hq * 128, klen.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(),
                                              pools[bits].view(i), st))
        res = {k: [] for k in arms}
        for k in arms:      # warm-up: code objects and clocks
            for i in range(4):
                launch(k[0], k[1], i)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k in arms:
                res[k].append(timed(lambda i: launch(k[0], k[1], i), a.iters))
        best = {}
        for bits in (42, 4, 8):
            splits = min((1, 2, 4), key=lambda s: median(res[(bits, s)]))
            med, mn = median(res[(bits, splits)]), min(res[(bits, splits)])
            nbytes = B * ctx * Hkv * ROW[bits]
            best[bits] = med
            print(f'attention ctx={ctx} bits={bits:2d} splits={splits}: median {med:8.1f} us  min {mn:8.1f} us  {nbytes / 1e6:7.1f} MB -> '
                  f'{nbytes / HBM * 1e6:6.1f} us at 8 TB/s = {nbytes / HBM * 1e6 / med:.3f} of the time   '
                  f'(all splits, median us: ' + ', '.join(f'{s}: {median(res[(bits, s)]):.1f}' for s in (1, 2, 4)) + ')', flush=True)
        print(f'attention ctx={ctx}: bits 42 / bits 4 = {best[42] / best[4]:.3f} (bytes alone: {ROW[42] / ROW[4]:.3f}), '
              f'bits 42 / bits 8 = {best[42] / best[8]:.3f} (bytes alone: {ROW[42] / ROW[8]:.3f})', flush=True)
        del pools


def bench_store(tm, a):
    B, Hq, Hkv = a.batch, 32, 8
    st = torch.cuda.current_stream().cuda_stream
    new, ctx = 128, 4096
    T = B * new
    qkv = torch.randn((T, (Hq + 2 * Hkv) * 128), device='cuda').half()
    cu_q = torch.arange(0, T + 1, new, dtype=torch.int32, device='cuda')
    klen = torch.full((B,), new, dtype=torch.int32, device='cuda')
    tab = np.zeros((new + 1, 64, 2), np.float16)
    _ffi.check(tm.tm_rope_table(tab.ctypes.data, new + 1, 128, 500000.0, 2, 8.0, 1.0, 4.0, 8192))
    tab_d = torch.from_numpy(tab).cuda()
    Bf = 8
    klen_f = torch.full((Bf,), ctx, dtype=torch.int32, device='cuda')
    koff = torch.arange(0, (Bf + 1) * ctx, ctx, dtype=torch.int32, device='cuda')
    kf = torch.empty((Hkv, Bf * ctx, 128), dtype=torch.float16, device='cuda')
    vf = torch.empty((Hkv, 128, Bf * ctx), dtype=torch.float16, device='cuda')
    pools = {bits: (Pool(tm, B, Hkv, new, bits, a.layers), Pool(tm, Bf, Hkv, ctx, bits, a.layers)) for bits in (42, 4)}

    def store(bits, i):
        _ffi.check(tm.tm_kv_rope_store(qkv.data_ptr(), Hq, cu_q.data_ptr(), klen.data_ptr(), B, T, tab_d.data_ptr(), new + 1,
                                       pools[bits][0].view(i), st))

    def flatten(bits, i):
        _ffi.check(tm.tm_flatten_kv(kf.data_ptr(), vf.data_ptr(), 1, koff.data_ptr(), klen_f.data_ptr(), Bf, ctx, Bf * ctx,
                                    pools[bits][1].view(i), st))
    res = {}
    for fn, name in ((store, 'store'), (flatten, 'flatten')):
        for bits in (42, 4):
            for i in range(4):
                fn(bits, i)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for bits in (42, 4):
                res.setdefault((name, bits), []).append(timed(lambda i: fn(bits, i), a.iters))
    for name, tokens in (('store', T), ('flatten', Bf * ctx)):
        for bits in (42, 4):
            med = median(res[(name, bits)])
            print(f'{name:7s} bits={bits:2d}: median {med:8.1f} us  min {min(res[(name, bits)]):8.1f} us for {tokens} tokens x {Hkv} kv heads '
                  f'= {med * 1e3 / tokens:.2f} ns per token', flush=True)
        print(f'{name}: bits 42 / bits 4 = {median(res[(name, 42)]) / median(res[(name, 4)]):.3f}', flush=True)


def bench_engine(a):
    from lmdeploy_amd.pipeline import SYNTHETIC
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.engine import Engine
    cfg = checkpoint.ModelConfig(**SYNTHETIC['llama3_8b'])
    ctx, warm, steps, rounds = a.engine_ctx, 8, 64, 3
    for qp in ((4, 42, 4, 42) if a.engine else ()):      # alternating
        eng = Engine.from_model_config(cfg, max_batch_size=a.batch, session_len=ctx + warm + rounds * steps + 8, quant_policy=qp,
                                       max_prefill_token_num=8192, use_graph=1)
        eng.init_synthetic(seed=1)
        eng.start()
        stats = eng.stats()
        rng = np.random.default_rng(0)
        eng.prefill([rng.integers(0, cfg.vocab, ctx).astype(np.int32) for _ in range(a.batch)], max_new_tokens=warm + rounds * steps + 1)
        eng.decode(warm)
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.decode(steps)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
        eng.close()
        med = median(ms)
        print(f'engine llama3_8b W4A16 batch {a.batch} ctx {ctx} quant_policy {qp:2d}: {med:.3f} ms per step (rounds '
              f'{[round(x, 3) for x in ms]}) = {a.batch / med * 1e3:.0f} tok/s; pool {stats["num_blocks"]} blocks (what the batch can own), '
              f'{stats["kv_bytes_per_token"]} KV bytes per token, decode_splits {stats["decode_splits"]}', flush=True)
    # the blocks the pool GETS when memory, not the batch, bounds it: a session so long that batch x blocks per sequence exceeds
    # cache_max_entry_count x free memory (nothing is run on these engines)
    for qp in (4, 42):
        eng = Engine.from_model_config(cfg, max_batch_size=a.batch, session_len=a.pool_session_len, quant_policy=qp,
                                       max_prefill_token_num=8192, use_graph=1)
        eng.init_synthetic(seed=1)
        eng.start()
        stats = eng.stats()
        eng.close()
        print(f'pool llama3_8b W4A16 batch {a.batch} session_len {a.pool_session_len} quant_policy {qp:2d}: {stats["num_blocks"]} blocks of 64 '
              f'tokens = {stats["num_blocks"] * 64} tokens ({stats["num_blocks"] * 64 * stats["kv_bytes_per_token"] / 2**30:.1f} GiB, '
              f'{stats["kv_bytes_per_token"]} bytes per token)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--attention', action='store_true')
    ap.add_argument('--store', action='store_true')
    ap.add_argument('--engine', action='store_true')
    ap.add_argument('--pool', action='store_true', help='only the memory-bound pool sizes of --engine')
    ap.add_argument('--ctx', default='1024,4096,16384')
    ap.add_argument('--engine-ctx', type=int, default=1024)
    ap.add_argument('--pool-session-len', type=int, default=262144,
                    help='--engine: session length of the engines that only report the memory-bound pool size')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_turboquant needs a GPU: nothing is measured without one')
    tm = _ffi.load()
    every = not (a.attention or a.store or a.engine or a.pool)
    if a.attention or every:
        bench_attention(tm, a)
    if a.store or every:
        bench_store(tm, a)
    if a.engine or a.pool or every:
        a.engine = a.engine or every
        bench_engine(a)


if __name__ == '__main__':
    main()
