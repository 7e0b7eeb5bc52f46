#!/usr/bin/env python
"""Launch the prefill attention kernel on random flattened KV: `--batch` prompts of `--len` tokens, no history.
    python tools/bench_prefill_attention.py [--head-dim 64|128] [--batch 8] [--len 1024] [--hq 32] [--hkv 8] [--iters 20]
Prints the median launch time from device events; run it under `rocprofv3 --kernel-trace --stats` for the kernel time."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--head-dim', type=int, default=128, choices=[64, 128])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--len', type=int, default=1024)
    ap.add_argument('--hq', type=int, default=32)
    ap.add_argument('--hkv', type=int, default=8)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    tm = _ffi.load()
    B, n, Hq, Hkv, D = a.batch, a.len, a.hq, a.hkv, a.head_dim
    pad = (n + 63) // 64 * 64
    stride = B * pad
    torch.manual_seed(0)
    q = torch.randn((B * n, Hq * D), device='cuda').half()
    k = torch.randn((Hkv, stride, D), device='cuda').half()
    vt = torch.randn((Hkv, D, stride), device='cuda').half()
    out = torch.empty((B * n, Hq * D), device='cuda').half()
    cu = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device='cuda')
    koff = torch.arange(0, (B + 1) * pad, pad, dtype=torch.int32, device='cuda')
    klen = torch.full((B,), n, dtype=torch.int32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        _ffi.check(tm.tm_prefill_attention_hd(out.data_ptr(), q.data_ptr(), Hq * D, k.data_ptr(), vt.data_ptr(), stride, cu.data_ptr(),
                                              koff.data_ptr(), klen.data_ptr(), B, n, Hq, Hkv, D, 0.0, st))
    for _ in range(4):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        launch()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(x.elapsed_time(y) for x, y in ev)
    med = ts[len(ts) // 2]
    flops = 4.0 * B * Hq * D * n * (n + 1) / 2      # QK^T and PV over the causal half
    print(f'prefill attention head_dim={D} {B} x {n} tokens, {Hq}/{Hkv} heads: median {med * 1e3:.1f} us over {a.iters} launches '
          f'(min {ts[0] * 1e3:.1f}) = {flops / (med * 1e-3) / 1e12:.1f} TFLOP/s (causal)', flush=True)


if __name__ == '__main__':
    main()
