#!/usr/bin/env python
"""Time flatten_kv for one prefill chunk behind a long history: one layer, one sequence of --hist cached tokens + a --chunk of new ones
(random cache bytes, finite dequantisation parameters; --layers cache layers rotated so that consecutive launches read cold bytes;
4 warm-up + --iters timed launches, device events, the median).
--window 0 times tm_flatten_kv, the whole context.  --window W > 0 times tm_flatten_kv_window: the tiles in front of
max(hist - W + 1, 0) are skipped, so the time follows W + chunk instead of hist + chunk.
python tools/bench_flatten.py --hist 31744 --chunk 1024 --window 4096 [--hkv 8] [--head-dim 128] [--bits 8]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hist', type=int, default=31744)
    ap.add_argument('--chunk', type=int, default=1024)
    ap.add_argument('--window', type=int, default=0)
    ap.add_argument('--hkv', type=int, default=8)
    ap.add_argument('--bits', type=int, default=8)
    ap.add_argument('--head-dim', type=int, default=128, choices=[64, 128])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--tag', default='')
    a = ap.parse_args()
    tm = _ffi.load()
    Hkv, D, bits, layers = a.hkv, a.head_dim, a.bits, a.layers
    ctx = a.hist + a.chunk
    nblk = (ctx + 63) // 64
    lsz = tm.tm_kv_layer_size(Hkv, D, 64, bits)
    pool = torch.randint(0, 255, (nblk, layers, lsz), dtype=torch.uint8, device='cuda')
    if bits < 16:       # finite (scale, zero) words
        nparam = Hkv * 2 * 64 * 4
        prm = torch.empty((nblk, layers, nparam // 2), dtype=torch.float16, device='cuda').uniform_(0.01, 0.05)
        pool[:, :, lsz - nparam:] = prm.view(torch.uint8).view(nblk, layers, nparam)
    ptrs = (pool.data_ptr() + torch.randperm(nblk).to(torch.int64) * layers * lsz).cuda()
    cu_blk = torch.tensor([0, nblk], dtype=torch.int32, device='cuda')
    stride = nblk * 64 + 64
    kf = torch.empty((Hkv, stride, D), dtype=torch.float16, device='cuda')
    vf = torch.empty((Hkv, D, stride), dtype=torch.float16, device='cuda')
    koff = torch.tensor([0, nblk * 64], dtype=torch.int32, device='cuda')
    klen = torch.tensor([ctx], dtype=torch.int32, device='cuda')
    cu_q = torch.tensor([0, a.chunk], dtype=torch.int32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def flatten(layer):
        view = _ffi.KvCache(ptrs.data_ptr(), cu_blk.data_ptr(), layer * lsz, Hkv, D, 64, bits)
        head = (kf.data_ptr(), vf.data_ptr(), 1, koff.data_ptr(), klen.data_ptr(), 1, ctx, stride, view)
        if a.window > 0:
            return tm.tm_flatten_kv_window(*head, cu_q.data_ptr(), a.window, st)
        return tm.tm_flatten_kv(*head, st)

    for i in range(4):
        _ffi.check(flatten(i % layers))
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        _ffi.check(flatten(i % layers))
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(x.elapsed_time(y) for x, y in ev)
    med = ts[len(ts) // 2]
    first = max(a.hist - a.window + 1, 0) // 64 * 64 if a.window > 0 else 0
    print(f'{a.tag}head_dim={D} hkv={Hkv} bits={bits} hist={a.hist} chunk={a.chunk} window={a.window}: {med * 1e3:8.1f} us  '
          f'(min {ts[0] * 1e3:.1f}, {ctx - first} of {ctx} tokens flattened)', flush=True)


if __name__ == '__main__':
    main()
