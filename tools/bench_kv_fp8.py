#!/usr/bin/env python
"""Decode-attention kernel time of the FP8 KV cache (quant_policy 16, attention_decode_fp8_mfma.hip) next to int8 KV on the window /
sink MFMA kernel (tm_decode_attention_window_mfma) and on the head_dim-128 int8 MFMA kernel (tm_decode_attention), at Llama-3-8B
geometry (32 q / 8 kv heads of 128), batch 64, on random cache contents.  python tools/bench_kv_fp8.py [--ctx 1024,4096] [--rounds 5]

One process; every round times the arms in turn (device events around each launch, the median of --iters launches per arm and round, over
--layers pool layers so consecutive launches read different cache bytes).  Bytes per launch are the cache bytes each policy has to read:
batch x ctx x 2 x kv_heads x (head_dim [+ 4 for int8]).  One more line times head_dim 64 (FP8 against int8 on the window / sink kernel)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402


def bench(tm, D, ctx, arms, a):
    B, Hq, Hkv, layers = a.batch, a.hq, a.hkv, a.layers
    nblk = (ctx + 63) // 64
    st = torch.cuda.current_stream().cuda_stream
    cu = torch.arange(0, (B + 1) * nblk, nblk, dtype=torch.int32, device='cuda')
    klen = torch.full((B,), ctx, dtype=torch.int32, device='cuda')
    q = torch.randn((B, Hq * D), device='cuda').half()
    out = torch.empty((B, Hq * D), device='cuda').half()
    ws = torch.empty(max(1, tm.tm_decode_attention_workspace(B, Hq, a.splits)), dtype=torch.uint8, device='cuda')
    state = {}
    for name, bits, _ in arms:
        if bits in state:
            continue
        lsz = tm.tm_kv_layer_size(Hkv, D, 64, bits)
        pool = torch.randint(0, 255, (B * nblk, layers, lsz), dtype=torch.uint8, device='cuda')
        if bits == 8:   # finite fp16 (scale, zero) words
            nparam = Hkv * 2 * 64 * 4
            prm = torch.empty((B * nblk, layers, nparam // 2), dtype=torch.float16, device='cuda').uniform_(0.01, 0.05)
            pool[:, :, lsz - nparam:] = prm.view(torch.uint8).view(B * nblk, layers, nparam)
        ptrs = (pool.data_ptr() + torch.randperm(B * nblk).to(torch.int64) * layers * lsz).cuda()
        state[bits] = (pool, ptrs, lsz)

    def launch(fn, bits, layer):
        _, ptrs, lsz = state[bits]
        view = _ffi.KvCache(ptrs.data_ptr(), cu.data_ptr(), layer * lsz, Hkv, D, 64, bits, 0.05, 0.05)
        if fn == 'mfma':
            return tm.tm_decode_attention_window_mfma(out.data_ptr(), q.data_ptr(), Hq * D, klen.data_ptr(), B, Hq, 0.0, a.splits, ws.data_ptr(),
                                                      view, 0, None, st)
        return tm.tm_decode_attention(out.data_ptr(), q.data_ptr(), Hq * D, klen.data_ptr(), B, Hq, 0.0, a.splits, ws.data_ptr(), view, st)

    for rnd in range(a.rounds):
        for name, bits, fn in arms:
            for i in range(4):   # warm-up: code-object load and clocks
                _ffi.check(launch(fn, bits, i % layers))
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for i, (e0, e1) in enumerate(ev):
                e0.record()
                _ffi.check(launch(fn, bits, i % layers))
                e1.record()
            torch.cuda.synchronize()
            med = sorted(x.elapsed_time(y) for x, y in ev)[len(ev) // 2]
            nbytes = B * ctx * 2 * Hkv * (D + (4 if bits == 8 else 0))
            gbs = nbytes / (med * 1e-3) / 1e9
            print(f'head_dim={D} batch={B} ctx={ctx} splits={a.splits} round={rnd} {name:22s}: {med * 1e3:8.1f} us  {gbs:7.0f} GB/s = '
                  f'{gbs / 8000:.3f} of 8 TB/s ({nbytes / 1e6:.1f} MB/launch)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ctx', default='1024,4096')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--hq', type=int, default=32)
    ap.add_argument('--hkv', type=int, default=8)
    ap.add_argument('--splits', type=int, default=1)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--layers', type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: this tool measures, it does not fall back')
    tm = _ffi.load()
    ctxs = [int(c) for c in a.ctx.split(',')]
    for ctx in ctxs:
        bench(tm, 128, ctx, [('fp8 (fp8 mfma)', _ffi.KV_BITS_FP8, 'default'), ('int8 (window/sink mfma)', 8, 'mfma'),
                             ('int8 (head_dim-128 mfma)', 8, 'default')], a)
    bench(tm, 64, ctxs[-1], [('fp8 (fp8 mfma)', _ffi.KV_BITS_FP8, 'default'), ('int8 (window/sink mfma)', 8, 'mfma')], a)


if __name__ == '__main__':
    main()
