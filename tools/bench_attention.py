#!/usr/bin/env python
"""Time the paged decode attention kernel at the metric shape (B=64, 32 q / 8 kv heads, int8 KV) on random cache
contents.  python tools/bench_attention.py [--ctx 1536] [--bits 8] [--splits 1,2,4] [--head-dim 128]
--head-dim 64 times the head_dim 64 kernel (VALU, every KV width); set TM_ATTN_VALU=1 to time the same kernel family at head_dim 128.
--window W times tm_decode_attention_window (the VALU kernel's sliding-window variant, both head dims): the bytes per launch are those
of the last min(ctx, W) tokens; --sinks adds one sink logit per head to it.
--rounds N repeats every measurement (a median of --iters launches each) N times in this one process.
--engine-decode times whole decode steps of a SYNTHETIC Llama-3.2-1B geometry instead (tm_engine_init_synthetic weights, int8 KV)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lmdeploy_amd import _ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ctx', type=int, default=1536)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--hq', type=int, default=32)
    ap.add_argument('--hkv', type=int, default=8)
    ap.add_argument('--bits', type=int, default=8)
    ap.add_argument('--head-dim', type=int, default=128, choices=[64, 128])
    ap.add_argument('--engine-decode', action='store_true',
                    help='decode tok/s of a synthetic Llama-3.2-1B geometry (2048 / 16 layers / 32 x 8 heads of 64 / 8192 / 128256)')
    ap.add_argument('--window', type=int, default=0, help='sliding window (0 = none): tm_decode_attention_window')
    ap.add_argument('--sinks', action='store_true', help='with --window: attention sinks (one logit per head)')
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--splits', default='1,2,4')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--layers', type=int, default=4, help='layers stored in the pool (32 = the engine\'s block stride)')
    ap.add_argument('--layout', default='block', choices=['block', 'layer'],
                    help='block: [block][layer] (reference: all layers of a block contiguous); layer: [layer][block]')
    a = ap.parse_args()
    if a.engine_decode:
        return engine_decode(a.batch, a.ctx, a.bits)
    tm = _ffi.load()
    B, Hq, Hkv, ctx, bits, D = a.batch, a.hq, a.hkv, a.ctx, a.bits, a.head_dim
    layers = a.layers   # several layers so that consecutive launches touch different (cold) cache bytes
    lsz = tm.tm_kv_layer_size(Hkv, D, 64, bits)
    nblk = (ctx + 63) // 64
    pool = torch.randint(0, 255, (B * nblk, layers * lsz), dtype=torch.uint8, device='cuda')
    # make the per-token (scale, zero) params finite fp16 values
    pv = pool.view(B * nblk, layers, lsz) if a.layout == 'block' else pool.view(-1).view(layers, B * nblk, lsz)
    if bits < 16:
        nparam = Hkv * 2 * 64 * 4
        prm = torch.empty((pv.shape[0], pv.shape[1], nparam // 2), dtype=torch.float16, device='cuda').uniform_(0.01, 0.05)
        pv[:, :, lsz - nparam:] = prm.view(torch.uint8).view(pv.shape[0], pv.shape[1], nparam)
    perm = torch.randperm(B * nblk)
    if a.layout == 'block':
        ptrs_of = lambda layer: (pool.data_ptr() + perm.to(torch.int64) * layers * lsz).cuda()   # + layer offset in the view
        off_of = lambda layer: layer * lsz
    else:   # layer-major: the same bytes, block b of layer l at (l * nblocks + b) * lsz
        ptrs_of = lambda layer: (pool.data_ptr() + (layer * B * nblk + perm.to(torch.int64)) * lsz).cuda()
        off_of = lambda layer: 0
    tables = [ptrs_of(l) for l in range(layers)]
    ptrs = tables[0]
    cu = torch.arange(0, (B + 1) * nblk, nblk, dtype=torch.int32, device='cuda')
    klen = torch.full((B,), ctx, dtype=torch.int32, device='cuda')
    q = torch.randn((B, Hq * D), device='cuda').half()
    out = torch.empty((B, Hq * D), device='cuda').half()
    st = torch.cuda.current_stream().cuda_stream
    seen = min(ctx, a.window) if a.window > 0 else ctx
    bytes_per_launch = B * seen * 2 * Hkv * (D * bits // 8 + (4 if bits < 16 else 0))

    sinks = torch.empty(Hq, device='cuda').uniform_(-2.0, 4.0).half() if a.sinks else None

    def attend(splits, ws, view):
        if a.window > 0:
            return tm.tm_decode_attention_window(out.data_ptr(), q.data_ptr(), Hq * D, klen.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(),
                                                 view, a.window, sinks.data_ptr() if a.sinks else None, st)
        return tm.tm_decode_attention(out.data_ptr(), q.data_ptr(), Hq * D, klen.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(), view, st)
    if a.trace:
        # in-kernel phase stamps (100 MHz): start / prologue done (q ready, first block issued) / wave 0 done /
        # all waves done / end, per workgroup
        splits = int(a.splits.split(',')[0])
        ws = torch.empty(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
        dbg = torch.zeros((8192, 8), dtype=torch.int64, device='cuda')
        for it in range(4):
            dbg.zero_()
            torch.cuda.synchronize()
            tm.tm_debug_set_gemm_trace(dbg.data_ptr())
            view = _ffi.KvCache(tables[it % layers].data_ptr(), cu.data_ptr(), off_of(it % layers), Hkv, D, 64, bits)
            _ffi.check(tm.tm_decode_attention(out.data_ptr(), q.data_ptr(), Hq * D, klen.data_ptr(), B, Hq, 0.0, splits,
                                              ws.data_ptr(), view, st))
            tm.tm_debug_set_gemm_trace(None)
            torch.cuda.synchronize()
            raw = dbg.cpu().numpy()
            t = raw[raw[:, 0] > 0].astype(np.float64) / 100.0
            t0 = t[:, 0].min()
            print(f'launch {it}: {len(t)} workgroups, span {t[:, 3].max() - t0:.2f} us')
            for name, v in (('start skew', t[:, 0] - t0), ('prologue', t[:, 1] - t[:, 0]), ('wave0 loop', t[:, 2] - t[:, 1]),
                            ('wait waves', t[:, 5] - t[:, 2]), ('merge+store', t[:, 3] - t[:, 5]), ('end time', t[:, 3] - t0)):
                print(f'  {name:11s} min {v.min():6.2f}  mean {v.mean():6.2f}  p90 {np.percentile(v, 90):6.2f}  max {v.max():6.2f} us')
            # where do the late workgroups sit?  end time by XCD, by CU, by (sequence, kv head)
            live = raw[raw[:, 0] > 0]
            end = live[:, 3].astype(np.float64) / 100.0 - t0
            xcc = ((live[:, 4] >> 32) & 0xf).astype(int)
            hw = (live[:, 4] & 0xffffffff).astype(np.int64)
            cuid = ((hw >> 8) & 0xf) | (((hw >> 13) & 0x7) << 4) | (xcc << 7)      # CU_ID | SE_ID << 4 | XCC << 7
            start = live[:, 0].astype(np.float64) / 100.0 - t0
            print('  end time by XCD: ' + '  '.join(f'{x}: {end[xcc == x].mean():5.1f} (n {int((xcc == x).sum())})' for x in range(8)))
            print('  start    by XCD: ' + '  '.join(f'{x}: {start[xcc == x].mean():5.2f}' for x in range(8)))
            print('  max end  by XCD: ' + '  '.join(f'{x}: {end[xcc == x].max():5.1f}' for x in range(8)))
            per_cu = {}
            for c, e_ in zip(cuid, end):
                per_cu.setdefault(int(c), []).append(e_)
            occ = np.bincount([len(v) for v in per_cu.values()])
            print(f'  CUs used {len(per_cu)}; workgroups per CU histogram {occ.tolist()}; mean end of CUs with 1 / 2 / 3+ WGs: ' +
                  ' / '.join(f"{np.mean([np.max(v) for v in per_cu.values() if (len(v) if len(v) < 3 else 3) == k]) if any((len(v) if len(v) < 3 else 3) == k for v in per_cu.values()) else float('nan'):.1f}" for k in (1, 2, 3)))
            order = np.argsort(live[:, 0])
            nq4 = len(order) // 4
            print('  end time by launch-order quartile: ' + '  '.join(f'{end[order[i * nq4:(i + 1) * nq4]].mean():5.1f}' for i in range(4)))
        return
    for splits in [int(s) for s in a.splits.split(',')]:
        ws = torch.empty(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
        for rnd in range(a.rounds):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for i in range(4):   # warm-up: code-object load and clocks, outside the timed launches
                view = _ffi.KvCache(tables[i % layers].data_ptr(), cu.data_ptr(), off_of(i % layers), Hkv, D, 64, bits)
                _ffi.check(attend(splits, ws, view))
            torch.cuda.synchronize()
            for i, (e0, e1) in enumerate(ev):
                view = _ffi.KvCache(tables[i % layers].data_ptr(), cu.data_ptr(), off_of(i % layers), Hkv, D, 64, bits)
                e0.record()
                _ffi.check(attend(splits, ws, view))
                e1.record()
            torch.cuda.synchronize()
            ts = sorted(x.elapsed_time(y) for x, y in ev)
            med = ts[len(ts) // 2]
            gbs = bytes_per_launch / (med * 1e-3) / 1e9
            tag = f' round={rnd}' if a.rounds > 1 else ''
            print(f'head_dim={D} ctx={ctx} window={a.window} bits={bits} splits={splits}{tag}: {med*1e3:8.1f} us  {gbs:7.0f} GB/s = '
                  f'{gbs / 8000:.3f} of 8 TB/s ({bytes_per_launch/1e6:.1f} MB/launch)  layout={a.layout} layers={layers}', flush=True)


def engine_decode(batch, ctx, bits, warmup=8, steps=64, rounds=3):
    """decode steps of a synthetic Llama-3.2-1B geometry (random u4 weights: the speed of the shape, not of a checkpoint)"""
    import time

    from lmdeploy_amd.turbomind.engine import Engine
    from oracle import tm_oracle as o
    cfg = o.ModelConfig(hidden=2048, layers=16, q_heads=32, kv_heads=8, head_dim=64, inter=8192, vocab=128256, kv_bits=bits,
                        rope=o.RopeParam(64, 500000.0, 'llama3', 32.0, 1.0, 4.0, 8192))
    eng = Engine.from_model_config(cfg, max_batch_size=batch, session_len=ctx + warmup + rounds * steps + 8,
                                   quant_policy=0 if bits == 16 else bits, max_prefill_token_num=8192, use_graph=1)
    eng.init_synthetic(seed=1)
    eng.start()
    rng = np.random.default_rng(0)
    eng.prefill([rng.integers(0, cfg.vocab, ctx).astype(np.int32) for _ in range(batch)], max_new_tokens=warmup + rounds * steps + 1)
    eng.decode(warmup)
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.decode(steps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    eng.close()
    med = sorted(ms)[len(ms) // 2]
    print(f'synthetic Llama-3.2-1B geometry, head_dim 64, batch {batch}, ctx {ctx}, kv bits {bits}: {med:.3f} ms per decode step '
          f'(rounds {[round(x, 3) for x in ms]}) = {batch / med * 1e3:.0f} tok/s', flush=True)


if __name__ == '__main__':
    main()
