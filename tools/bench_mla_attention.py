"""Times tm_mla_attention (csrc/attention_mla.hip) in decode: batch 64, context 1024 and 4096, H = 16 and 128, with the split count
lmdeploy_amd.mla.default_splits picks.  Prints one JSON line per shape: microseconds per call (device events around `--iters` calls
after `--warmup`, best and median of `--repeats` windows) and the achieved bytes/s over the ALGORITHMIC bytes batch x ctx x 1152 x
chunks per sequence (a workgroup reads its sequence's latent once per 16 score columns), with its share of 8 TB/s.  Needs a GPU; there
is no fallback."""
import argparse
import json
import statistics

import numpy as np
import torch

from lmdeploy_amd import _ffi, mla

ROW, RANK, HBM = 576, 512, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ctx', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--heads', type=int, nargs='+', default=[16, 128])
    ap.add_argument('--splits', type=int, default=0, help='0 = mla.default_splits')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mla_attention needs a GPU'
    tm, B = _ffi.load(), a.batch
    st = torch.cuda.current_stream().cuda_stream
    for ctx in a.ctx:
        nblk = -(-ctx // 64)
        layer = tm.tm_mla_layer_size(64, RANK, 64)
        pool = torch.randn((B * nblk, layer // 2), dtype=torch.float16, device='cuda')       # 64 x 4096 rows: 302 MB, beyond any cache
        perm = torch.randperm(B * nblk)
        ptrs = (pool.data_ptr() + perm.to(torch.int64) * layer).cuda()
        cu_blk = torch.arange(0, (B + 1) * nblk, nblk, dtype=torch.int32, device='cuda')
        cache = _ffi.KvCache(ptrs.data_ptr(), cu_blk.data_ptr(), 0, 1, ROW, 64, 16)
        cu_q = torch.arange(B + 1, dtype=torch.int32, device='cuda')
        k_len = torch.full((B,), ctx, dtype=torch.int32, device='cuda')
        for H in a.heads:
            splits = a.splits or mla.default_splits(B, 1, H, ctx)
            q = (0.6 * torch.randn((B, H * ROW), device='cuda')).half()
            out = torch.empty((B, H * RANK), dtype=torch.float16, device='cuda')
            ws = torch.empty(max(1, tm.tm_mla_attention_workspace(B, H, splits)), dtype=torch.uint8, device='cuda')

            def call():
                _ffi.check(tm.tm_mla_attention(out.data_ptr(), q.data_ptr(), H * ROW, cu_q.data_ptr(), k_len.data_ptr(), B, H, 192 ** -0.5,
                                               splits, ws.data_ptr(), cache, st))
            for _ in range(a.warmup):
                call()
            us = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    call()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
            chunks = -(-H // 16)
            nbytes = B * ctx * ROW * 2 * chunks
            best = min(us)
            print(json.dumps({'op': 'tm_mla_attention', 'batch': B, 'ctx': ctx, 'H': H, 'splits': splits, 'us_best': round(best, 2),
                              'us_median': round(statistics.median(us), 2), 'algorithmic_bytes': nbytes,
                              'bytes_per_s': round(nbytes / (best * 1e-6), 0), 'frac_of_8TBps': round(nbytes / (best * 1e-6) / HBM, 3),
                              'note': 'call time: the entry reads cu_q_len / k_len back (one stream synchronise per call) and, with '
                                      'splits > 1, includes the reduce kernel'}))
            assert np.isfinite(out.float().cpu().numpy()).all()


if __name__ == '__main__':
    main()
