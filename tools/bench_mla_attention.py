"""Times tm_mla_attention (csrc/attention_mla.hip) in decode: batch 64, context 1024 and 4096, H = 16 and 128, with the split count
lmdeploy_amd.mla.default_splits picks.  Prints one JSON line per shape: microseconds per call (device events around `--iters` calls
after `--warmup`, best and median of `--repeats` windows) and the achieved bytes/s over the ALGORITHMIC bytes batch x ctx x 1152 x
chunks per sequence (a workgroup reads its sequence's latent once per 16 score columns), with its share of 8 TB/s.
--fp8: every row is run on the fp16 latent view and on the FP8 one (csrc/attention_mla_fp8.hip: 640-byte rows, the same tokens'
algorithmic bytes at 640 per row), one JSON line per view with the field `view`; with --prefill too.
--prefill: one prompt per call (`--shapes q_len:hist`) through tm_mla_attention and through the expanded path (tm_mla_flatten, the
expansion einsums, tm_mla_prefill_attention: timed apart and summed), one JSON line per shape and H; see prefill().
Needs a GPU; there is no fallback."""
import argparse
import json
import statistics

import numpy as np
import torch

from lmdeploy_amd import _ffi, mla

ROW, RANK, HBM = 576, 512, 8.0e12
K_SCALE = 0.0123   # the FP8 view's latent scale: N(0, 1) rows use the codes' range up to ~400 of 448


def _pool(tm, nblk, bits):
    """(pool of nblk blocks of N(0, 1) latent rows as the view `bits` stores them, bytes of a layer = of a block here, k_scale)"""
    if bits == 16:
        layer = tm.tm_mla_layer_size(64, RANK, 64)
        return torch.randn((nblk, layer // 2), dtype=torch.float16, device='cuda'), layer, 0.0
    rows = torch.randn((nblk * 64, ROW), device='cuda')
    codes = (rows[:, :RANK] / K_SCALE).clamp(-448.0, 448.0).cpu().to(torch.float8_e4m3fn).view(torch.uint8).cuda()   # cast on the host
    pool = torch.cat([codes, rows[:, RANK:].half().contiguous().view(torch.uint8)], 1).reshape(nblk, -1).contiguous()
    return pool, tm.tm_mla_layer_size_fp8(64, RANK, 64), K_SCALE


def _view(ptrs, cu_blk, bits, k_scale):
    c = _ffi.KvCache(ptrs.data_ptr(), cu_blk.data_ptr(), 0, 1, ROW, 64, bits)
    c.k_scale = k_scale
    return c


def _timed(fn, warmup, repeats, budget_s=0.25):
    """microseconds per call: `repeats` windows of device events after `warmup` calls; the window is sized to ~budget_s"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    iters = int(max(3, min(200, budget_s * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    us = []
    for _ in range(repeats):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {'median': round(statistics.median(us), 2), 'min': round(min(us), 2), 'max': round(max(us), 2), 'iters': iters}


def prefill(a):
    """One prompt per call through both kernels on the same latent pool: tm_mla_attention as mla_forward calls it (default_splits, its
    length read-back included) against tm_mla_flatten + the two expansion einsums + tm_mla_prefill_attention, each part timed on its
    own and summed.  `--shapes` are q_len:hist pairs.  PFLOP/s of the new kernel counts 640 flop per (row, head, key) over the causal
    region."""
    tm = _ffi.load()
    st = torch.cuda.current_stream().cuda_stream
    for shape, bits in ((s, b) for s in a.shapes for b in a.views):
        q_len, hist = (int(x) for x in shape.split(':'))
        ctx = q_len + hist
        nblk = -(-ctx // 64)
        pool, layer, k_scale = _pool(tm, nblk, bits)
        ptrs = (pool.data_ptr() + torch.randperm(nblk).to(torch.int64) * layer).cuda()
        cu_blk = torch.tensor([0, nblk], dtype=torch.int32, device='cuda')
        cache = _view(ptrs, cu_blk, bits, k_scale)
        cu_q = torch.tensor([0, q_len], dtype=torch.int32, device='cuda')
        k_len = torch.tensor([ctx], dtype=torch.int32, device='cuda')
        k_off = torch.zeros(1, dtype=torch.int32, device='cuda')
        for H in a.heads:
            W_UK = (torch.randn((H, 128, RANK), device='cuda') / RANK ** 0.5).half()
            W_UV = (torch.randn((H, RANK, 128), device='cuda') / RANK ** 0.5).half()
            # absorbed
            splits = mla.default_splits(1, q_len, H, ctx)
            q = (0.6 * torch.randn((q_len, H * ROW), device='cuda')).half()
            o_lat = torch.empty((q_len, H * RANK), dtype=torch.float16, device='cuda')
            ws = torch.empty(max(1, tm.tm_mla_attention_workspace(q_len, H, splits)), dtype=torch.uint8, device='cuda')
            t_abs = _timed(lambda: _ffi.check(tm.tm_mla_attention(o_lat.data_ptr(), q.data_ptr(), H * ROW, cu_q.data_ptr(), k_len.data_ptr(), 1,
                                                                  H, 192 ** -0.5, splits, ws.data_ptr(), cache, st)), a.warmup, a.repeats)
            del q, o_lat, ws
            # expanded
            qx = (0.6 * torch.randn((q_len, H * 192), device='cuda')).half()
            lat = torch.empty((ctx, ROW), dtype=torch.float16, device='cuda')
            kv = torch.empty((ctx, H, 256), dtype=torch.float16, device='cuda')
            out = torch.empty((q_len, H * 128), dtype=torch.float16, device='cuda')

            def flatten():
                _ffi.check(tm.tm_mla_flatten(lat.data_ptr(), k_off.data_ptr(), k_len.data_ptr(), 1, ctx, cache, st))

            def expand():
                kv[:, :, :128].copy_(torch.einsum('tr,hdr->thd', lat[:, :RANK], W_UK))
                kv[:, :, 128:].copy_(torch.einsum('tr,hrv->thv', lat[:, :RANK], W_UV))

            def attend():
                _ffi.check(tm.tm_mla_prefill_attention(out.data_ptr(), qx.data_ptr(), H * 192, kv.data_ptr(), H * 256, lat.data_ptr() + RANK * 2,
                                                       ROW, cu_q.data_ptr(), k_off.data_ptr(), k_len.data_ptr(), 1, q_len, H, 192 ** -0.5, st))
            t_f, t_e, t_a = (_timed(f, a.warmup, a.repeats) for f in (flatten, expand, attend))
            assert np.isfinite(out.float().cpu().numpy()).all()
            flop = 640 * H * (q_len * hist + q_len * (q_len + 1) // 2)
            total = t_f['median'] + t_e['median'] + t_a['median']
            print(json.dumps({'op': 'mla_prefill', 'view': 'fp8' if bits != 16 else 'fp16', 'q_len': q_len, 'hist': hist, 'H': H, 'absorbed_splits': splits, 'absorbed_us': t_abs,
                              'flatten_us': t_f, 'expand_us': t_e, 'prefill_attention_us': t_a, 'expanded_sum_us_median': round(total, 2),
                              'prefill_attention_pflops': round(flop / (t_a['median'] * 1e-6) / 1e15, 4),
                              'absorbed_over_expanded': round(t_abs['median'] / total, 2)}), flush=True)
            del qx, lat, kv, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fp8', action='store_true', help='run every row on the FP8 latent view too')
    ap.add_argument('--prefill', action='store_true', help='time one prompt per call through the absorbed and the expanded path')
    ap.add_argument('--shapes', nargs='+', default=['1024:0', '4096:0', '1024:3072'], help='--prefill: q_len:hist pairs')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ctx', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--heads', type=int, nargs='+', default=[16, 128])
    ap.add_argument('--splits', type=int, default=0, help='0 = mla.default_splits')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mla_attention needs a GPU'
    a.views = [16, _ffi.KV_BITS_FP8] if a.fp8 else [16]
    if a.prefill:
        return prefill(a)
    tm, B = _ffi.load(), a.batch
    st = torch.cuda.current_stream().cuda_stream
    for ctx, bits in ((c, b) for c in a.ctx for b in a.views):
        nblk = -(-ctx // 64)
        pool, layer, k_scale = _pool(tm, B * nblk, bits)       # 64 x 4096 rows: 302 MB fp16, 168 MB FP8 -- at ctx 1024 the FP8 pool
        perm = torch.randperm(B * nblk)                        # (42 MB) is below the 256 MB last-level cache: read that row with care
        ptrs = (pool.data_ptr() + perm.to(torch.int64) * layer).cuda()
        cu_blk = torch.arange(0, (B + 1) * nblk, nblk, dtype=torch.int32, device='cuda')
        cache = _view(ptrs, cu_blk, bits, k_scale)
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
            nbytes = B * ctx * mla.row_bytes(bits) * chunks
            best = min(us)
            print(json.dumps({'op': 'tm_mla_attention', 'view': 'fp8' if bits != 16 else 'fp16', 'batch': B, 'ctx': ctx, 'H': H, 'splits': splits, 'us_best': round(best, 2),
                              'us_median': round(statistics.median(us), 2), 'algorithmic_bytes': nbytes,
                              'bytes_per_s': round(nbytes / (best * 1e-6), 0), 'frac_of_8TBps': round(nbytes / (best * 1e-6) / HBM, 3),
                              'note': 'call time: the entry reads cu_q_len / k_len back (one stream synchronise per call) and, with '
                                      'splits > 1, includes the reduce kernel'}))
            assert np.isfinite(out.float().cpu().numpy()).all()


if __name__ == '__main__':
    main()
