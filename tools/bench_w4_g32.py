#!/usr/bin/env python
"""Times the group-32 W4A16 linear (gemm_u4_g32.hip) against the group-128 kernels at the same (K, N).

GEMMs: (K, N) = 4096 x 6144 (w_qkv), 4096 x 4096 (wo), 4096 x 28672 gated (w1w3), 14336 x 4096 (w2) at M = 1, 16, 64 and 2048.
Both arms are tm_linear_forward on a u4 handle (group 32: the kernel's own split-K and reduce; group 128: the measured / heuristic
tiling of the AWQ kernels), as the engine runs them.  Every launch of a graph reads another of `--copies` weight copies (together more
bytes than the Infinity Cache holds, as in a decode step); n launches are captured into one graph, device events bracket one replay,
the two arms alternate repeat by repeat in one process; after three warm-up rounds the table gives the median and the range of
`--repeats` replays, the ratio of the medians, and the achieved fraction of the 8 TB/s HBM peak counting the bytes the checkpoint
carries: 4 bits per weight + one 32-bit (scale, zero) pair per group and column (K N / 2 + (K / g) N 4 bytes).

    python tools/bench_w4_g32.py [--out profiles/w4_g32.txt] [--repeats 9]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('w_qkv', 4096, 6144, False), ('wo', 4096, 4096, False), ('w1w3', 4096, 28672, True), ('w2', 14336, 4096, False)]
ROWS = (1, 16, 64, 2048)
GROUPS = (32, 128)
HBM_PEAK = 8.0e12


def weight_bytes(K, N, g):
    return K * N // 2 + (K // g) * N * 4


def bench(a, lines):
    import torch

    from lmdeploy_amd import _ffi
    tm = _ffi.load()
    torch.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    for M in ROWS:
        lines.append(f'# M = {M}: us per linear, median (min-max) of {a.repeats} graph replays; % = weight bytes / time over 8 TB/s')
        for name, K, N, gated in SHAPES:
            copies = a.copies if M <= 64 else 2
            handles = {g: [] for g in GROUPS}
            for _ in range(copies):
                qw = torch.randint(-2**31, 2**31 - 1, (K, N // 8), device='cuda', dtype=torch.int32)
                for g in GROUPS:
                    sc = (torch.rand((K // g, N), device='cuda') * 2e-3 + 1e-3).half()
                    zs = torch.full((K // g, N), 8.0, device='cuda', dtype=torch.float16)
                    h = C.c_void_p()
                    _ffi.check(tm.tm_linear_create(C.byref(h), K, N, 0, g))
                    _ffi.check(tm.tm_linear_prepare(h, qw.data_ptr(), sc.data_ptr(), zs.data_ptr(), st))
                    handles[g].append(h)
                torch.cuda.synchronize()
                del qw
            x = torch.randn((M, K), device='cuda').half()
            ldy = N // 2 if gated else N
            y = torch.empty((M, ldy), device='cuda', dtype=torch.float16)
            ws = torch.zeros((max(tm.tm_linear_workspace(handles[g][0], M) for g in GROUPS),), device='cuda', dtype=torch.uint8)
            n = 2 * copies if M <= 64 else 2

            def launch(g, i):
                s = torch.cuda.current_stream().cuda_stream
                _ffi.check(tm.tm_linear_forward(handles[g][i % copies], x.data_ptr(), K, y.data_ptr(), ldy, M, int(gated), 0, 0, 0,
                                                ws.data_ptr(), s))
            graphs = {}
            for g in GROUPS:
                launch(g, 0)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for i in range(n):
                        launch(g, i)
                graphs[g] = gr
            samples = {g: [] for g in GROUPS}
            for rep in range(-3, a.repeats):
                for g, gr in graphs.items():
                    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    gr.replay()
                    t.record()
                    t.synchronize()
                    if rep >= 0:
                        samples[g].append(s.elapsed_time(t) * 1e3 / n)
            med, cells = {}, []
            for g, v in samples.items():
                v.sort()
                med[g] = v[len(v) // 2]
                frac = weight_bytes(K, N, g) / (med[g] * 1e-6) / HBM_PEAK
                cells.append(f'g{g:<3} {med[g]:9.2f} ({v[0]:.2f}-{v[-1]:.2f}) {100 * frac:5.1f} %')
            lines.append(f'{name:<5} {K:>5} x {N:<5}{" gated" if gated else "      "} ' + '   '.join(cells) + f'   g32 / g128 {med[32] / med[128]:.3f}')
            del graphs
            for hs in handles.values():
                for h in hs:
                    tm.tm_linear_destroy(h)
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--copies', type=int, default=6)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_w4_g32.py needs a GPU')
    lines = []
    bench(a, lines)
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
