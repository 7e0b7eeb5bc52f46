#!/usr/bin/env python
"""Times the decode grouped expert GEMMs of an MXFP4 gpt-oss block against u4 (AWQ) experts of the same shape, launch by launch
(tm_moe_forward_stages, as tools/bench_moe_router.py): the gated w1w3 launch and the w2 launch.

Shape: hidden = inter = 2944 (23 x 128, the nearest legal shape to gpt-oss' 2880), 32 experts, top-4, 64 tokens.  Both formats move
4.25 bits per weight; the u4 kernels are the yardstick.  `n` copies of a launch are captured into one graph and device events bracket
one replay; the two formats alternate repeat by repeat in one process; after three warm-up rounds the table gives the median and the
range of `--repeats` replays, the MXFP4 / u4 ratio of the medians and the spread (max / min) of the repeated u4 runs.

    python tools/bench_moe_mxfp4.py [--out profiles/mxfp4_moe_ab.txt] [--repeats 9]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = I = 2944
E, K_TOP, T = 32, 4, 64
STAGES = [('w1w3', 4), ('w2', 8), ('forward', 31)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=9)
    a = ap.parse_args()
    import torch

    from lmdeploy_amd import _ffi
    tm = _ffi.load()
    torch.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    gate = (0.02 * torch.randn((H, E), device='cuda')).half()
    blocks = {}
    for fmt, wtype in (('u4', 0), ('mxfp4', 3)):
        h = C.c_void_p()
        _ffi.check(tm.tm_moe_create(C.byref(h), H, I, E, K_TOP, wtype, 1, 1.0))
        _ffi.check(tm.tm_moe_set_gate(h, gate.data_ptr(), st))
        if fmt == 'mxfp4':
            _ffi.check(tm.tm_moe_set_activation(h, 1))
            _ffi.check(tm.tm_moe_set_gate_bias(h, torch.zeros(E, device='cuda').data_ptr(), st))
        for e in range(E):
            if fmt == 'u4':
                def lin(K, N):
                    return (torch.randint(-2**31, 2**31 - 1, (K, N // 8), device='cuda', dtype=torch.int32),
                            (torch.rand((K // 128, N), device='cuda') * 0.02 + 0.01).half() / (K ** 0.5),
                            torch.randint(4, 12, (K // 128, N), device='cuda').half())
            else:
                def lin(K, N):
                    return (torch.randint(0, 256, (N, K // 2), device='cuda', dtype=torch.uint8),
                            torch.randint(118, 121, (N, K // 32), device='cuda', dtype=torch.uint8), None)
            w13, w2 = lin(H, 2 * I), lin(I, H)
            p = [t.data_ptr() if t is not None else None for t in w13 + w2]
            _ffi.check(tm.tm_moe_set_expert(h, e, *p, st))
            if fmt == 'mxfp4':
                b13, b2 = (0.1 * torch.randn(2 * I, device='cuda')).half(), (0.1 * torch.randn(H, device='cuda')).half()
                _ffi.check(tm.tm_moe_set_expert_bias(h, e, b13.data_ptr(), b2.data_ptr(), st))
            torch.cuda.synchronize()
        blocks[fmt] = h
    x = torch.randn((T, H), device='cuda').half()
    out = torch.empty((T, H), device='cuda', dtype=torch.float16)
    graphs = {}
    keep = []
    for fmt, h in blocks.items():
        ws = torch.empty((tm.tm_moe_workspace(h, T),), device='cuda', dtype=torch.uint8)
        keep.append(ws)

        def stages(mask, h=h, ws=ws):
            _ffi.check(tm.tm_moe_forward_stages(h, out.data_ptr(), x.data_ptr(), T, ws.data_ptr(), mask,
                                                torch.cuda.current_stream().cuda_stream))
        stages(31)      # fills the workspace the single stages run on
        torch.cuda.synchronize()
        for what, mask in STAGES:
            n = 20 if mask != 31 else 10
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(n):
                    stages(mask)
            graphs[(fmt, what)] = (g, n)

    def timed(g, n):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) * 1e3 / n
    samples = {key: [] for key in graphs}
    for rep in range(-3, a.repeats):
        for what, _ in STAGES:
            for fmt in blocks:
                v = timed(*graphs[(fmt, what)])
                if rep >= 0:
                    samples[(fmt, what)].append(v)
    lines = [f'# grouped expert GEMMs, decode: hidden = inter = {H}, {E} experts, top-{K_TOP}, {T} tokens; us per launch, median (min-max) of '
             f'{a.repeats} graph replays,', '# u4 (gated SiLU) and MXFP4 (gated gpt-oss epilogue with biases) alternating in one process']
    for what, _ in STAGES:
        u, m = sorted(samples[('u4', what)]), sorted(samples[('mxfp4', what)])
        mu, mm = u[len(u) // 2], m[len(m) // 2]
        lines.append(f'{what:<8} u4 {mu:8.2f} ({u[0]:.2f}-{u[-1]:.2f})   mxfp4 {mm:8.2f} ({m[0]:.2f}-{m[-1]:.2f})   mxfp4 / u4 {mm / mu:.3f}   '
                     f'u4 spread max / min {u[-1] / u[0]:.3f}')
    for h in blocks.values():
        tm.tm_moe_destroy(h)
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
