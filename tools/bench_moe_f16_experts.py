#!/usr/bin/env python
"""Times the grouped expert GEMMs of the MoE block (the w1w3 and w2 launches of tm_moe_forward_stages) for the three weight formats
gemm_kernel serves in its grouped mode -- fp16, e4m3 weight-only (TM_FP8_MFMA=0) and u4 -- at T = 64 tokens:

  * Qwen3-30B-A3B's block: H 2048, I 768, 128 experts, top-8;
  * Mixtral-8x7B's block:  H 4096, I 14336, 8 experts, top-2;

for every forced row tile (16 / 32 / 64) and for the launcher's own choice.  The three formats are three blocks with the same router
in one process, timed alternately repeat by repeat, so they see the same box at the same time.

Every figure is device time: `n` copies of the launch are captured into one graph and device events bracket one replay (as
tools/bench_moe_router.py does).  The copies run back to back on the same operands: activations and tables are cache-warm; an
arm whose expert weights are smaller than the 256 MB Infinity Cache may be served from it (marked `*`).  After three warm-up rounds
the table gives the median and the range of `--repeats` replays, and weight bytes / time as a fraction of 8 TB/s, where weight bytes
= (experts with at least one row) x the packed size of one expert's linear in that format (scales included).
Weights are random, drawn on the device.  Each geometry runs in a child process under a time limit; the first child that fails
ends the run.

    python tools/bench_moe_f16_experts.py [--out profiles/moe_f16_experts.txt] [--repeats 9]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRIES = [      # name, H, I, E, k
    ('qwen3-30b-a3b', 2048, 768, 128, 8),
    ('mixtral-8x7b', 4096, 14336, 8, 2),
]
ARMS = [('f16', 1), ('fp8wo', 2), ('u4', 0)]      # name, weight_type
TILES = (0, 16, 32, 64)
T = 64
HBM = 8e12
MALL = 256 * 2**20


def linear_bytes(arm, K, N):
    """packed weights + scales of one K x N expert linear as the kernel streams them"""
    if arm == 'f16':
        return K * N * 2
    return (K * N if arm == 'fp8wo' else K * N // 2) + (K // 128) * N * 4


def child(name, repeats):
    import ctypes as C

    os.environ['TM_FP8_MFMA'] = '0'      # e4m3 experts stay on gemm_kernel's weight-only arm
    import torch

    from lmdeploy_amd import _ffi
    tm = _ffi.load()
    _, H, I, E, k = next(g for g in GEOMETRIES if g[0] == name)
    torch.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    gate = (0.02 * torch.randn((H, E), device='cuda')).half()
    blocks = {}
    for arm, wt in ARMS:
        h = C.c_void_p()
        _ffi.check(tm.tm_moe_create(C.byref(h), H, I, E, k, wt, 1, 1.0))
        _ffi.check(tm.tm_moe_set_gate(h, gate.data_ptr(), st))
        for e in range(E):
            def lin(K, N, gated):
                if arm == 'f16':
                    return ((torch.randn((K, N), device='cuda') / K ** 0.5).half(), None, None)
                if arm == 'fp8wo':      # e4m3 codes without NaN (0x7f / 0xff), one block scale
                    q = torch.randint(0, 127, (K, N), device='cuda', dtype=torch.uint8) | (torch.randint(0, 2, (K, N), device='cuda', dtype=torch.uint8) << 7)
                    return (q, torch.full((K // 128, N // 128), 0.01 / K ** 0.5, device='cuda', dtype=torch.float32), None)
                return (torch.randint(-2**31, 2**31 - 1, (K, N // 8), device='cuda', dtype=torch.int32),
                        (torch.rand((K // 128, N), device='cuda') * 0.02 + 0.01).half() / (K ** 0.5),
                        torch.randint(4, 12, (K // 128, N), device='cuda').half())
            a, b = lin(H, 2 * I, True), lin(I, H, False)
            p = [t.data_ptr() if t is not None else None for t in a + b]
            _ffi.check(tm.tm_moe_set_expert(h, e, *p, st))
            torch.cuda.synchronize()
        blocks[arm] = h
    x = torch.randn((T, H), device='cuda').half()
    out = torch.empty((T, H), device='cuda', dtype=torch.float16)
    graphs, hit = {}, {}
    keep = []
    for arm, _ in ARMS:
        h = blocks[arm]
        ws = torch.empty((tm.tm_moe_workspace(h, T),), device='cuda', dtype=torch.uint8)
        ids = torch.zeros((T, k), device='cuda', dtype=torch.int32)
        keep.append(ws)
        _ffi.check(tm.tm_moe_forward(h, out.data_ptr(), x.data_ptr(), T, ws.data_ptr(), ids.data_ptr(), None, st))      # fills the workspace
        torch.cuda.synchronize()
        hit[arm] = int(torch.unique(ids).numel())
        for rows in TILES:
            _ffi.check(tm.tm_debug_set_grouped_rows(rows))      # read when the launch is enqueued, i.e. at capture
            for what, mask, n in (('w1w3', 4, 12), ('w2', 8, 12)):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(n):
                        _ffi.check(tm.tm_moe_forward_stages(h, out.data_ptr(), x.data_ptr(), T, ws.data_ptr(), mask,
                                                            torch.cuda.current_stream().cuda_stream))
                graphs[(arm, rows, what)] = (g, n)
            tm.tm_debug_set_grouped_rows(0)

    def timed(g, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n      # us per launch
    samples = {key: [] for key in graphs}
    for rep in range(-3, repeats):                  # the arms alternate inside a round
        for what in ('w1w3', 'w2'):
            for rows in TILES:
                for arm, _ in ARMS:
                    v = timed(*graphs[(arm, rows, what)])
                    if rep >= 0:
                        samples[(arm, rows, what)].append(v)
    res = []
    for (arm, rows, what), v in samples.items():
        v = sorted(v)
        K, N = (H, 2 * I) if what == 'w1w3' else (I, H)
        res.append(dict(name=name, H=H, I=I, E=E, k=k, arm=arm, rows=rows, what=what, us=(v[len(v) // 2], v[0], v[-1]), hit=hit[arm],
                        bytes=hit[arm] * linear_bytes(arm, K, N)))
    for h in blocks.values():
        tm.tm_moe_destroy(h)
    print('ROWS ' + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moe_f16_experts.txt'))
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--child')
    ap.add_argument('--limit', type=int, default=240, help='seconds per geometry')
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats)
    rows = []
    for g in GEOMETRIES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', g[0], '--repeats', str(a.repeats)],
                           capture_output=True, text=True, timeout=a.limit)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f'{g[0]}: exit status {p.returncode}; nothing more is started on the GPU')
        rows += json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith('ROWS '))[5:])
    lines = ['# Grouped expert GEMMs of the MoE block (tm_moe_forward_stages: w1w3 = mask 4, w2 = mask 8) at T = 64, MI355X, gemm_kernel grouped mode.',
             '# Arms: f16 (fp16 experts), fp8wo (e4m3 weight-only, TM_FP8_MFMA=0), u4 (AWQ); three blocks in one process, timed alternately.',
             f'# Device events around one replay of a graph of 12 back-to-back launches; us per launch: median (min-max) of {a.repeats} replays.',
             '# bytes = experts with rows x packed bytes of one expert linear (scales included); frac = bytes / time / 8 TB/s.',
             '# `*`: the arm\'s weight bytes fit the 256 MB Infinity Cache, so back-to-back copies may not stream from HBM.',
             f'{"geometry":<15}{"linear":>6}{"K":>6}{"N":>6} {"arm":>6} {"hit":>4} {"MB":>8} {"rows":>5} {"us per launch":>24} {"GB/s":>8} {"frac":>6}']
    for r in rows:
        K, N = (r['H'], 2 * r['I']) if r['what'] == 'w1w3' else (r['I'], r['H'])
        us = r['us']
        bw = r['bytes'] / (us[0] * 1e-6)
        lines.append(f'{r["name"]:<15}{r["what"]:>6}{K:>6}{N:>6} {r["arm"]:>6} {r["hit"]:>4} {r["bytes"] / 1e6:>8.1f} '
                     f'{(str(r["rows"]) if r["rows"] else "auto"):>5} {f"{us[0]:.1f} ({us[1]:.1f}-{us[2]:.1f})":>24} {bw / 1e9:>8.0f} '
                     f'{bw / HBM:>6.3f}{"*" if r["bytes"] < MALL else ""}')
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
