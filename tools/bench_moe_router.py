#!/usr/bin/env python
"""Times the MoE block launch by launch on the GPU: gate + top-k, routing tables, the grouped w1w3 and w2 GEMMs, the combine
(tm_moe_forward_stages), the router pair (gate + tables) and the whole block (tm_moe_forward).

  * 8 experts / top-2 / H 4096 / I 14336 (Mixtral) and 64 experts / top-8 / H 2048 / I 768, T = 64 and 8192: the serial router
    (TM_MOE_ROUTER=auto) against the wide one (=wide), in one process, the two settings alternating repeat by repeat;
  * 128 experts / top-8 at H 2048 / I 768 (Qwen3-30B-A3B) and H 4096 / I 1536 (Qwen3-235B-A22B), T = 1, 64, 256, 8192: wide only.

Every figure is device time: `n` copies of the launch(es) are captured into one graph, and device events bracket one replay of it,
so the host's enqueue rate is not in the window; what is in it is the launch-to-launch gap of a graph, as in the engine's captured
decode step.  The copies run back to back on the same operands, so x, Wg and the tables are cache-warm; the expert weights of the
larger geometries exceed the caches.  A stage runs on what a whole forward left in the workspace.  After three warm-up replays the
table gives the median and the range of `--repeats` replays.  Every geometry runs in a child process of its own under a time limit;
the first child that fails ends the run.  Expert weights are random u4 codes drawn on the device.

    python tools/bench_moe_router.py [--out profiles/moe_router_ab.txt] [--repeats 9]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = [('gate', 1), ('route', 2), ('router', 3), ('w1w3', 4), ('w2', 8), ('combine', 16), ('forward', 31)]

GEOMETRIES = [      # name, H, I, E, k, Ts, modes
    ('mixtral-8x7b', 4096, 14336, 8, 2, (64, 8192), ('auto', 'wide')),
    ('e64-top8', 2048, 768, 64, 8, (64, 8192), ('auto', 'wide')),
    ('qwen3-30b-a3b', 2048, 768, 128, 8, (1, 64, 256, 8192), ('wide',)),
    ('qwen3-235b-a22b', 4096, 1536, 128, 8, (1, 64, 256, 8192), ('wide',)),
]


def child(name, repeats):
    import ctypes as C

    import torch

    from lmdeploy_amd import _ffi
    tm = _ffi.load()
    _, H, I, E, k, Ts, modes = next(g for g in GEOMETRIES if g[0] == name)
    torch.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    h = C.c_void_p()
    _ffi.check(tm.tm_moe_create(C.byref(h), H, I, E, k, 0, 1, 1.0))
    gate = (0.02 * torch.randn((H, E), device='cuda')).half()
    _ffi.check(tm.tm_moe_set_gate(h, gate.data_ptr(), st))
    for e in range(E):
        def lin(K, N):
            return (torch.randint(-2**31, 2**31 - 1, (K, N // 8), device='cuda', dtype=torch.int32),
                    (torch.rand((K // 128, N), device='cuda') * 0.02 + 0.01).half() / (K ** 0.5),
                    torch.randint(4, 12, (K // 128, N), device='cuda').half())
        a, b = lin(H, 2 * I), lin(I, H)
        _ffi.check(tm.tm_moe_set_expert(h, e, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
                                        b[2].data_ptr(), st))
        torch.cuda.synchronize()
    rows = []
    for T in Ts:
        x = torch.randn((T, H), device='cuda').half()
        out = torch.empty((T, H), device='cuda', dtype=torch.float16)
        ws = torch.empty((tm.tm_moe_workspace(h, T),), device='cuda', dtype=torch.uint8)

        def stages(mask):
            _ffi.check(tm.tm_moe_forward_stages(h, out.data_ptr(), x.data_ptr(), T, ws.data_ptr(), mask,
                                                torch.cuda.current_stream().cuda_stream))
        graphs = {}
        for m in modes:             # one eager forward fills the workspace (and prepares the block), then the graphs are captured
            _ffi.check(tm.tm_debug_set_moe_router(1 if m == 'wide' else 0))
            stages(31)
            torch.cuda.synchronize()
            for what, mask in STAGES:
                n = (40 if mask != 31 else 10) if T <= 256 else (4 if mask != 31 else 2)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(n):
                        stages(mask)
                graphs[(m, what)] = (g, n)
        tm.tm_debug_set_moe_router(-1)

        def timed(g, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / n      # us per copy
        samples = {key: [] for key in graphs}
        for rep in range(-3, repeats):              # three warm-up rounds; the settings alternate inside a round
            for what, _ in STAGES:
                for m in modes:
                    v = timed(*graphs[(m, what)])
                    if rep >= 0:
                        samples[(m, what)].append(v)
        for m in modes:
            row = dict(name=name, H=H, I=I, E=E, k=k, T=T, mode=m)
            for what, _ in STAGES:
                v = sorted(samples[(m, what)])
                row[what] = (v[len(v) // 2], v[0], v[-1])
            rows.append(row)
        del graphs
    tm.tm_moe_destroy(h)
    print('ROWS ' + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moe_router_ab.txt'))
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
    lines = ['# MoE block launch by launch (tm_moe_forward_stages, u4 experts), MI355X; device events around one replay of a graph of n',
             f'# back-to-back copies; us per copy: median (min-max) of {a.repeats} replays; auto (serial router) and wide alternate in one process.',
             '# router = gate + route captured as a pair; share = router / forward; r/w1w3 = router / grouped w1w3 GEMM',
             f'{"geometry":<16}{"E":>4}{"k":>2}{"T":>5} {"mode":>4} ' + ' '.join(f'{w:>20}' for w, _ in STAGES) + f' {"share":>6} {"r/w1w3":>6}']

    def cell(v):
        return f'{v[0]:.1f} ({v[1]:.1f}-{v[2]:.1f})'
    for r in rows:
        lines.append(f'{r["name"]:<16}{r["E"]:>4}{r["k"]:>2}{r["T"]:>5} {r["mode"]:>4} ' + ' '.join(f'{cell(r[w]):>20}' for w, _ in STAGES)
                     + f' {r["router"][0] / r["forward"][0]:>6.3f} {r["router"][0] / r["w1w3"][0]:>6.2f}')
    lines.append('# serial / wide, medians, where both run:')
    for r in rows:
        if r['mode'] == 'auto':
            n = next(q for q in rows if q['mode'] == 'wide' and (q['name'], q['T']) == (r['name'], r['T']))
            lines.append(f'#   {r["name"]} T={r["T"]}: ' + ', '.join(f'{w} {r[w][0] / n[w][0]:.2f}x' for w in ('gate', 'route', 'router', 'forward')))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
