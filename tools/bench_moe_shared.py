#!/usr/bin/env python
"""Times the Qwen2-MoE block's shared-expert combine on the GPU at Qwen2-57B-A14B's geometry (H 3584, 64 experts, top-8, expert
width 2560, shared width 20480; u4 weights), T = 64 and T = 1024:

  * combine:  the fused launch of a block with a shared gate (moe_combine_shared_kernel: sigmoid gate + shared term + routed sum;
              tm_moe_forward_shared_stages, stage 16) against the plain moe_combine_kernel of a gate-less twin with the same router and
              experts on the same tables (tm_moe_forward_stages, stage 16);
  * ffn:      the whole layer FFN with the shared expert (its w1w3 and w2 through tm_linear_forward, then tm_moe_forward_shared)
              against the routed block alone (tm_moe_forward on the twin).

Method as tools/bench_moe_router.py: `n` back-to-back copies of an arm are captured into one graph and device events bracket one
replay, so the window holds the graph's launch-to-launch gap and not the host's enqueue rate; the copies run on the same operands,
so x, the gate vector and the tables are cache-warm, the expert weights are not.  The arms alternate repeat by repeat in one
process; after three warm-up rounds the table gives the median and the range of `--repeats` replays.  The measurement runs in a
child process under a time limit.  Weights are random u4 codes drawn on the device.

    python tools/bench_moe_shared.py [--out profiles/moe_shared_combine.txt] [--repeats 9]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, I, S, E, K = 3584, 2560, 20480, 64, 8
TS = (64, 1024)
ARMS = ('combine plain', 'combine shared', 'ffn routed', 'ffn routed+shared')


def child(repeats):
    import ctypes as C

    import torch

    from lmdeploy_amd import _ffi
    tm = _ffi.load()
    torch.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream

    def lin(Kd, N):
        return (torch.randint(-2**31, 2**31 - 1, (Kd, N // 8), device='cuda', dtype=torch.int32),
                (torch.rand((Kd // 128, N), device='cuda') * 0.02 + 0.01).half() / (Kd ** 0.5),
                torch.randint(4, 12, (Kd // 128, N), device='cuda').half())
    plain, gated = C.c_void_p(), C.c_void_p()
    router = (0.02 * torch.randn((H, E), device='cuda')).half()
    for h in (plain, gated):
        _ffi.check(tm.tm_moe_create(C.byref(h), H, I, E, K, 0, 0, 1.0))
        _ffi.check(tm.tm_moe_set_gate(h, router.data_ptr(), st))
    sgate = (0.02 * torch.randn((H,), device='cuda')).half()
    _ffi.check(tm.tm_moe_set_shared_gate(gated, sgate.data_ptr(), st))
    for e in range(E):
        a, b = lin(H, 2 * I), lin(I, H)
        for h in (plain, gated):
            _ffi.check(tm.tm_moe_set_expert(h, e, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
                                            b[2].data_ptr(), st))
        torch.cuda.synchronize()
    w13, w2 = C.c_void_p(), C.c_void_p()       # the shared expert: a dense FFN of width S
    for h, (Kd, N) in ((w13, (H, 2 * S)), (w2, (S, H))):
        _ffi.check(tm.tm_linear_create(C.byref(h), Kd, N, 0, 128))
        q, s, z = lin(Kd, N)
        _ffi.check(tm.tm_linear_prepare(h, q.data_ptr(), s.data_ptr(), z.data_ptr(), st))
        torch.cuda.synchronize()
    rows = []
    for T in TS:
        x = torch.randn((T, H), device='cuda').half()
        out = torch.empty((T, H), device='cuda', dtype=torch.float16)
        shared = torch.randn((T, H), device='cuda').half()
        act = torch.empty((T, S), device='cuda', dtype=torch.float16)
        ws = {h.value: torch.empty((tm.tm_moe_workspace(h, T),), device='cuda', dtype=torch.uint8) for h in (plain, gated)}
        lws = torch.zeros((max(tm.tm_linear_workspace(w13, T), tm.tm_linear_workspace(w2, T), 256),), device='cuda', dtype=torch.uint8)

        def cur():
            return torch.cuda.current_stream().cuda_stream

        def arm(name):
            if name == 'combine plain':
                _ffi.check(tm.tm_moe_forward_stages(plain, out.data_ptr(), x.data_ptr(), T, ws[plain.value].data_ptr(), 16, cur()))
            elif name == 'combine shared':
                _ffi.check(tm.tm_moe_forward_shared_stages(gated, out.data_ptr(), x.data_ptr(), shared.data_ptr(), T,
                                                           ws[gated.value].data_ptr(), None, None, 16, cur()))
            elif name == 'ffn routed':
                _ffi.check(tm.tm_moe_forward(plain, out.data_ptr(), x.data_ptr(), T, ws[plain.value].data_ptr(), None, None, cur()))
            else:
                _ffi.check(tm.tm_linear_forward(w13, x.data_ptr(), H, act.data_ptr(), S, T, 1, 0, 0, 0, lws.data_ptr(), cur()))
                _ffi.check(tm.tm_linear_forward(w2, act.data_ptr(), S, shared.data_ptr(), H, T, 0, 0, 0, 0, lws.data_ptr(), cur()))
                _ffi.check(tm.tm_moe_forward_shared(gated, out.data_ptr(), x.data_ptr(), shared.data_ptr(), T, ws[gated.value].data_ptr(),
                                                    None, None, cur()))
        # one eager run of the whole forwards fills both workspaces (and prepares the blocks), then the graphs are captured
        arm('ffn routed')
        arm('ffn routed+shared')
        torch.cuda.synchronize()
        graphs = {}
        for name in ARMS:
            n = (40 if name.startswith('combine') else 6) if T <= 256 else (8 if name.startswith('combine') else 2)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(n):
                    arm(name)
            graphs[name] = (g, n)

        def timed(g, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / n      # us per copy
        samples = {name: [] for name in ARMS}
        for rep in range(-3, repeats):              # three warm-up rounds; the arms alternate inside a round
            for name in ARMS:
                v = timed(*graphs[name])
                if rep >= 0:
                    samples[name].append(v)
        row = dict(T=T)
        for name in ARMS:
            v = sorted(samples[name])
            row[name] = (v[len(v) // 2], v[0], v[-1])
        rows.append(row)
        del graphs
    for h in (plain, gated):
        tm.tm_moe_destroy(h)
    for h in (w13, w2):
        tm.tm_linear_destroy(h)
    print('ROWS ' + json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moe_shared_combine.txt'))
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--limit', type=int, default=300, help='seconds for the measurement')
    a = ap.parse_args()
    if a.child:
        return child(a.repeats)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--repeats', str(a.repeats)], capture_output=True, text=True,
                       timeout=a.limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit(f'exit status {p.returncode}')
    rows = json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith('ROWS '))[5:])
    lines = [f'# Qwen2-MoE shared-expert combine, Qwen2-57B-A14B block (H {H}, {E} experts, top-{K}, widths {I} / {S}, u4), MI355X;',
             '# device events around one replay of a graph of n back-to-back copies; us per copy: median (min-max) of '
             f'{a.repeats} replays; the arms alternate in one process.',
             '# combine: moe_combine_kernel of the gate-less twin / moe_combine_shared_kernel (gate + shared term + routed sum), same tables;',
             '# ffn: tm_moe_forward of the twin / shared w1w3 + w2 (tm_linear_forward) + tm_moe_forward_shared',
             f'{"T":>5} ' + ' '.join(f'{w:>24}' for w in ARMS) + f' {"shared - plain":>14} {"ffn ratio":>9}']

    def cell(v):
        return f'{v[0]:.1f} ({v[1]:.1f}-{v[2]:.1f})'
    for r in rows:
        lines.append(f'{r["T"]:>5} ' + ' '.join(f'{cell(r[w]):>24}' for w in ARMS)
                     + f' {r["combine shared"][0] - r["combine plain"][0]:>14.1f} {r["ffn routed+shared"][0] / r["ffn routed"][0]:>9.2f}')
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
