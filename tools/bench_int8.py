#!/usr/bin/env python
"""Times the INT8 W8A8 linear (int8 x int8 on v_mfma_i32_32x32x32_i8) against the channel-scaled fp8 x fp8 kernel and the AWQ kernels at
Llama-3-8B's decoder linears, and a synthetic Llama-3-8B in model_format int8, fp8_channel and awq.

GEMMs: (K, N) = 4096 x 6144 (w_qkv), 4096 x 4096 (wo), 4096 x 28672 gated (w1w3), 14336 x 4096 (w2) at M = 64 (decode) and
M = 8192 (prefill).  `int8` and `fp8_channel` are tm_linear_forward_int8 / tm_linear_forward_fp8 -- activation quantiser + GEMM
(+ split-K reduce), as the engine runs them --, `awq` is tm_linear_forward on a u4 handle.  Every launch of a graph reads another of
`--copies` weight copies (together more bytes than the Infinity Cache holds, as in a decode step); n launches are captured into
one graph, device events bracket one replay, the three kernels alternate repeat by repeat in one process; after three warm-up rounds
the table gives the median and the range of `--repeats` replays and the ratio of the medians.

Model: `synthetic:llama3_8b`, 64 sequences of 128 tokens (one 8192-token prefill forward: its time to first token), then decode
steps under the captured graph; int8 KV, one engine after the other, `--rounds` times.

    python tools/bench_int8.py [--out profiles/int8.txt] [--repeats 9] [--skip-model]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('w_qkv', 4096, 6144, False), ('wo', 4096, 4096, False), ('w1w3', 4096, 28672, True), ('w2', 14336, 4096, False)]
KINDS = ('int8', 'fp8_channel', 'awq')


def bench_gemms(a, lines):
    import torch

    from lmdeploy_amd import _ffi
    tm = _ffi.load()
    torch.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    for M in (64, 8192):
        lines.append(f'# M = {M}: us per linear (quantiser + GEMM + reduce for int8 and fp8_channel), median (min-max) of {a.repeats} graph replays')
        for name, K, N, gated in SHAPES:
            copies = a.copies if M == 64 else 2
            handles = {k: [] for k in KINDS}
            for _ in range(copies):
                i8 = torch.randint(-128, 128, (K, N), device='cuda', dtype=torch.int8)
                codes = torch.randint(0, 0x77, (K, N), device='cuda', dtype=torch.uint8) | (torch.randint(0, 2, (K, N), device='cuda', dtype=torch.uint8) << 7)
                cs = (torch.rand(N, device='cuda') * 2e-4 + 1e-4).float()
                qw = torch.randint(-2**31, 2**31 - 1, (K, N // 8), device='cuda', dtype=torch.int32)
                sc = (torch.rand((K // 128, N), device='cuda') * 2e-3 + 1e-3).half()
                zs = torch.full((K // 128, N), 8.0, device='cuda', dtype=torch.float16)
                for mode in KINDS:
                    h = C.c_void_p()
                    _ffi.check(tm.tm_linear_create(C.byref(h), K, N, {'int8': 4, 'awq': 0, 'fp8_channel': 2}[mode], 128))
                    if mode == 'int8':
                        _ffi.check(tm.tm_linear_prepare_int8(h, i8.data_ptr(), cs.data_ptr(), st))
                    elif mode == 'awq':
                        _ffi.check(tm.tm_linear_prepare(h, qw.data_ptr(), sc.data_ptr(), zs.data_ptr(), st))
                    else:
                        _ffi.check(tm.tm_linear_prepare_fp8_channel(h, codes.data_ptr(), cs.data_ptr(), st))
                    handles[mode].append(h)
                torch.cuda.synchronize()
                del i8, codes, qw
            x = torch.randn((M, K), device='cuda').half()
            ldy = N // 2 if gated else N
            y = torch.empty((M, ldy), device='cuda', dtype=torch.float16)
            ws = torch.zeros((max(tm.tm_linear_fp8_workspace(handles['fp8_channel'][0], M), tm.tm_linear_workspace(handles['awq'][0], M),
                                  tm.tm_linear_int8_workspace(handles['int8'][0], M)),), device='cuda', dtype=torch.uint8)
            n = 2 * copies if M == 64 else 2

            def launch(kind, i):
                s = torch.cuda.current_stream().cuda_stream
                h = handles[kind][i % copies]
                if kind == 'awq':
                    _ffi.check(tm.tm_linear_forward(h, x.data_ptr(), K, y.data_ptr(), ldy, M, int(gated), 0, 0, 0, ws.data_ptr(), s))
                elif kind == 'int8':
                    _ffi.check(tm.tm_linear_forward_int8(h, x.data_ptr(), K, y.data_ptr(), ldy, M, int(gated), 0, ws.data_ptr(), s))
                else:
                    _ffi.check(tm.tm_linear_forward_fp8(h, x.data_ptr(), K, y.data_ptr(), ldy, M, int(gated), 0, ws.data_ptr(), s))
            graphs = {}
            for kind in KINDS:
                launch(kind, 0)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for i in range(n):
                        launch(kind, i)
                graphs[kind] = g
            samples = {k: [] for k in graphs}
            for rep in range(-3, a.repeats):
                for kind, g in graphs.items():
                    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    g.replay()
                    t.record()
                    t.synchronize()
                    if rep >= 0:
                        samples[kind].append(s.elapsed_time(t) * 1e3 / n)
            med = {}
            cells = []
            for kind, v in samples.items():
                v.sort()
                med[kind] = v[len(v) // 2]
                cells.append(f'{kind} {med[kind]:9.2f} ({v[0]:.2f}-{v[-1]:.2f})')
            lines.append(f'{name:<5} {K:>5} x {N:<5}{" gated" if gated else "      "} ' + '   '.join(cells)
                         + f'   int8 / fp8_channel {med["int8"] / med["fp8_channel"]:.3f}   int8 / awq {med["int8"] / med["awq"]:.3f}')
            del graphs
            for hs in handles.values():
                for h in hs:
                    tm.tm_linear_destroy(h)
            torch.cuda.synchronize()


def bench_model(a, lines):
    import numpy as np

    from lmdeploy_amd import TurbomindEngineConfig, pipeline
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, 128000, 128).astype(np.int32) for _ in range(64)]
    lines.append('# synthetic:llama3_8b, batch 64, 128-token prompts (one 8192-token prefill forward), int8 KV: ms per decode step over 64 graph '
                 'steps, time to first token of the prefill')
    for rnd in range(a.rounds):
        for fmt in KINDS:
            pipe = pipeline('synthetic:llama3_8b', backend_config=TurbomindEngineConfig(model_format=fmt, quant_policy=8, max_batch_size=64,
                                                                                        session_len=512, cache_max_entry_count=0.2))
            try:
                eng = pipe.engine
                eng.prefill(prompts, max_new_tokens=200)
                ttft = float(np.max(eng.prefill_times_ms()))
                eng.decode(8)
                eng.sync()
                t0 = time.perf_counter()
                eng.decode(64)
                eng.sync()
                ms = (time.perf_counter() - t0) * 1e3 / 64
                eng.release()
            finally:
                pipe.close()
            lines.append(f'round {rnd} {fmt:<12} decode {ms:7.3f} ms / step ({64 / ms * 1e3:9.1f} tok/s)   TTFT of 64 x 128 tokens {ttft:8.1f} ms')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--copies', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--skip-gemms', action='store_true')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_int8.py needs a GPU')
    lines = []
    if not a.skip_gemms:
        bench_gemms(a, lines)
    if not a.skip_model:
        bench_model(a, lines)
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
