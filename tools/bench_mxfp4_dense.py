#!/usr/bin/env python
"""Times the MXFP4 W4A4 dense linear (block-scaled FP4 matrix cores) against the AWQ W4A16 kernels and the channel-scaled
fp8 x fp8 kernel at Llama-3-8B's decoder linears, and a synthetic Llama-3-8B in model_format mxfp4 against awq.

GEMMs: (K, N) = 4096 x 6144 (w_qkv), 4096 x 4096 (wo), 4096 x 28672 gated (w1w3), 14336 x 4096 (w2) at M = 64 (decode) and
M = 8192 (prefill).  `mxfp4` is tm_linear_forward_mxfp4 and `fp8_channel` tm_linear_forward_fp8 -- activation quantiser + GEMM
(+ split-K reduce), as the engine runs them --, `awq` is tm_linear_forward on a u4 handle.  Every launch of a graph reads another of
`--copies` weight copies (together more bytes than the Infinity Cache holds, as in a decode step); n launches are captured into
one graph, device events bracket one replay, the three kernels alternate repeat by repeat in one process; after three warm-up rounds
the table gives the median and the range of `--repeats` replays and the ratio of the medians.

Model: `synthetic:llama3_8b`, int8 KV, model_format mxfp4 and awq, one engine after the other, `--rounds` times: the time to first
token of one 1024-token prompt, then 64 sequences of 128 tokens and decode steps under the captured graph.

One process per section (`--skip-model` / `--skip-gemms`):

    python tools/bench_mxfp4_dense.py [--out profiles/mxfp4_dense.txt] [--repeats 9] [--skip-model | --skip-gemms]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('w_qkv', 4096, 6144, False), ('wo', 4096, 4096, False), ('w1w3', 4096, 28672, True), ('w2', 14336, 4096, False)]


def bench_gemms(a, lines):
    import torch

    from lmdeploy_amd import _ffi
    tm = _ffi.load()
    torch.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    for M in (64, 8192):
        lines.append(f'# M = {M}: us per linear (quantiser + GEMM + reduce for mxfp4 and fp8_channel), median (min-max) of {a.repeats} graph replays')
        for name, K, N, gated in SHAPES:
            copies = a.copies if M == 64 else 2
            handles = {'mxfp4': [], 'awq': [], 'fp8_channel': []}
            for _ in range(copies):
                codes = torch.randint(0, 0x77, (K, N), device='cuda', dtype=torch.uint8) | (torch.randint(0, 2, (K, N), device='cuda', dtype=torch.uint8) << 7)
                cs = (torch.rand(N, device='cuda') * 2e-4 + 1e-4).float()
                blocks = torch.randint(0, 256, (N, K // 2), device='cuda', dtype=torch.uint8)
                sb = torch.randint(115, 118, (N, K // 32), device='cuda', dtype=torch.uint8)
                qw = torch.randint(-2**31, 2**31 - 1, (K, N // 8), device='cuda', dtype=torch.int32)
                sc = (torch.rand((K // 128, N), device='cuda') * 2e-3 + 1e-3).half()
                zs = torch.full((K // 128, N), 8.0, device='cuda', dtype=torch.float16)
                for mode in handles:
                    h = C.c_void_p()
                    _ffi.check(tm.tm_linear_create(C.byref(h), K, N, {'mxfp4': 3, 'awq': 0, 'fp8_channel': 2}[mode], 32 if mode == 'mxfp4' else 128))
                    if mode == 'mxfp4':
                        _ffi.check(tm.tm_linear_prepare_mxfp4(h, blocks.data_ptr(), sb.data_ptr(), st))
                    elif mode == 'awq':
                        _ffi.check(tm.tm_linear_prepare(h, qw.data_ptr(), sc.data_ptr(), zs.data_ptr(), st))
                    else:
                        _ffi.check(tm.tm_linear_prepare_fp8_channel(h, codes.data_ptr(), cs.data_ptr(), st))
                    handles[mode].append(h)
                torch.cuda.synchronize()
                del codes, blocks, qw
            x = torch.randn((M, K), device='cuda').half()
            ldy = N // 2 if gated else N
            y = torch.empty((M, ldy), device='cuda', dtype=torch.float16)
            ws = torch.zeros((max(tm.tm_linear_fp8_workspace(handles['fp8_channel'][0], M), tm.tm_linear_workspace(handles['awq'][0], M),
                                  tm.tm_linear_mxfp4_workspace(handles['mxfp4'][0], M)),), device='cuda', dtype=torch.uint8)
            n = 2 * copies if M == 64 else 2

            def launch(kind, i):
                s = torch.cuda.current_stream().cuda_stream
                if kind == 'awq':
                    _ffi.check(tm.tm_linear_forward(handles['awq'][i % copies], x.data_ptr(), K, y.data_ptr(), ldy, M, int(gated), 0, 0, 0,
                                                    ws.data_ptr(), s))
                elif kind == 'mxfp4':
                    _ffi.check(tm.tm_linear_forward_mxfp4(handles[kind][i % copies], x.data_ptr(), K, y.data_ptr(), ldy, M, int(gated), 0,
                                                          ws.data_ptr(), s))
                else:
                    _ffi.check(tm.tm_linear_forward_fp8(handles[kind][i % copies], x.data_ptr(), K, y.data_ptr(), ldy, M, int(gated), 0,
                                                        ws.data_ptr(), s))
            graphs = {}
            for kind in ('mxfp4', 'awq', 'fp8_channel'):
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
                         + f'   mxfp4 / awq {med["mxfp4"] / med["awq"]:.3f}   mxfp4 / fp8_channel {med["mxfp4"] / med["fp8_channel"]:.3f}')
            del graphs
            for hs in handles.values():
                for h in hs:
                    tm.tm_linear_destroy(h)
            torch.cuda.synchronize()


def bench_model(a, lines):
    import numpy as np

    from lmdeploy_amd import TurbomindEngineConfig, pipeline
    rng = np.random.default_rng(0)
    long_prompt = [rng.integers(0, 128000, 1024).astype(np.int32)]
    prompts = [rng.integers(0, 128000, 128).astype(np.int32) for _ in range(64)]
    lines.append('# synthetic:llama3_8b, int8 KV: time to first token of one 1024-token prompt (second of two prefills); batch 64 with 128-token '
                 'prompts: ms per decode step over 64 graph steps')
    for rnd in range(a.rounds):
        for fmt in ('mxfp4', 'awq'):
            pipe = pipeline('synthetic:llama3_8b', backend_config=TurbomindEngineConfig(model_format=fmt, quant_policy=8, max_batch_size=64,
                                                                                        session_len=2048, cache_max_entry_count=0.2))
            try:
                eng = pipe.engine
                for _ in range(2):
                    eng.prefill(long_prompt, max_new_tokens=2)
                    ttft = float(np.max(eng.prefill_times_ms()))
                    eng.release()
                eng.prefill(prompts, max_new_tokens=200)
                eng.decode(8)
                eng.sync()
                t0 = time.perf_counter()
                eng.decode(64)
                eng.sync()
                ms = (time.perf_counter() - t0) * 1e3 / 64
                eng.release()
            finally:
                pipe.close()
            lines.append(f'round {rnd} {fmt:<6} decode {ms:7.3f} ms / step ({64 / ms * 1e3:9.1f} tok/s)   TTFT of 1024 tokens {ttft:8.1f} ms')


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
        sys.exit('bench_mxfp4_dense.py needs a GPU')
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
