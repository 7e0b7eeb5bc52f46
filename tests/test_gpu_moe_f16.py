"""The MoE block with unquantised (fp16) experts through the C-ABI: tm_moe_create(TM_WEIGHT_F16) / tm_moe_set_expert with
scales = zeros = NULL / tm_moe_forward, on the grouped instantiations of gemm_kernel's fp16 arm.

The reference is oracle.moe_ffn's arithmetic on the very fp16 weights the block is given (fp16 x fp16 products, fp32 accumulation,
the gated-SiLU epilogue, one fp16 rounding per linear, an fp32 combine), the bound the project's own for the u4 arm, whose operand
and accumulation are the same: 4e-3 + 2^-6 |ref|; routing ids exact, weights within 1e-5; the workspace is poisoned with 0xFF.
Shapes are the smallest that reach every branch of the launcher: every decode row tile (16 / 32 / 64, forced and by the rule), the
prefill tiling (T = 300: several 64-row blocks per expert), w13 with two k-blocks and w2 with one (the weight ring's tail
re-loads), the serial router at 8 experts and the wide one at 72 with skewed routings (an expert that takes every token, experts
without rows, an expert at exactly twice the expected rows and one row past it)."""
import math

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.gpu_helpers import dev, host, release_all, st
from tests.qwen2_moe_reference import Qwen2MoeConfig, routed_f32, shared_combine
from tests.test_gpu_geometry import _expert_ffn
from tests.test_gpu_moe_wide import _forward, _picked_x, _skewed_picks

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
F16 = 1                      # TM_WEIGHT_F16
TILES = (0, 16, 32, 64)      # 0: the launcher's own rule


def _f16_expert(rng, H, I):
    """w13 [H][2I] ~ 1.5 / sqrt(H) N(0, 1) with (gate_j, up_j) interleaved columns, w2 [I][H] ~ 1 / sqrt(I) N(0, 1)"""
    return ((rng.standard_normal((H, 2 * I)) * (1.5 / math.sqrt(H))).astype(f16), (rng.standard_normal((I, H)) * (1.0 / math.sqrt(I))).astype(f16))


def _set_expert(tm, h, e, w13, w2):
    _ffi.check(tm.tm_moe_set_expert(h, e, dev(w13).data_ptr(), None, None, dev(w2).data_ptr(), None, None, st()))


def _small_f16_moe(tm, rng, H, I, E, k, norm_topk=1, shared_gate=None):
    """a block with a random router -> (handle, router, [(w13, w2)])"""
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E, k, F16, norm_topk, 1.0))
    router = (0.2 * rng.standard_normal((H, E))).astype(f16)
    _ffi.check(tm.tm_moe_set_gate(h, dev(router).data_ptr(), st()))
    if shared_gate is not None:
        _ffi.check(tm.tm_moe_set_shared_gate(h, dev(shared_gate).data_ptr(), st()))
    experts = [_f16_expert(rng, H, I) for _ in range(E)]
    for e, (w13, w2) in enumerate(experts):
        _set_expert(tm, h, e, w13, w2)
    return h, router, experts


def _f16_block(tm, H, I, E, k, cases, seed, norm_topk=True, scale=1.0):
    """tests.test_gpu_moe_wide._block for fp16 experts: a router that sends every token where the case wants it, the experts drawn
    one at a time (uploaded, their rows of every case computed by the oracle's expert arithmetic), o.moe_ffn's combine"""
    rng = np.random.default_rng(seed)
    gate = (rng.standard_normal((H, E)) * 0.00005).astype(f16)
    gate[:E] = np.eye(E, dtype=f16)
    xs, labels, wants = [], [], []
    for kind, T in cases:
        if kind == 'random':
            picks, want = [rng.permutation(E)[:k].tolist() for _ in range(T)], {}
        else:
            picks, want = _skewed_picks(kind, T, E, k)
        xs.append(_picked_x(rng, E, T, H, picks))
        labels.append(f'{kind} T={T}')
        wants.append((picks, want))
    routing = [o.moe_gate(x, gate, k, norm_topk, scale) for x in xs]
    for (picks, want), (_, ids, _), lab in zip(wants, routing, labels):
        assert np.array_equal(ids, np.asarray(picks)), f'{lab}: the routing is not the one aimed for'
        hist = np.bincount(ids.ravel(), minlength=E)
        assert all(hist[e] == n for e, n in want.items()), lab
    y = [np.zeros((len(x), k, H), f32) for x in xs]
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E, k, F16, int(norm_topk), scale))
    try:
        _ffi.check(tm.tm_moe_set_gate(h, dev(gate).data_ptr(), st()))
        for e in range(E):
            w13, w2 = _f16_expert(rng, H, I)
            _set_expert(tm, h, e, w13, w2)
            for c, (x, (_, ids, _)) in enumerate(zip(xs, routing)):
                t, j = np.nonzero(ids == e)
                if len(t):
                    y[c][t, j] = _expert_ffn('f16', (w13, w2), x[t]).astype(f32)
            release_all()
        for c, x in enumerate(xs):
            _, ids, w = routing[c]
            ref = np.zeros((len(x), H), f32)
            for j in range(k):
                ref += w[:, j:j + 1] * y[c][:, j]
            ref = ref.astype(f16).astype(f32)
            tol = 4e-3 + 2.0**-6 * np.abs(ref)
            assert np.any(np.abs(ref) > tol) and np.any(0.25 * np.abs(ref) > tol), f'{labels[c]}: outputs too small to test'
            for rows in (TILES if len(x) <= 64 else (0,)):
                out, gids, gw = _forward(tm, h, x, k, rows)
                what = f'f16 H {H} I {I} E {E} {labels[c]} rows {rows or "auto"}'
                assert np.array_equal(gids, ids), f'{what}: routing differs'
                assert np.abs(gw - w).max() <= 1e-5, what
                err = np.abs(out - ref)      # (a NaN left from the poisoned workspace fails the comparison below)
                print(f'{what}: |ref| max {np.abs(ref).max():.4f}, worst err / tol {(err / tol).max():.3f}')
                assert np.all(err <= tol), f'{what}: max err {err.max()} at {np.unravel_index(np.argmax(err - tol), err.shape)}'
    finally:
        tm.tm_moe_destroy(h)


@pytest.mark.parametrize('T', [1, 37, 64, 300])
def test_f16_experts_serial_router(tm, cuda, T):
    """H 256 (w13: two k-blocks), I 128 (w2: one), 8 experts, top-2, norm_topk: T <= 64 on every row tile, T = 300 on the prefill
    tiling (expected 75 rows per expert: two 64-row blocks each)"""
    _f16_block(tm, 256, 128, 8, 2, [('random', T)], seed=100 + T)


def test_f16_experts_skewed_routing(tm, cuda):
    """72 experts (the wide router), top-8, H 256 / I 256, routed_scale 2.5: one expert takes every token (row blocks past the
    first at every tile; at T = 300 five 64-row blocks), most experts have no rows, and an expert has exactly 2 * hint rows, another
    2 * hint + 1"""
    _f16_block(tm, 256, 256, 72, 8, [('one', 64), ('one', 300), ('edge', 64)], seed=7, scale=2.5)


def test_f16_forward_under_graph_capture(tm, cuda):
    """tm_moe_forward captured once and replayed once equals the eager result bit for bit"""
    H, I, E, k, T = 256, 128, 8, 2, 48
    rng = np.random.default_rng(8)
    h, _, _ = _small_f16_moe(tm, rng, H, I, E, k)
    try:
        xd = dev(rng.standard_normal((T, H)).astype(f16))
        ws = torch.full((tm.tm_moe_workspace(h, T),), 0xFF, dtype=torch.uint8, device='cuda')
        out = torch.zeros((T, H), dtype=torch.float16, device='cuda')
        ids = torch.zeros((T, k), dtype=torch.int32, device='cuda')
        w = torch.zeros((T, k), dtype=torch.float32, device='cuda')

        def run():
            _ffi.check(tm.tm_moe_forward(h, out.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), ids.data_ptr(), w.data_ptr(), st()))
        run()                      # eager (also prepares the block: the allocation happens here)
        torch.cuda.synchronize()
        eager = (host(out).copy(), host(ids).copy(), host(w).copy())
        assert np.isfinite(eager[0].astype(f32)).all() and np.abs(eager[0].astype(f32)).max() > 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        out.zero_(), ids.zero_(), w.zero_()
        ws.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out).view(np.uint16), eager[0].view(np.uint16)), 'replay: output'
        assert np.array_equal(host(ids), eager[1]) and np.array_equal(host(w).view(np.uint32), eager[2].view(np.uint32)), 'replay: routing'
    finally:
        tm.tm_moe_destroy(h)
        release_all()


def test_f16_forward_stages_equal_the_whole_forward(tm, cuda):
    """tm_moe_forward_stages(31) and the five launches enqueued one by one on one workspace give what tm_moe_forward gives"""
    H, I, E, k, T = 256, 128, 8, 2, 37
    rng = np.random.default_rng(5)
    h, _, _ = _small_f16_moe(tm, rng, H, I, E, k)
    try:
        xd = dev(rng.standard_normal((T, H)).astype(f16))
        outs = []
        for masks in ((31,), (1, 2, 4, 8, 16)):
            ws = torch.full((tm.tm_moe_workspace(h, T),), 0xFF, dtype=torch.uint8, device='cuda')
            out = torch.zeros((T, H), dtype=torch.float16, device='cuda')
            for m in masks:
                _ffi.check(tm.tm_moe_forward_stages(h, out.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), m, st()))
            torch.cuda.synchronize()
            outs.append(host(out).copy())
        whole = torch.zeros((T, H), dtype=torch.float16, device='cuda')
        ws = torch.full((tm.tm_moe_workspace(h, T),), 0xFF, dtype=torch.uint8, device='cuda')
        _ffi.check(tm.tm_moe_forward(h, whole.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), None, None, st()))
        torch.cuda.synchronize()
        assert np.isfinite(outs[0].astype(f32)).all() and np.abs(outs[0].astype(f32)).max() > 0
        assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16))
        assert np.array_equal(outs[0].view(np.uint16), host(whole).view(np.uint16))
    finally:
        tm.tm_moe_destroy(h)
        release_all()


def test_f16_shared_expert_block(tm, cuda):
    """tm_moe_forward_shared on an fp16 block against the formula of the header:
    out[t] = fp16( f32(shared[t]) * sigmoid(x_t . g) + sum_j w_j * f32(y_j) ), within 4e-3 + 2^-6 |ref|"""
    H, I, E, k, T = 256, 128, 8, 2, 37
    rng = np.random.default_rng(12)
    g = (0.05 * rng.standard_normal(H)).astype(f16)
    h, router, experts = _small_f16_moe(tm, rng, H, I, E, k, norm_topk=0, shared_gate=g)
    try:
        x = rng.standard_normal((T, H)).astype(f16)
        shared = (2.0 * rng.standard_normal((T, H))).astype(f16)
        cfg = Qwen2MoeConfig(hidden=H, layers=1, q_heads=1, kv_heads=1, head_dim=128, inter=I, vocab=8, moe_experts=E, moe_top_k=k,
                             moe_norm_topk=False)
        Lw = dict(moe_gate=router, experts=[], _dense=experts)
        ref = shared_combine(shared, x, g, routed_f32(x, Lw, cfg)).astype(f32)
        ws = torch.full((tm.tm_moe_workspace(h, T),), 0xFF, dtype=torch.uint8, device='cuda')
        out = torch.zeros((T, H), dtype=torch.float16, device='cuda')
        xd = dev(x)
        assert tm.tm_moe_forward(h, out.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), None, None, st()) != 0      # needs `shared`
        _ffi.check(tm.tm_moe_forward_shared(h, out.data_ptr(), xd.data_ptr(), dev(shared).data_ptr(), T, ws.data_ptr(), None, None, st()))
        torch.cuda.synchronize()
        got = host(out).astype(f32)
        tol = 4e-3 + 2.0**-6 * np.abs(ref)
        assert np.any(0.25 * np.abs(ref) > tol), 'outputs too small to test'
        err = np.abs(got - ref)
        print(f'f16 shared block: |ref| max {np.abs(ref).max():.3f}, worst err / tol {(err / tol).max():.3f}')
        assert np.all(err <= tol), f'err {err.max()} at {np.unravel_index(np.argmax(err - tol), err.shape)}'
    finally:
        tm.tm_moe_destroy(h)
        release_all()
