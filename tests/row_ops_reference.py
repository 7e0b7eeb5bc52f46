"""Inputs and the kernel-order restatement for the RMSNorm edge tests (tests/test_gpu_row_ops.py on the device,
tests/test_host.py for the bound itself).

The norm tests hold y to "at most 1 fp16 ulp off o.rmsnorm on fewer than 0.1 % of the elements".  The 0.1 % is a cap, so the
inputs have to be able to meet it: o.rmsnorm sums the squares in fp64, the kernel in fp32 in a fixed order, and every row whose
fp32 `inv` lands on the other side of a rounding boundary moves a few of its elements by one ulp.  rmsnorm_kernel_order() is
that fixed order written out in numpy; the host test holds it to the same cap on exactly the tensors made here, so a device
failure means the kernel left its stated order, not that the inputs were unlucky.
"""
from __future__ import annotations

import numpy as np

from oracle import tm_oracle as o

f16, f32 = np.float16, np.float32

NORM_H = (8, 896, 1000, 3584, 5120)
NORM_EPS = (1e-5, 1e-6)
ROW_SCALE_LOG2 = (-12, -6, 0, 6, 10)         # row i is scaled by 2**ROW_SCALE_LOG2[i % 5]
RESIDUAL_CASES = ((5, 896, 1, False), (5, 5120, 2, True), (3, 1000, 5, False), (4, 3584, 8, True))


def norm_geometry(H):
    """norm_row.h norm_geometry: (threads, vectors per thread)"""
    nvec = H // 8
    t = min((nvec + 63) // 64 * 64, 512)
    return t, (nvec + t - 1) // t


def _row_scales(M):
    return np.exp2(np.asarray(ROW_SCALE_LOG2, f32)[np.arange(M) % 5])[:, None]


def norm_rows(H):
    """M rows (M * H >= 16384, so that one element is below the 0.1 % share), at least one of every scale and an all-zero row"""
    return max(-(-16384 // H), 2 * len(ROW_SCALE_LOG2))


def rmsnorm_inputs(H):
    """-> x [M, H], w [H], index of the all-zero row"""
    M = norm_rows(H)
    rng = np.random.default_rng(1000 + H)
    x = (rng.standard_normal((M, H)).astype(f32) * _row_scales(M)).astype(f16)
    zero_row = 7                                  # a row of scale 2**0 otherwise
    x[zero_row] = 0
    w = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    return x, w, zero_row


def residual_inputs(M, H, splits, bias):
    """-> resid [M, H], hidden [M, H] or None, partial fp32 [splits, M, H] or None, bias [H] or None, w [H]
    splits == 0: the fp16 `hidden` form; otherwise `partial` are the split-K slabs of the producing GEMM"""
    rng = np.random.default_rng(77 + 31 * M + H + splits)
    sc = _row_scales(M)
    r = (rng.standard_normal((M, H)).astype(f32) * sc).astype(f16)
    w = (1 + 0.02 * rng.standard_normal(H)).astype(f16)
    b = (0.1 * rng.standard_normal(H)).astype(f16) if bias else None
    if splits:
        return r, None, (0.3 * rng.standard_normal((splits, M, H)).astype(f32) * sc[None]).astype(f32), b, w
    return r, (rng.standard_normal((M, H)).astype(f32) * sc).astype(f16), None, b, w


def sum_partials(part):
    """the slabs summed in order in fp32 from 0, then the GEMM's fp16 output rounding (norm_row.h, MODE 2)"""
    acc = np.zeros(part.shape[1:], f32)
    for s in range(part.shape[0]):
        acc = acc + part[s]
    return acc.astype(f16)


def rmsnorm_kernel_order(x, w, eps):
    """o.rmsnorm with the sum of squares in rmsnorm_kernel's fp32 order (norm_row.h): thread t owns the 16-byte vectors
    t, t + threads, ... and runs one fma chain over their elements in memory order (x^2 of an fp16 is exact in fp32, so the
    fma rounds like an add); the 64 lanes of a wave are combined as a pairwise tree (group_sum<64>: xor 1, 2, half mirror,
    rotate 8, xor 16, xor 32 -- each step adds the two neighbouring subtrees, in either order); the waves are then added in
    order from 0.  inv = 1 / sqrt(ss / H + eps) in fp32; y = h(h(f32(x) * inv) * w) as in the oracle."""
    x = np.asarray(x, f16)
    M, H = x.shape
    threads, nv = norm_geometry(H)
    nvec = H // 8
    xf = x.astype(f32)
    sq = (xf * xf).reshape(M, nvec, 8)
    lane = np.zeros((M, threads), f32)
    for i in range(nv):
        n = min(threads, nvec - i * threads)     # threads whose i-th vector lies inside the row
        for e in range(8):
            lane[:, :n] = lane[:, :n] + sq[:, i * threads:i * threads + n, e]
    acc = lane.reshape(M, threads // 64, 64)
    for _ in range(6):
        acc = acc[..., 0::2] + acc[..., 1::2]
    ss = np.zeros((M, 1), f32)
    for wv in range(threads // 64):
        ss = ss + acc[:, wv]
    inv = f32(1) / np.sqrt(ss / f32(H) + f32(eps))
    return o.hmul((xf * inv).astype(f16), np.asarray(w, f16))
