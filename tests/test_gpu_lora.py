"""The multi-LoRA delta launch (lora.hip) through the C-ABI against the float64 form of its contract:
    t = fp16(x[m] . A_a^T),   y[m][n] = fp16(y[m][n] + sum_r t[r] B_a[n][r])   for rows with an adapter id, nothing else written.
Exact test: integer operands (x in [-2, 2], A four non-zeros per rank row, B in {-1, 0, 1}, base in [-400, 400]) keep |t| <= 16 and every
sum below 400 + 64 * 16 < 2048, so all three roundings are exact and every bit must match.  y is wider than N and pre-filled with an fp16
NaN pattern, rows without an adapter over their whole width; the whole buffer is compared.
Random test: Gaussian B and base; x and A are Gaussian draws on the 2^-4 / 2^-6 grids (|x| <= 4, |A| <= 1), so the K-long fp32 sum of the
shrink is exact in any order and the device's t IS the reference's.  Left is the expand: n = R_pad + 1 fp32 terms (exact products, the base
value) summed in the matrix core's order, each addition within 2^-23 relative (its adds need not round to nearest), one fp16 rounding --
against the float64 y_ref BEFORE that rounding:  |err| <= 2^-11 |y_ref| + c 2^-24 (|y_base| + sum |t| |B|),  c = 2 (R_pad + 1)."""
import ctypes as C

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16 = np.float16
POISON = 0x7DAD
# (K, N) -> segment ends of the three-segment table; K = 144: the K % 32 == 16 tail; N = 528 / 1040 at M = 1024: 128- / 256-column tiles
SHAPES = {(128, 48): (16, 32, 48), (384, 272): (128, 192, 272), (144, 80): (16, 48, 80), (128, 528): (256, 400, 528), (128, 1040): (512, 768, 1040)}
_pad16 = lambda r: -(-r // 16) * 16      # noqa: E731


def _case(M, K, N, rank, nseg, exact, seed):
    """operands of 3 adapters in a 4-slot table; slot 1 of a three-segment table leaves the middle segment alone"""
    rng = np.random.default_rng(seed)
    ends = SHAPES[(K, N)] if nseg == 3 else (N,)
    begins = (0,) + ends[:-1]
    ids = np.array([(0, 1, 2, -1)[m % 4] for m in range(M)], np.int32)
    Rp = _pad16(rank)
    if exact:
        x = rng.integers(-2, 3, (M, K)).astype(f16)
        base = rng.integers(-400, 401, (M, N)).astype(f16)
    else:
        x = (np.clip(np.round(rng.standard_normal((M, K)) * 16), -64, 64) / 16).astype(f16)
        base = rng.standard_normal((M, N)).astype(f16)
    slots = []
    for s in range(3):
        ranks = [0 if (nseg == 3 and s == 1 and g == 1) else Rp for g in range(nseg)]
        A = np.zeros((sum(ranks), K), f16)
        B = np.zeros((N, Rp), f16)
        toff = 0
        for g in range(nseg):
            if ranks[g] == 0:
                continue
            if exact:
                for r in range(rank):
                    A[toff + r, rng.choice(K, 4, replace=False)] = rng.choice([-2, -1, 1, 2], 4)
                B[begins[g]:ends[g], :rank] = rng.integers(-1, 2, (ends[g] - begins[g], rank))
            else:
                A[toff:toff + rank] = np.clip(np.round(rng.standard_normal((rank, K)) * 0.25 * 64), -64, 64) / 64
                B[begins[g]:ends[g], :rank] = rng.standard_normal((ends[g] - begins[g], rank)) * 0.5
            toff += ranks[g]
        slots.append((A, B, ranks))
    return x, base, ids, slots, begins, ends


def _reference(x, base, ids, slots, begins, ends):
    """float64 contract -> (y fp16, y before its last rounding, error scale |y_base| + sum |t| |B|)"""
    y, y64, mag = base.copy(), base.astype(np.float64), np.abs(base.astype(np.float64))
    for m, a in enumerate(ids):
        if a < 0:
            continue
        A, B, ranks = slots[a]
        t = (x[m].astype(np.float64) @ A.astype(np.float64).T).astype(f16).astype(np.float64)
        toff = 0
        for g, R in enumerate(ranks):
            if R:
                Bg = B[begins[g]:ends[g], :R].astype(np.float64)
                y64[m, begins[g]:ends[g]] += Bg @ t[toff:toff + R]
                y[m, begins[g]:ends[g]] = y64[m, begins[g]:ends[g]].astype(f16)
                mag[m, begins[g]:ends[g]] += np.abs(Bg) @ np.abs(t[toff:toff + R])
            toff += R
    return y, y64, mag


def _run(x, base, ids, slots, begins, ends, ldx_pad=8, ldy_pad=12):
    """-> (y buffer after the launch, the same buffer as it was before) as uint16 [M][ldy]"""
    tm = _ffi.load()
    M, K = x.shape
    N = base.shape[1]
    xb = np.zeros((M, K + ldx_pad), f16)
    xb[:, :K] = x
    yb = np.full((M, N + ldy_pad), POISON, np.uint16)
    yb[ids >= 0, :N] = base[ids >= 0].view(np.uint16)
    tab = C.c_void_p()
    nseg = len(ends)
    _ffi.check(tm.tm_lora_table_create(C.byref(tab), K, N, nseg, (C.c_int * nseg)(*begins), (C.c_int * nseg)(*ends), 4))
    try:
        for s, (A, B, ranks) in enumerate(slots):
            _ffi.check(tm.tm_lora_table_set(tab, s, A.ctypes.data, B.ctypes.data, (C.c_int * nseg)(*ranks), B.shape[1]))
        ws = torch.zeros(tm.tm_lora_plan_workspace(M), dtype=torch.uint8, device='cuda')
        d_ids, d_x, d_y = dev(ids), dev(xb), dev(yb.view(np.int16))
        _ffi.check(tm.tm_lora_plan(ws.data_ptr(), d_ids.data_ptr(), ids.ctypes.data, M, 4, st()))
        _ffi.check(tm.tm_lora_apply(tab, d_x.data_ptr(), K + ldx_pad, d_y.data_ptr(), N + ldy_pad, M, ws.data_ptr(), st()))
        torch.cuda.synchronize()
        return host(d_y).view(np.uint16), yb
    finally:
        tm.tm_lora_table_destroy(tab)


@pytest.mark.parametrize('M,rank,nseg,K,N', [(M, r, g, K, N) for K, N in list(SHAPES)[:3] for g in (1, 3) for r in (8, 16, 64) for M in (1, 17, 50)]
                         + [(1024, 16, 3, 128, 528), (1024, 64, 1, 128, 1040)])
def test_lora_delta_exact(M, rank, nseg, K, N):
    case = _case(M, K, N, rank, nseg, True, seed=M * 1000 + rank * 10 + nseg)
    x, base, ids = case[:3]
    ref, _, _ = _reference(*case)
    got, want = _run(*case)
    want[ids >= 0, :N] = ref[ids >= 0].view(np.uint16)
    assert np.abs(ref.astype(np.float64)).max() < 2048
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{len(bad)} elements differ, first (row, column) {bad[0].tolist()}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}'


@pytest.mark.parametrize('nseg', [1, 3])
@pytest.mark.parametrize('rank', [16, 64])
def test_lora_delta_random(rank, nseg):
    M, K, N = 50, 384, 272
    case = _case(M, K, N, rank, nseg, False, seed=7 + rank + nseg)
    ids = case[2]
    _, ref, mag = _reference(*case)     # the float64 value: the fp16 rounding of y is the kernel's own error
    got, before = _run(*case)
    assert np.array_equal(got[:, N:], before[:, N:]) and np.array_equal(got[ids < 0], before[ids < 0])
    live = ids >= 0
    err = np.abs(got[live, :N].view(f16).astype(np.float64) - ref[live].astype(np.float64))
    c = 2 * (_pad16(rank) + 1)
    bound = 2.0 ** -11 * np.abs(ref[live].astype(np.float64)) + c * 2.0 ** -24 * mag[live]
    print(f'rank {rank} segments {nseg}: worst err / bound {np.max(err / bound):.3f}')
    assert np.all(err <= bound)


def test_lora_refusals():
    tm = _ffi.load()
    tab, one, end = C.c_void_p(), (C.c_int * 1)(0), (C.c_int * 1)(64)
    assert tm.tm_lora_table_create(C.byref(tab), 128, 64, 1, one, end, 9) == 1 and 'at most 8 adapter slots' in _ffi.last_error()
    assert tm.tm_lora_table_create(C.byref(tab), 120, 64, 1, one, end, 4) == 1 and 'multiples of 16' in _ffi.last_error()
    _ffi.check(tm.tm_lora_table_create(C.byref(tab), 128, 64, 1, one, end, 4))
    try:
        A, B = np.zeros((80, 128), f16), np.zeros((64, 80), f16)
        assert tm.tm_lora_table_set(tab, 0, A.ctypes.data, B.ctypes.data, (C.c_int * 1)(80), 80) == 1
        assert 'rank over 64 per segment' in _ffi.last_error()
        ws = torch.zeros(tm.tm_lora_plan_workspace(4), dtype=torch.uint8, device='cuda')
        ids = np.array([0, 4, -1, 1], np.int32)
        assert tm.tm_lora_plan(ws.data_ptr(), dev(ids).data_ptr(), ids.ctypes.data, 4, 4, st()) == 1
        assert 'adapter id outside [-1, slots)' in _ffi.last_error()
        x = dev(np.zeros((4, 128), f16))
        assert tm.tm_lora_apply(None, x.data_ptr(), 128, x.data_ptr(), 128, 4, ws.data_ptr(), st()) == 1 and 'null table' in _ffi.last_error()
    finally:
        tm.tm_lora_table_destroy(tab)
