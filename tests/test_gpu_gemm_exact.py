"""Every GEMM tiling against exactly summable operands (tests/gemm_exact_reference.py; proved on the CPU by
tests/test_host_gemm_exact.py): every partial sum is representable in fp32, so the order of summation is out of the picture and
every tiling, split count, merge order and weight layout must return the same bits -- fp16(exact integer sum).  A mismatch is a
wrong, missing or duplicated term, an fp16 intermediate or a race, never an accumulation-order effect.

All comparisons are equalities of uint16 views, on the device.  The gated-SiLU outputs are the one exception: their accumulators
are exact, the only freedom left is expf, and they must lie within 1 fp16 ulp of o.gated_silu_epilogue of the exact accumulators
with equal inf / NaN patterns (the bound test_silu_mul_edges holds the same expression a / (1 + expf(-a)) to); the worst ulp per
family is printed.

Each configuration runs the dense x at every M of its family and the few-hot sweep (two non-zeros per row; every k index hit) at
one M.  The split-K workspace is allocated once per test, its slab area filled with 0xFF (fp32 NaN), its ticket tail zero as the
API requires, and never cleared again; configurations that split or merge run three times on it.

Configurations this module caught: none so far."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import gemm_exact_reference as r
from tests.gpu_helpers import dev, host, st, ulp_diff_f16
from tests.test_gpu_fullsize import _candidates as _p32_candidates
from tests.test_gpu_general_gemm import _tilings as _general_tilings

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
U4, F16, FP8 = 0, 1, 2
SENT = 0x7DAD                                                   # an fp16 NaN pattern no GEMM epilogue writes
MAX_M = 300
P32_SHAPES = [s for s in r.SHAPES if s[1] % 32 == 0]
CASES = [(K, N, 0) for K, N in P32_SHAPES] + [r.GATED_SHAPE + (1,)]
ALL_CASES = [(K, N, 0) for K, N in r.SHAPES] + [r.GATED_SHAPE + (1,)]
SPLITS = (1, 2, 3, 4, 7)
# test_w4a16_linear's tilings of the general kernel (+ the two more of test_w4a16_linear_prefill_tiles)
GENERAL = ((0, 0, 0), (1, 1, 4), (2, 2, 4), (4, 4, 4), (1, 2, 8), (2, 1, 8), (2, 16, 8), (1, 1, 0x108), (2, 2, 0x108), (2, 4, 0x108),
           (2, 2, 8), (2, 4, 8), (4, 1, 4))
PREFILL = ((0, 0, 0), (0, 1, 0x204), (0, 2, 0x204), (0, 3, 0x204), (0, 1, 0x205), (0, 2, 0x205), (0, 5, 0x205), (0, 1, 0x20c),
           (0, 2, 0x20c), (0, 3, 0x20c), (0, 1, 0x20d), (2, 1, 8), (2, 2, 8), (2, 4, 8), (4, 1, 4))

_DENSE = {}


def _ids(cases):
    return [f'{K}x{N}{"-gated" if g else ""}' for K, N, g in cases]


def _dense(K, N, gated, kind):
    """(x int [MAX_M][K], expected fp16 [MAX_M][N or N / 2]) of one operand kind ('w': u4 / fp16, 'w8': e4m3, 'w8g': gated e4m3),
    computed once; every M takes a prefix of the rows"""
    key = (K, N, gated, kind)
    if key not in _DENSE:
        W = r.weights(K, N, bool(gated))
        w = W.w() if kind == 'w' else W.w8(kind == 'w8g')
        x = r.dense_x(MAX_M, K, r.X_SEED)
        _DENSE[key] = (x, r.expected(x, w, W.lsb, gated=bool(gated)))
    return _DENSE[key]


def _create(tm, kind, K, N, gated, fp8_gated_scales=False):
    W = r.weights(K, N, bool(gated))
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_linear_create(_ffi.C.byref(h), K, N, kind, 128))
    if kind == U4:
        q, s, z = W.u4()
        _ffi.check(tm.tm_linear_prepare(h, dev(o.pack_u4_row(q)).data_ptr(), dev(s).data_ptr(), dev(z).data_ptr(), st()))
    elif kind == F16:
        _ffi.check(tm.tm_linear_prepare(h, dev(W.f16_weight()).data_ptr(), None, None, st()))
    elif fp8_gated_scales:
        codes, sc = W.fp8(gated=True)
        _ffi.check(tm.tm_linear_prepare_fp8_gated(h, dev(codes).data_ptr(), dev(sc).data_ptr(), st()))
    else:
        codes, sc = W.fp8()
        _ffi.check(tm.tm_linear_prepare(h, dev(codes).data_ptr(), dev(sc).data_ptr(), None, st()))
    torch.cuda.synchronize()
    return h, W


def _poisoned(nbytes, tail):
    """a workspace whose slab area is 0xFF and whose last `tail` bytes (the arrival counters) are zero"""
    ws = torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device='cuda')
    if tail:
        ws[nbytes - tail:] = 0
    return ws


def _reps(cfg):
    nt, splits, waves = cfg
    return 1 if splits == 1 else 3                              # split, merged and self-dispatched configurations: three launches


def _name(cfg):
    nt, splits, waves = cfg
    return f'nt {nt} splits {splits} waves {waves:#x}'


class _Runner:
    """one prepared linear, one never-cleared workspace; compares bits on the device"""

    def __init__(self, tm, h, K, N, gated, family, forward=None):
        self.tm, self.h, self.K, self.N, self.gated, self.family = tm, h, K, N, gated, family
        self.cols = N // 2 if gated else N
        self.ws = _poisoned(tm.tm_linear_workspace(h, MAX_M), 8192)
        self.forward = forward or self._forward
        self.compared, self.worst_ulp = 0, 0

    def _forward(self, x_d, M, cfg):
        nt, splits, waves = cfg
        y = torch.full((M, self.cols), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(self.tm.tm_linear_forward(self.h, x_d.data_ptr(), self.K, y.data_ptr(), self.cols, M, self.gated, nt, splits, waves,
                                             self.ws.data_ptr(), st()))
        return y

    def _where(self, M, cfg, r0, ks=None):
        KB, splits = self.K // 128, cfg[1]
        s = f'K {self.K} = {KB} k-blocks, M {M} (row block {r0 // 32} of 32, {r0 // 64} of 64)'
        if splits > 1:
            per = -(-KB // splits)
            s += f', {splits} splits of {per} k-blocks (before rounding to whole stages)'
            if ks is not None:
                s += ', the row\'s non-zeros: ' + ', '.join(f'k {k} = k-block {k // 128} in slice {k // 128 // per}' for k in ks)
        elif ks is not None:
            s += ', the row\'s non-zeros: ' + ', '.join(f'k {k} = k-block {k // 128}' for k in ks)
        return s

    def check(self, x_d, M, cfg, want_d, want, what, rows=None):
        """`want_d` on the device (fp16), `want` its numpy form (read only on a mismatch / for the gated ulp)"""
        for rep in range(_reps(cfg)):
            y = self.forward(x_d, M, cfg)
            bad = y.view(torch.int16) != want_d.view(torch.int16)
            if not bool(bad.any()):
                continue
            tag = f'{self.family} {self.K} x {self.N} {what} {_name(cfg)} launch {rep}'
            got = host(y)
            if self.gated:
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)]) \
                    and np.array_equal(np.isinf(got), np.isinf(want)), f'{tag}: inf / NaN pattern differs'
                ulp = ulp_diff_f16(np.nan_to_num(got), np.nan_to_num(want))
                self.worst_ulp = max(self.worst_ulp, int(ulp.max()))
                if ulp.max() <= 1:
                    continue
                r0, c0 = np.argwhere(ulp > 1)[0].tolist()
                n_bad = int((ulp > 1).sum())
            else:
                r0, c0 = bad.nonzero()[0].tolist()
                n_bad = int(bad.sum())
            ks = None if rows is None else (int(rows[0][r0]), int(rows[1][r0]))
            pytest.fail(f'{tag}: {n_bad} outputs differ, first at (row {r0}, column {c0}): got {float(got[r0, c0])!r} '
                        f'({got.view(np.uint16)[r0, c0]:#06x}) want {float(want[r0, c0])!r} ({want.view(np.uint16)[r0, c0]:#06x}); '
                        + self._where(M, cfg, r0, ks))
        self.compared += 1

    def dense(self, Ms, configs_of, kind='w'):
        x, want = _dense(self.K, self.N, self.gated, kind)
        for M in Ms:
            x_d, want_d = dev(x[:M].astype(f16)), dev(want[:M])
            for cfg in configs_of(M):
                self.check(x_d, M, cfg, want_d, want[:M], f'dense M {M}')

    def fewhot(self, M, configs, kind='w'):
        if self.gated:
            return                                              # exactly representable only before the SiLU
        W = r.weights(self.K, self.N, False)
        w = W.w() if kind == 'w' else W.w8()
        r.fewhot_check_budget(self.K, M, W.wint)
        for t in range(r.fewhot_launches(self.K, M)):
            x, want = r.fewhot_expected(self.K, M, t, w, W.lsb)
            rows = r.fewhot_rows(self.K, M, t)
            x_d, want_d = dev(x.astype(f16)), dev(want)
            for cfg in configs:
                self.check(x_d, M, cfg, want_d, want, f'few-hot M {M} launch {t}', rows)

    def report(self):
        print(f'{self.family} {self.K} x {self.N}{" gated" if self.gated else ""}: {self.compared} comparisons'
              + (f', worst gated ulp {self.worst_ulp}' if self.gated else ''))


def _p32(shape, splits):
    return (0, splits, 0x200 | shape)


def _k_splits(K, splits=SPLITS):
    return [s for s in splits if s <= max(1, K // 512)]


def _tuner(tm, K, N, M):
    """every (shape, splits) the start-up tuner may pick + the heuristic's own pick"""
    hs, hp = _ffi.C.c_int(0), _ffi.C.c_int(0)
    _ffi.check(tm.tm_debug_pick_tiling(K, N, M, 0, _ffi.C.byref(hs), _ffi.C.byref(hp)))
    return [_p32(s, p) for s, p in _p32_candidates(tm, K, N, M) + [(hs.value, hp.value)]]


def _unique(configs):
    return list(dict.fromkeys(configs))


@pytest.mark.parametrize('K,N,gated', CASES, ids=_ids(CASES))
def test_u4_decode_tiles(tm, cuda, K, N, gated):
    """gemm_decode.hip / gemm_decode_lc.hip at M <= 64: shapes 0-3, 6-9, 10 and 11 with 1, 2, 3, 4, 7 splits (<= K / 512), the
    in-launch merged shapes 16 + {0, 3, 6, 10}, the automatic pick and every tuner candidate; few-hot sweep at M = 64"""
    h, _ = _create(tm, U4, K, N, gated)
    run = _Runner(tm, h, K, N, gated, 'u4 decode tiles')
    fixed = [_p32(s, p) for s in (0, 1, 2, 3, 6, 7, 8, 9, 10, 11) for p in _k_splits(K)]
    fixed += [_p32(16 + s, p) for s in (0, 3, 6, 10) for p in _k_splits(K, (2, 3, 4, 7))]
    try:
        run.dense((1, 17, 33, 64), lambda M: _unique([(0, 0, 0)] + fixed + _tuner(tm, K, N, M)))
        run.fewhot(64, _unique([(0, 0, 0)] + fixed + _tuner(tm, K, N, 64)))
        run.report()
    finally:
        _ffi.check(tm.tm_linear_destroy(h))


@pytest.mark.parametrize('K,N,gated', CASES, ids=_ids(CASES))
def test_u4_row_block_tiles_above_64_rows(tm, cuda, K, N, gated):
    """shapes 6-9 (32-row blocks on grid.z) at M = 65, 100, 256, the automatic pick and every tuner candidate there (the 128-row
    tiles 4 / 5 among them); few-hot sweep at M = 100 (a ragged last row block)"""
    h, _ = _create(tm, U4, K, N, gated)
    run = _Runner(tm, h, K, N, gated, 'u4 row-block tiles')
    fixed = [_p32(s, p) for s in (6, 7, 8, 9) for p in _k_splits(K)]
    try:
        run.dense((65, 100, 256), lambda M: _unique([(0, 0, 0)] + fixed + _tuner(tm, K, N, M)))
        run.fewhot(100, _unique([(0, 0, 0)] + fixed + _tuner(tm, K, N, 100)))
        run.report()
    finally:
        _ffi.check(tm.tm_linear_destroy(h))


@pytest.mark.parametrize('K,N,gated', CASES, ids=_ids(CASES))
def test_u4_prefill_tiles(tm, cuda, K, N, gated):
    """M = 257, 300: the 128 x 256 / 128 x 512 tiles (0x204 / 0x205), the 256 x 256 LDS-dequantised tile (0x20c), the fp16 image
    (0x20d) with the split counts of test_w4a16_linear_prefill_tiles, the automatic pick, every tuner candidate; few-hot at 300"""
    h, _ = _create(tm, U4, K, N, gated)
    run = _Runner(tm, h, K, N, gated, 'u4 prefill tiles')
    fixed = [c for c in PREFILL if c[1] <= K // 128]
    try:
        run.dense((257, 300), lambda M: _unique(fixed + _tuner(tm, K, N, M)))
        run.fewhot(300, _unique(fixed + _tuner(tm, K, N, 300)))
        run.report()
    finally:
        _ffi.check(tm.tm_linear_destroy(h))


@pytest.mark.parametrize('K,N,gated', ALL_CASES, ids=_ids(ALL_CASES))
def test_u4_general_kernel(tm, cuda, K, N, gated):
    """gemm_w4a16.hip with u4 weights: the (nt, splits, waves) list of test_w4a16_linear at M = 1 .. 256 (N = 48: the only kernel
    that serves it); few-hot sweep at M = 256"""
    h, _ = _create(tm, U4, K, N, gated)
    run = _Runner(tm, h, K, N, gated, 'u4 general kernel')
    try:
        run.dense((1, 17, 33, 64, 65, 100, 256), lambda M: GENERAL)
        run.fewhot(256, GENERAL)
        run.report()
    finally:
        _ffi.check(tm.tm_linear_destroy(h))


@pytest.mark.parametrize('kind', [F16, FP8], ids=['f16', 'fp8'])
@pytest.mark.parametrize('K,N,gated', ALL_CASES, ids=_ids(ALL_CASES))
def test_f16_and_fp8_weight_only(tm, cuda, K, N, gated, kind):
    """the general kernel with fp16 and e4m3 weight-only weights: the automatic pick and every entry of
    tm_debug_general_candidates (+ the heuristic's) at M = 1 .. 256, the automatic pick at 257 and 300; few-hot at M = 64"""
    h, _ = _create(tm, kind, K, N, gated)
    run = _Runner(tm, h, K, N, gated, 'fp16 general kernel' if kind == F16 else 'e4m3 weight-only general kernel')
    op = 'w' if kind == F16 else 'w8'

    def configs(M):
        if M > 256:
            return [(0, 0, 0)]
        return _unique([(0, 0, 0)] + [(nt, sp, 0) for nt, sp in _general_tilings(tm, kind, 0, K, N, M, run.ws.numel() - 8192)])

    try:
        run.dense((1, 17, 33, 64, 65, 100, 256, 257, 300), configs, op)
        run.fewhot(64, configs(64), op)
        run.report()
    finally:
        _ffi.check(tm.tm_linear_destroy(h))


def _fp8_runner(tm, h, K, N, gated):
    run = _Runner(tm, h, K, N, gated, 'e4m3 x e4m3 (gemm_fp8.hip)')
    run.ws = _poisoned(tm.tm_linear_fp8_workspace(h, MAX_M), 0)

    def forward(x_d, M, cfg):
        y = torch.full((M, run.cols), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(tm.tm_linear_forward_fp8(h, x_d.data_ptr(), K, y.data_ptr(), run.cols, M, gated, cfg[1], run.ws.data_ptr(), st()))
        return y

    run.forward = forward
    return run


@pytest.mark.parametrize('K,N', P32_SHAPES, ids=[f'{K}x{N}' for K, N in P32_SHAPES])
def test_fp8_mfma_linear(tm, cuda, K, N):
    """tm_linear_forward_fp8: the activation quantiser's codes and scales (e4m3(64 x), 2^-6) bit for bit, then splits 0 .. 3 at
    M = 1, 17, 33, 64, 130 with the dense x and the few-hot sweep at M = 64"""
    h, _ = _create(tm, FP8, K, N, 0)
    run = _fp8_runner(tm, h, K, N, 0)
    splits = [(0, s, 0) for s in (0, 1, 2, 3) if s <= max(1, K // 512)]
    try:
        x = r.dense_x(MAX_M, K, r.X_SEED)[:130]
        ldsx = 132
        xq = torch.full((130, K), 0xFF, dtype=torch.uint8, device='cuda')
        sx = torch.zeros((K // 128, ldsx), dtype=torch.float32, device='cuda')
        _ffi.check(tm.tm_quant_fp8_rows(xq.data_ptr(), sx.data_ptr(), dev(x.astype(f16)).data_ptr(), K, 130, K, ldsx, st()))
        assert np.array_equal(host(xq), o.fp8_e4m3_from_f32((64 * x).astype(f32))), 'activation codes are not e4m3(64 x)'
        assert np.array_equal(host(sx)[:, :130].view(np.uint32), np.full((K // 128, 130), 2.0**-6, f32).view(np.uint32)), 'scales != 2^-6'
        run.dense((1, 17, 33, 64, 130), lambda M: splits, 'w8')
        run.fewhot(64, splits, 'w8')
        run.report()
    finally:
        _ffi.check(tm.tm_linear_destroy(h))


def test_fp8_mfma_linear_gated(tm, cuda):
    """the fused w1w3 form (tm_linear_prepare_fp8_gated: scale row [w1 blocks | w3 blocks]) with the gated-SiLU epilogue"""
    K, N = r.GATED_SHAPE
    h, _ = _create(tm, FP8, K, N, 1, fp8_gated_scales=True)
    run = _fp8_runner(tm, h, K, N, 1)
    try:
        run.dense((1, 17, 33, 64, 130), lambda M: [(0, s, 0) for s in (0, 1, 2, 3)], 'w8g')
        run.report()
    finally:
        _ffi.check(tm.tm_linear_destroy(h))
