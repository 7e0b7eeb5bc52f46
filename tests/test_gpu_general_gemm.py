"""GPU parity of the general GEMM (gemm_kernel, gemm_w4a16.hip) at the published geometries, over every tiling the start-up tuner
may time.  With fp16 weights it is every model's lm_head; with e4m3 weight-only weights it runs Mixtral's dense w_qkv / wo.  The
timed configuration must be a tested tiling: each sweep takes tm_debug_general_candidates (= gen_dense_candidates, the list
tune_aux_gemms walks) with a workspace large enough for every split the K rule allows -- a superset of what any engine's workspace
admits -- plus the heuristic's own pick (tm_debug_pick_general), and asserts that the list is not empty.

Every forward writes into a y of ldy > N with 16 extra rows, all set to a sentinel NaN pattern: the columns past N and the rows past M
must come back untouched (the partial last workgroup at N = 16032, row tiles that overrun M).  At M = 64 a one-hot x (64 distinct
rows of the identity) must return those weight rows exactly: a mis-packed, transposed or swapped 16-column tile fails there even
where a tolerance would forgive it.

References are float64 products of the exact fp16 (or dequantised e4m3) operands, computed in column blocks.  Tolerances are the
ones of test_f16_linear / test_fp8_linear (fp16 1e-3 + 2^-10 |ref|, fp8 2e-3 + 2^-10 |ref|); every case asserts that they would
reject an all-zero output and 0.75 ref on at least 90 % of the entries.  One full-size weight is resident at a time."""
import math

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16 = np.float16
F16, FP8 = 1, 2
SENT = 0x7DAD                     # an fp16 NaN pattern no GEMM epilogue writes
FLT_MAX = float(np.finfo(np.float32).max)
EPS = float(np.float32(1e-9))

# (K, N): Llama-3-8B (headline), InternLM2-20B, Llama-3-70B on one TP = 8 rank (N % 128 = 32: the last workgroup is partial for
# both nt), Mixtral at TP = 1 / one TP = 2 rank
HEADLINE = (4096, 128256)
HEADS = [(6144, 92544), (8192, 16032), (4096, 32000), (4096, 16000)]
# Mixtral fp8 weight-only (K, N, role): w_qkv / wo at TP = 1, then one TP = 2 rank (KB 16 for wo: split <= 2)
FP8_SHAPES = [(4096, 6144, 1), (4096, 4096, 2), (4096, 3072, 1), (2048, 4096, 2)]

_HELD = []


@pytest.fixture(scope='module', autouse=True)
def _free_linears(tm):
    yield
    _release(tm)


def _release(tm):
    for h in _HELD:
        _ffi.check(tm.tm_linear_destroy(h))
    _HELD.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _f16_weight(K, N, seed):
    """random fp16 codes: sign and mantissa uniform, magnitudes over [2^-8, 2^-4) (rms ~ 0.03: logits of a few units for unit x),
    with planted subnormals and zeros"""
    rng = np.random.default_rng(seed)
    w = np.empty((K, N), np.uint16)
    for k in range(0, K, 512):
        b = rng.integers(0, 1 << 16, (min(512, K - k), N), dtype=np.uint16)
        w[k:k + 512] = (b & 0x83FF) | ((7 + ((b >> 10) & 3)) << 10)
    w[::97, ::89] &= 0x83FF                                     # subnormal (or signed zero) codes
    w[3::101, 7::83] = 0
    return w.view(f16)


def _fp8_weight(K, N, seed):
    """e4m3 codes + 128 x 128 block scales quantised from N(0, 1/K) weights, with planted subnormal and +-448 codes (as
    test_fp8_linear); returns (codes, scales, dequantised fp16 operand)"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((K, N), dtype=np.float32) * np.float32(1.0 / math.sqrt(K))
    q, sc = o.fp8_quantize_blockwise(w)
    q[::37, ::11] = 0x01                                        # subnormal codes
    q[5::53, 3::7] = 0xFE                                       # -448
    q[11::41, 5::13] = 0x7E                                     # +448
    return q, sc, o.fp8_dequant(q, sc)


def _prepare(tm, K, N, wt, seed):
    """create + prepare one linear (the previous one is destroyed first); returns (handle, fp16 operand [K][N])"""
    _release(tm)
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_linear_create(_ffi.C.byref(h), K, N, wt, 128))
    _HELD.append(h)
    if wt == F16:
        wd = _f16_weight(K, N, seed)
        w_d = torch.from_numpy(wd).cuda()
        _ffi.check(tm.tm_linear_prepare(h, w_d.data_ptr(), None, None, st()))
        bufs = [w_d]
    else:
        q, sc, wd = _fp8_weight(K, N, seed)
        bufs = [torch.from_numpy(q).cuda(), torch.from_numpy(sc).cuda()]
        _ffi.check(tm.tm_linear_prepare(h, bufs[0].data_ptr(), bufs[1].data_ptr(), None, st()))
    torch.cuda.synchronize()
    del bufs
    torch.cuda.empty_cache()
    return h, wd


def _ref64(x16, wd, cb=4096):
    """float64 x . W from the exact fp16 operands, in column blocks of W"""
    x = x16.astype(np.float64)
    out = np.empty((x.shape[0], wd.shape[1]), np.float64)
    for j in range(0, wd.shape[1], cb):
        out[:, j:j + cb] = x @ wd[:, j:j + cb].astype(np.float64)
    return out


def _candidates(tm, wt, K, N, M, ws_bytes):
    nt, sp = np.zeros(16, np.int32), np.zeros(16, np.int32)
    n = _ffi.C.c_int(-1)
    _ffi.check(tm.tm_debug_general_candidates(wt, K, N, M, ws_bytes, nt.ctypes.data, sp.ctypes.data, 16, _ffi.C.byref(n)))
    assert 0 <= n.value <= 16
    return list(zip(nt[:n.value].tolist(), sp[:n.value].tolist()))


def _heuristic(tm, wt, role, K, N, M):
    v = (_ffi.C.c_int * 4)()
    _ffi.check(tm.tm_debug_pick_general(wt, role, K, N, M, v))
    return (v[0], v[1])


def _tilings(tm, wt, role, K, N, M, ws_bytes):
    """every tuner candidate (a non-empty list) + the heuristic's pick, each once"""
    cands = _candidates(tm, wt, K, N, M, ws_bytes)
    assert cands, f'no tuner candidates for {K} x {N} at M = {M}'
    return list(dict.fromkeys(cands + [_heuristic(tm, wt, role, K, N, M)]))


def _x_dev(x16, ldx):
    """x [M][K] on the device with row stride ldx; padding columns are NaN (a read of them poisons the row)"""
    M, K = x16.shape
    if ldx == K:
        return dev(x16)
    xp = np.full((M, ldx), np.nan, f16)
    xp[:, :K] = x16
    return dev(xp)


def _workspace(M, N, splits):
    """the fp32 split-K slabs of one forward (gemm_workspace_bytes)"""
    return torch.zeros(max(1, splits * M * N * 4 if splits > 1 else 1), dtype=torch.uint8, device='cuda')


def _forward(tm, h, x_d, ldx, M, N, nt, sp, ws, ldy):
    y = torch.full((M + 16, ldy), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
    _ffi.check(tm.tm_linear_forward(h, x_d.data_ptr(), ldx, y.data_ptr(), ldy, M, 0, nt, sp, 0, ws.data_ptr(), st()))
    return y


def _untouched(y, M, N, what):
    v = y.view(torch.int16)
    assert bool((v[:M, N:] == SENT).all()), f'{what}: columns past N written ({int((v[:M, N:] != SENT).sum())} entries)'
    assert bool((v[M:] == SENT).all()), f'{what}: rows past M written ({int((v[M:] != SENT).sum())} entries)'


class _Bound:
    """the reference on the device and its tolerance; asserts the tolerance rejects a zero output and 0.75 ref"""

    def __init__(self, ref64, atol, what):
        self.ref = torch.from_numpy(ref64.astype(np.float32)).cuda()
        self.tol = atol + 2.0**-10 * self.ref.abs()
        for scale in (0.0, 0.75):
            caught = float(((self.ref * (1.0 - scale)).abs() > self.tol).float().mean())
            assert caught >= 0.9, f'{what}: the tolerance would accept {scale} x ref on {1 - caught:.1%} of the entries'

    def check(self, y, M, N, what):
        _untouched(y, M, N, what)
        err = (y[:M, :N].float() - self.ref).abs()
        ok = err <= self.tol                                    # NaN (an unwritten sentinel) fails
        if not bool(ok.all()):
            bad = (~ok).nonzero()
            r, c = bad[0].tolist()
            pytest.fail(f'{what}: {bad.shape[0]} entries out of tolerance, first at ({r}, {c}): got {float(y[r, c])} ref '
                        f'{float(self.ref[r, c])}; max err {float(torch.nan_to_num(err, nan=float("inf")).max())}')
        return err


def _one_hot_check(tm, h, wd, wt, K, N, tilings, ws, seed, what):
    """M = 64 distinct identity rows: y = those weight rows, exactly (fp8: bit exact in the normal fp16 range; fp16 subnormal
    products may be flushed by the matrix core there, as test_fp8_linear allows)"""
    rows = np.random.default_rng(seed).permutation(K)[:64]
    x = np.zeros((64, K), f16)
    x[np.arange(64), rows] = 1
    x_d = dev(x)
    exp = torch.from_numpy(np.ascontiguousarray(wd[rows])).cuda()
    normal = exp.float().abs() >= 2.0**-14
    for nt, sp in tilings:
        tag = f'{what} one-hot nt {nt} splits {sp}'
        y = _forward(tm, h, x_d, K, 64, N, nt, sp, ws, N + 64)
        _untouched(y, 64, N, tag)
        got = y[:64, :N]
        if wt == F16:
            bad = got.float() != exp.float()                    # values (+0 == -0): every fp16 weight passes unrounded
        else:
            bad = (got.view(torch.int16) != exp.view(torch.int16)) & normal
            bad |= ((got.float() - exp.float()).abs() > 2.0**-14) & ~normal
        if bool(bad.any()):
            r, c = bad.nonzero()[0].tolist()
            pytest.fail(f'{tag}: {int(bad.sum())} weights differ, first at row {r} col {c}: got {float(got[r, c])} want '
                        f'{float(exp[r, c])}')


def _sweep(tm, h, wd, wt, role, K, N, Ms, atol, seed, what, ldx_pad=()):
    """every tuner candidate + the heuristic at each M (prefix rows of one x), the one-hot check at M = 64"""
    ws = torch.zeros(tm.tm_linear_workspace(h, max(Ms)), dtype=torch.uint8, device='cuda')
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((max(Ms), K), dtype=np.float32).astype(f16)
    REF = _ref64(X, wd)
    ran = 0
    for M in Ms:
        ldx = K + 40 if M in ldx_pad else K
        x_d = _x_dev(X[:M], ldx)
        bound = _Bound(REF[:M], atol, f'{what} M {M}')
        tilings = _tilings(tm, wt, role, K, N, M, ws.numel())
        worst = 0.0
        for nt, sp in tilings:
            tag = f'{what} M {M} ldx {ldx} nt {nt} splits {sp}'
            err = bound.check(_forward(tm, h, x_d, ldx, M, N, nt, sp, ws, N + 64), M, N, tag)
            worst = max(worst, float((err / bound.tol).max()))
            ran += 1
        print(f'{what} M {M}: {len(tilings)} tilings {tilings}, worst err / tol {worst:.3f}')
        if M == 64:
            _one_hot_check(tm, h, wd, wt, K, N, tilings, ws, seed + 1, what)
    return ran


def test_lm_head_headline_every_candidate(tm, cuda):
    """Llama-3-8B head (4096 x 128256) at 1 .. 256 rows across the 16 / 32 / 64-row tile boundaries; x with ldx > K at two M"""
    K, N = HEADLINE
    h, wd = _prepare(tm, K, N, F16, 1)
    _sweep(tm, h, wd, F16, 5, K, N, (1, 16, 17, 33, 64, 100, 128, 256), 1e-3, 11, 'lm_head 4096 x 128256', ldx_pad=(33, 100))


@pytest.mark.parametrize('K,N', HEADS)
def test_lm_head_every_candidate(tm, cuda, K, N):
    h, wd = _prepare(tm, K, N, F16, K + N)
    _sweep(tm, h, wd, F16, 5, K, N, (1, 64, 128), 1e-3, K * 3 + N, f'lm_head {K} x {N}')


def test_lm_head_largest_supported(tm, cuda):
    """Llama-3-70B head at tp = 1 (8192 x 128256): the packed image is 2 101 346 304 B, 97.9 % of the 2^31 the kernel addresses"""
    K, N = 8192, 128256
    h, wd = _prepare(tm, K, N, F16, 70)
    _sweep(tm, h, wd, F16, 5, K, N, (64,), 1e-3, 71, 'lm_head 8192 x 128256')


def _nll64(logits, tgt):
    """float64 NLL per row, the formula of tm_cross_entropy (max from -FLT_MAX, + 1e-9 inside the log)"""
    m = np.maximum(logits.max(axis=1), -FLT_MAX)
    s = np.exp(logits - m[:, None]).sum(axis=1)
    return np.log(s + EPS) + m - logits[np.arange(len(logits)), tgt]


@pytest.mark.parametrize('K,N', [HEADLINE, (6144, 92544)])
def test_lm_head_scoring_rows_and_cross_entropy(tm, cuda, K, N):
    """Pipeline.get_ppl runs the head over up to 1024 rows per chunk into a buffer of ld = vocab rounded up to 8, then
    tm_cross_entropy.  M > 256: the heuristic alone serves (no tuner candidates) -- run it and an explicit nt = 1, ldy = N + 8, then
    the NLLs against float64 NLLs of the float64 logits: the CE bound of test_gpu_cross_entropy plus 2 max |d logit| of the row
    (the NLL is 2-Lipschitz in the max-norm of the logits)."""
    h, wd = _prepare(tm, K, N, F16, K + 2 * N)
    rng = np.random.default_rng(K + N)
    X = rng.standard_normal((1024, K), dtype=np.float32).astype(f16)
    REF = _ref64(X, wd)
    ldy = N + 8
    for M in (257, 1000, 1024):
        assert _candidates(tm, F16, K, N, M, tm.tm_linear_workspace(h, M)) == []
        tgt = rng.integers(0, N, M).astype(np.int32)
        nll_ref = _nll64(REF[:M], tgt)
        bound = _Bound(REF[:M], 1e-3, f'{K} x {N} M {M}')
        x_d, tgt_d = dev(X[:M]), dev(tgt)
        for nt, sp in list(dict.fromkeys([_heuristic(tm, F16, 5, K, N, M), (1, 1)])):
            what = f'lm_head {K} x {N} M {M} nt {nt} splits {sp}'
            y = _forward(tm, h, x_d, K, M, N, nt, sp, _workspace(M, N, sp), ldy)
            err = bound.check(y, M, N, what)
            nll = torch.full((M,), -7.0, dtype=torch.float32, device='cuda')
            _ffi.check(tm.tm_cross_entropy(nll.data_ptr(), y.data_ptr(), tgt_d.data_ptr(), M, N, ldy, st()))
            got = host(nll).astype(np.float64)
            dlogit = host(err.max(dim=1).values).astype(np.float64)
            d = np.abs(got - nll_ref)
            lim = 5e-5 + 1e-5 * np.abs(nll_ref) + 2 * dlogit
            assert np.all(d <= lim), f'{what}: NLL off by {d.max()} (row {int(np.argmax(d - lim))})'
            print(f'{what}: max |d logit| {dlogit.max():.2e}, max |d nll| {d.max():.2e}')


@pytest.mark.parametrize('K,N,role', FP8_SHAPES)
def test_fp8_weight_only_every_candidate(tm, cuda, K, N, role):
    """Mixtral's dense e4m3 weight-only linears (general kernel, weight type 2): every candidate + the heuristic at decode rows,
    the heuristic at prefill rows (300, 1000), the one-hot check at M = 64"""
    h, wd = _prepare(tm, K, N, FP8, K + N + role)
    what = f'fp8 {K} x {N}'
    _sweep(tm, h, wd, FP8, role, K, N, (1, 17, 64, 128, 256), 2e-3, K + N, what)
    rng = np.random.default_rng(K * N)
    X = rng.standard_normal((1000, K), dtype=np.float32).astype(f16)
    REF = _ref64(X, wd)
    for M in (300, 1000):
        assert _candidates(tm, FP8, K, N, M, tm.tm_linear_workspace(h, M)) == []
        nt, sp = _heuristic(tm, FP8, role, K, N, M)
        tag = f'{what} M {M} heuristic nt {nt} splits {sp}'
        y = _forward(tm, h, dev(X[:M]), K, M, N, nt, sp, _workspace(M, N, sp), N + 64)
        _Bound(REF[:M], 2e-3, tag).check(y, M, N, tag)
