"""The group-32 W4A16 linear (gemm_u4_g32.hip) through the C-ABI: tm_linear_create(TM_WEIGHT_U4, 32) / tm_linear_prepare /
tm_linear_dequant_f16 / tm_linear_forward.

  * the repacked image dequantises to oracle.w4a16_dequant(group=32) bit for bit (tm_linear_dequant_f16 runs the GEMM's own dequantisation);
  * exactly summable operands (the technique of tests/test_gpu_gemm_exact.py with groups of 32): W = (q - z) 2^e with a DIFFERENT power
    of two in every group of a column and zeros drawn per (group, column), integer x -- every partial sum is representable in fp32, so
    every M class and every split of K must return the same bits, and a pair taken from a neighbouring group or column gives another
    integer.  The gated outputs are held to 1 fp16 ulp of the oracle's epilogue of the exact accumulators (expf is the only freedom left);
  * random operands against oracle.w4a16_linear(group=32) with the tolerance tests/test_gpu_ops.py holds the u4 linear to
    (2e-3 + 2^-10 |ref|; its gated cases: 2e-3 + 2^-9 |ref|);
  * refusals: group 64 at creation, a mixture-of-experts engine with group 32."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
SENT = 0x7DAD                                                   # an fp16 NaN pattern no kernel writes
G = 32
KS, NS, MS = (128, 384), (32, 96, 160), (1, 7, 64, 65, 130)
GATED_NS = (64, 192)


class _Linear:
    def __init__(self, tm, q, s, z):
        self.tm, (self.K, self.N) = tm, q.shape
        self.h = _ffi.C.c_void_p()
        _ffi.check(tm.tm_linear_create(_ffi.C.byref(self.h), self.K, self.N, 0, G))
        _ffi.check(tm.tm_linear_prepare(self.h, dev(o.pack_u4_row(q)).data_ptr(), dev(np.asarray(s, f16)).data_ptr(),
                                        dev(np.asarray(z, f16)).data_ptr(), st()))
        torch.cuda.synchronize()

    def dequant(self):
        out = torch.full((self.N, self.K), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(self.tm.tm_linear_dequant_f16(self.h, out.data_ptr(), st()))
        return host(out).T

    def __call__(self, x, gated=False, splits=0):
        """y with one NaN-poisoned row behind the last one, which must come back untouched; the workspace is poisoned too"""
        M, ldy = x.shape[0], self.N // 2 if gated else self.N
        ws = torch.full((max(1, self.tm.tm_linear_workspace(self.h, M)),), 0xFF, dtype=torch.uint8, device='cuda')
        y = torch.full((M + 1, ldy), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(self.tm.tm_linear_forward(self.h, dev(x).data_ptr(), self.K, y.data_ptr(), ldy, M, int(gated), 0, splits, 0,
                                             ws.data_ptr(), st()))
        got = host(y)
        assert (got[M].view(np.uint16) == SENT).all(), 'the row behind the last one was written'
        return got[:M]

    def close(self):
        self.tm.tm_linear_destroy(self.h)


def _splits(K):
    """every split-K depth the launcher can run for K (0 = its own pick): ceil(KB / ceil(KB / s)) over s = 1 .. KB"""
    KB = K // 128
    return [0] + sorted({-(-KB // -(-KB // s)) for s in range(1, KB + 1)})


# ---- exactly summable operands ------------------------------------------------------------------------------------------------------
E0 = {False: -13, True: -14}       # exponents e0 .. e0 + 11: every non-zero |W| >= 2^-14 is a normal fp16 number
_EXACT = {}


def _exact(K, N, gated):
    """(q, s, z, W float64, x int64 [130][K], expected fp16 [130][N or N / 2]); sums are exact: sum |x| |W| / 2^e0 <= 2^23"""
    key = (K, N, gated)
    if key not in _EXACT:
        rng = np.random.default_rng(K * 31 + N + 7 * gated)
        ng = K // G
        q = rng.integers(0, 16, (K, N)).astype(np.uint8)
        z = rng.integers(0, 16, (ng, N)).astype(np.uint8)
        for g in range(1, ng):                                  # zeros that differ between adjacent groups of a column
            same = z[g] == z[g - 1]
            z[g, same] = (z[g, same] + 1 + rng.integers(0, 14, int(same.sum()))) % 16
        assert ng <= 12
        e = E0[gated] + (np.arange(ng)[:, None] + rng.integers(0, 12, N)[None, :]) % 12        # distinct in every group of a column
        wint = q.astype(np.int64) - np.repeat(z, G, axis=0).astype(np.int64)
        W = wint.astype(f64) * np.exp2(np.repeat(e, G, axis=0).astype(f64))
        nz = np.abs(W[W != 0])
        assert nz.min() >= 2.0**-14
        s = np.exp2(e.astype(f64)).astype(f16)
        assert np.array_equal(o.w4a16_dequant(q, s, z.astype(f16), G).astype(f64), W)     # the on-chip form is exact on these operands
        x = rng.integers(-3, 4, (max(MS), K)).astype(np.int64)
        load = (np.abs(x).astype(f64) @ np.abs(W)) / 2.0**E0[gated]
        assert load.max() <= 2.0**23, load.max()
        acc = x.astype(f64) @ W
        assert np.array_equal(acc.astype(f32).astype(f64), acc)
        with np.errstate(over='raise'):
            want = o.gated_silu_epilogue(acc.astype(f32)) if gated else acc.astype(f16)
        assert np.isfinite(want).all()
        _EXACT[key] = (q, s, z, W, x, want)
    return _EXACT[key]


def _ulp(a, b):
    def key(v):
        i = np.ascontiguousarray(v, f16).view(np.int16).astype(np.int32)
        return np.where(i < 0, -(i & 0x7FFF), i)
    return np.abs(key(a) - key(b))


def test_image_dequantises_bit_for_bit(tm, cuda):
    """random (q, s, z) with every code and zero value present; the read-back covers every unit of a 3 k-block x 5 column-unit image"""
    rng = np.random.default_rng(5)
    K, N = 384, 160
    q = rng.integers(0, 16, (K, N)).astype(np.uint8)
    s = (rng.random((K // G, N)) * 0.02 + 1e-3).astype(f16)
    z = rng.integers(0, 16, (K // G, N)).astype(f16)
    lin = _Linear(tm, q, s, z)
    try:
        got = lin.dequant()
    finally:
        lin.close()
    want = o.w4a16_dequant(q, s, z, G)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    q2, s2, z2, W, _, _ = _exact(384, 96, False)
    lin = _Linear(tm, q2, s2, z2)
    try:
        assert np.array_equal(lin.dequant().astype(f64), W)
    finally:
        lin.close()


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('K', KS)
def test_exact_linear(tm, cuda, K, N):
    q, s, z, _, x, want = _exact(K, N, False)
    lin = _Linear(tm, q, s, z)
    try:
        for M in MS:
            for sp in _splits(K):
                got = lin(x[:M].astype(f16), splits=sp)
                assert np.array_equal(got.view(np.uint16), want[:M].view(np.uint16)), f'K {K} N {N} M {M} splits {sp}'
    finally:
        lin.close()


@pytest.mark.parametrize('N', GATED_NS)
@pytest.mark.parametrize('K', KS)
def test_exact_linear_gated(tm, cuda, K, N):
    q, s, z, _, x, want = _exact(K, N, True)
    lin = _Linear(tm, q, s, z)
    worst = 0
    try:
        first = {}
        for M in MS:
            for sp in _splits(K):
                got = lin(x[:M].astype(f16), gated=True, splits=sp)
                assert np.isfinite(got).all()
                worst = max(worst, int(_ulp(got, want[:M]).max()))
                # exact accumulators: the split launches (reduce kernel) and the unsplit one (GEMM epilogue) agree bit for bit
                assert np.array_equal(got.view(np.uint16), first.setdefault(M, got).view(np.uint16)), f'K {K} N {N} M {M} splits {sp}'
    finally:
        lin.close()
    print(f'u4 g32 gated {K} x {N}: worst ulp {worst}')
    assert worst <= 1


# ---- random operands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,gated', [(384, 160, 0), (1024, 512, 0), (384, 192, 1), (1024, 512, 1)])
def test_random_linear(tm, cuda, K, N, gated):
    rng = np.random.default_rng(K + N + gated)
    w = (rng.standard_normal((K, N)) * (0.1 / np.sqrt(K))).astype(f16)
    q, s, z, _ = o.quantize_groupwise_u4(w, G)
    lin = _Linear(tm, q, s, z)
    try:
        for M in (1, 17, 64, 65, 130, 300):
            x = rng.standard_normal((M, K)).astype(f16)
            ref = (o.w4a16_linear_gated_silu(x, q, s, z, G) if gated else
                   x.astype(f32) @ o.w4a16_dequant(q, s, z, G).astype(f32)).astype(f32)
            for sp in (0, 1, 3):
                err = np.abs(lin(x, gated=bool(gated), splits=sp).astype(f32) - ref)
                tol = 2e-3 + (2.0**-9 if gated else 2.0**-10) * np.abs(ref)
                assert np.all(err <= tol), f'M {M} splits {sp}: max err {err.max()} (ref max {np.abs(ref).max()})'
    finally:
        lin.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(tm, cuda):
    h = _ffi.C.c_void_p()
    rc = tm.tm_linear_create(_ffi.C.byref(h), 128, 32, 0, 64)
    assert rc != 0 and 'group_size 64' in tm.tm_last_error().decode()
    rc = tm.tm_linear_create(_ffi.C.byref(h), 128, 48, 0, 32)
    assert rc != 0 and 'N % 32' in tm.tm_last_error().decode()
    # a mixture-of-experts engine with group 32
    from lmdeploy_amd.turbomind.engine import Engine
    cfg = o.ModelConfig(hidden=256, layers=1, q_heads=2, kv_heads=1, head_dim=128, inter=128, vocab=512, group=32, moe_experts=4, moe_top_k=2)
    with pytest.raises(_ffi.TmError, match='group_size 32 with moe_experts'):
        Engine.from_model_config(cfg, max_batch_size=2, session_len=128)
    cfg = o.ModelConfig(hidden=256, layers=1, q_heads=2, kv_heads=1, head_dim=128, inter=128, vocab=512, group=64)
    with pytest.raises(_ffi.TmError, match='group_size 64'):
        Engine.from_model_config(cfg, max_batch_size=2, session_len=128)
    # the kernel picks its own tile: an explicit nt is refused by name
    q, s, z, _, _, _ = _exact(128, 32, False)
    lin = _Linear(tm, q, s, z)
    try:
        buf = torch.zeros(4096, dtype=torch.float16, device='cuda')
        rc = tm.tm_linear_forward(lin.h, buf.data_ptr(), 128, buf.data_ptr(), 32, 1, 0, 2, 0, 0, None, st())
        assert rc != 0 and 'group-32' in tm.tm_last_error().decode()
    finally:
        lin.close()
