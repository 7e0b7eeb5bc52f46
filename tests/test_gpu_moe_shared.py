"""The MoE block with a shared expert behind a sigmoid gate (Qwen2-MoE) through the C-ABI: tm_moe_set_shared_gate /
tm_moe_forward_shared against a gate-less twin of the same block (tm_moe_forward) and against tests.qwen2_moe_reference.

Per block: x [70][H] with row 0 = +1 and row 1 = -1 on every channel and N(0, 1) elsewhere, a gate vector 0.5 + N(0, 0.05) -- so
the logit of row 0 is about +H / 2 (sigma = 1) and that of row 1 about -H / 2, past expf's range: sigma = 1 / (1 + inf) = 0 --
and a random fp16 `shared` ~ N(0, 2).  T = 1, 3, 64, 70 are the first T rows (every operator is row-wise; the reference is computed
once for the 70 rows).
  (a) on the row with sigma = 0 the gated block's output equals the twin's bit for bit;
  (b) everywhere |out1 - (shared sigma64 + out0)| <= 2^-10 (|out0| + |shared sigma64 + out0|) + |shared| / 4 * H 2^-24 sum_h |x_h g_h|
      + 2^-20: the two fp16 roundings (out0's and out1's, 2^-11 each, doubled to cover the fp32 chain), the worst-case error of an fp32
      summation of H products (H 2^-24 sum |x g|) carried through sigma' <= 1 / 4, and a floor for subnormal outputs;
  (c) three launches in a row and the in-place call (out == shared) give identical bits;
  (d) the call captured in a graph and replayed three times equals the eager result;
  (e) tm_moe_forward on the gated block returns an error;
and the whole block is within the MoE tests' bound 4e-3 + 2^-6 |ref| of the reference module."""
import math

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from tests.gpu_helpers import dev, host, release_all, st
from tests.qwen2_moe_reference import Qwen2MoeConfig, routed_f32, shared_combine, sigma64
from tests.test_gpu_geometry import _fp8_expert, _u4_expert

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
TMAX, TS = 70, (1, 3, 64, 70)


class _Blocks:
    """a block with a shared gate and its gate-less twin (same router, same experts), the inputs and the reference for 70 rows"""

    def __init__(self, tm, H, I, E, k, fmt, seed):
        self.tm, self.H, self.k = tm, H, k
        rng = np.random.default_rng(seed)
        self.x = rng.standard_normal((TMAX, H)).astype(f16)
        self.x[0], self.x[1] = 1.0, -1.0
        self.g = (0.5 + 0.05 * rng.standard_normal(H)).astype(f16)
        self.shared = (2.0 * rng.standard_normal((TMAX, H))).astype(f16)
        assert np.abs(self.shared.astype(f32)).max() >= 4
        router = (0.2 * rng.standard_normal((H, E))).astype(f16)
        self.plain, self.gated = _ffi.C.c_void_p(), _ffi.C.c_void_p()
        for h in (self.plain, self.gated):
            _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E, k, 2 if fmt == 'fp8' else 0, 0, 1.0))      # norm_topk 0
            _ffi.check(tm.tm_moe_set_gate(h, dev(router).data_ptr(), st()))
        _ffi.check(tm.tm_moe_set_shared_gate(self.gated, dev(self.g).data_ptr(), st()))
        Lw = dict(moe_gate=router, experts=[], _dense=[])
        for e in range(E):
            if fmt == 'fp8':
                q13, s13 = _fp8_expert(rng, H, 2 * I, 1.5 / math.sqrt(H))
                q2, s2 = _fp8_expert(rng, I, H, 0.02 / math.sqrt(I))
                args = (dev(q13).data_ptr(), dev(s13).data_ptr(), None, dev(q2).data_ptr(), dev(s2).data_ptr(), None)
                Lw['experts'].append(dict(w1w3=dict(f8=q13, bs=s13), w2=dict(f8=q2, bs=s2)))
            else:
                p13, s13, z13, w13, _ = _u4_expert(rng, H, 2 * I, 1.5 / math.sqrt(H))
                p2, s2, z2, w2, _ = _u4_expert(rng, I, H, 1.0 / math.sqrt(I))
                args = (dev(p13).data_ptr(), dev(s13).data_ptr(), dev(z13).data_ptr(), dev(p2).data_ptr(), dev(s2).data_ptr(),
                        dev(z2).data_ptr())
                Lw['_dense'].append((w13, w2))
            for h in (self.plain, self.gated):
                _ffi.check(tm.tm_moe_set_expert(h, e, *args, st()))
        release_all()
        cfg = Qwen2MoeConfig(hidden=H, layers=1, q_heads=1, kv_heads=1, head_dim=128, inter=I, vocab=8, weight_format=fmt,
                             moe_fp8_act=fmt == 'fp8', moe_experts=E, moe_top_k=k, moe_norm_topk=False)
        self.sigma = sigma64(self.x, self.g)
        self.ref = shared_combine(self.shared, self.x, self.g, routed_f32(self.x, Lw, cfg)).astype(f32)
        # the worst-case fp32 summation error of the logit through sigma' <= 1 / 4, per row
        self.dsig = 0.25 * H * 2.0**-24 * (np.abs(self.x.astype(f64)) * np.abs(self.g.astype(f64))).sum(1)

    def bufs(self, T):
        ws = torch.full((self.tm.tm_moe_workspace(self.gated, T),), 0xFF, dtype=torch.uint8, device='cuda')   # NaN where unwritten
        out = torch.zeros((T, self.H), dtype=torch.float16, device='cuda')
        return ws, out

    def close(self):
        self.tm.tm_moe_destroy(self.plain)
        self.tm.tm_moe_destroy(self.gated)


@pytest.mark.parametrize('H,I,E,k,fmt', [(256, 128, 12, 4, 'u4'), (2304, 128, 4, 2, 'u4'), (256, 128, 12, 4, 'fp8')])
def test_shared_gate_block(tm, cuda, H, I, E, k, fmt):
    """(2304: two workgroups per token in the combine)"""
    b = _Blocks(tm, H, I, E, k, fmt, seed=H + E)
    try:
        assert b.sigma[0] == 1.0 and b.sigma[1] < 1e-40
        for T in TS:
            xd, sh = dev(b.x[:T]), dev(b.shared[:T])
            ws, out = b.bufs(T)
            what = f'{fmt} H {H} E {E} k {k} T {T}'
            # (e) the plain entry point refuses the gated block
            assert tm.tm_moe_forward(b.gated, out.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), None, None, st()) != 0, what
            assert 'shared' in _ffi.last_error()
            _ffi.check(tm.tm_moe_forward(b.plain, out.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), None, None, st()))
            out0_h = host(out).copy()
            out0 = out0_h.astype(f64)

            def run(dst, src):
                _ffi.check(tm.tm_moe_forward_shared(b.gated, dst.data_ptr(), xd.data_ptr(), src.data_ptr(), T, ws.data_ptr(), None,
                                                    None, st()))
            # (c) three launches, then in place
            got = []
            for _ in range(3):
                out.zero_()
                ws.fill_(0xFF)
                run(out, sh)
                got.append(host(out).copy())
            inplace = sh.clone()
            run(inplace, inplace)
            got.append(host(inplace).copy())
            for i in range(1, 4):
                assert np.array_equal(got[i].view(np.uint16), got[0].view(np.uint16)), f'{what}: launch {i} (3 = in place) differs'
            assert np.array_equal(host(sh), b.shared[:T]), f'{what}: the shared input was written'
            out1 = got[0].astype(f64)
            assert np.isfinite(out1).all(), what
            # (a) sigma = 0: the routed sum alone, bit for bit
            if T >= 2:
                assert np.array_equal(got[0][1].view(np.uint16), out0_h[1].view(np.uint16)), f'{what}: sigma = 0 row'
            # (b) against the twin
            shf = b.shared[:T].astype(f64)
            want = shf * b.sigma[:T, None] + out0
            tol = 2.0**-10 * (np.abs(out0) + np.abs(want)) + np.abs(shf) * b.dsig[:T, None] + 2.0**-20
            err = np.abs(out1 - want)
            print(f'{what}: against the twin, worst err / bound {(err / tol).max():.3f}')
            assert np.all(err <= tol), f'{what}: err {err.max()} at {np.unravel_index(np.argmax(err - tol), err.shape)}'
            # the whole block against the reference module
            ref = b.ref[:T]
            tol = 4e-3 + 2.0**-6 * np.abs(ref)
            err = np.abs(out1 - ref)
            print(f'{what}: against the reference, |ref| max {np.abs(ref).max():.3f}, worst err / tol {(err / tol).max():.3f}')
            assert np.all(err <= tol), f'{what}: err {err.max()} at {np.unravel_index(np.argmax(err - tol), err.shape)}'
            # (d) captured and replayed
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(out, sh)
            for i in range(3):
                out.zero_()
                ws.fill_(0xFF)
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(host(out).view(np.uint16), got[0].view(np.uint16)), f'{what}: replay {i}'
            release_all()
    finally:
        b.close()


def test_shared_gate_arguments(tm, cuda):
    """tm_moe_forward_shared needs the gate and the shared output; x must not be the output"""
    b = _Blocks(tm, 256, 128, 4, 2, 'u4', seed=1)
    try:
        T = 3
        xd, sh = dev(b.x[:T]), dev(b.shared[:T])
        ws, out = b.bufs(T)
        args = (T, ws.data_ptr(), None, None, st())
        assert tm.tm_moe_forward_shared(b.plain, out.data_ptr(), xd.data_ptr(), sh.data_ptr(), *args) != 0      # no gate set
        assert tm.tm_moe_forward_shared(b.gated, out.data_ptr(), xd.data_ptr(), None, *args) != 0
        assert tm.tm_moe_forward_shared(b.gated, xd.data_ptr(), xd.data_ptr(), sh.data_ptr(), *args) != 0
        assert tm.tm_moe_forward_stages(b.gated, out.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), 31, st()) != 0
        # the stage form: a whole forward, then the combine alone on what it left gives the same bits
        _ffi.check(tm.tm_moe_forward_shared(b.gated, out.data_ptr(), xd.data_ptr(), sh.data_ptr(), *args))
        whole = host(out).copy()
        out.zero_()
        _ffi.check(tm.tm_moe_forward_shared_stages(b.gated, out.data_ptr(), xd.data_ptr(), sh.data_ptr(), T, ws.data_ptr(), None, None, 16,
                                                   st()))
        assert np.array_equal(host(out).view(np.uint16), whole.view(np.uint16))
        release_all()
    finally:
        b.close()
