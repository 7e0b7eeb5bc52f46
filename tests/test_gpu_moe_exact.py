"""The mixture-of-experts path against exactly summable blocks (tests/moe_exact_reference.py; proved on the CPU by
tests/test_host_moe_exact.py): the router's logits are integers and its picks tie, so the routing weights are exactly
routed_scale / k; the gate accumulators are powers of two in [32, 256], where a / (1 + expf(-a)) is a itself; every partial sum of
both grouped GEMMs and of the combine is representable in fp32.  Every row tile, segment layout, router and order of summation
must return the same bits -- h(sum_j h(h(gate * up) . W2) * routed_scale / k [+ shared * sigma]) -- and the kernels are held to
them.  A mismatch is a wrong, missing or duplicated term, a foreign row or expert, an fp16 intermediate, a pair the combine lost
or took twice, or a race; never an accumulation-order effect.

Blocks: (H 256, I 384) and (H 384, I 128: w2's 24 column tiles leave the last workgroup of the 8-wave decode grid and of the
16-tile prefill grid half empty) x (experts, top_k, routed_scale) = (8, 2, 1.0) on the serial router and again on the wide one,
(8, 1, 2.0), (72, 8, 1.0), (128, 4, 0.5) x u4, fp16 and e4m3 weight-only experts (TM_FP8_MFMA=0 before the block's first forward).
Forwards: T = 1, 37, 64, 65, 300 x routings random / one (an expert takes every token, most are empty) / edge (an expert with
exactly 2 * hint rows and one with 2 * hint + 1; not at T = 1); T <= 64 on every forced row tile (0 = the launcher's rule, 16, 32,
64), T > 64 on the prefill tile.  The workspace is filled with 0xFF once per block and never cleared, the output is pre-filled
with an fp16 NaN pattern, every forward runs twice.  ids equal the oracle's in order, topk_w equal routed_scale / k as uint32,
every output element equals the expectation as uint16 with -0 mapped to +0; no ulp allowance anywhere.

Also: tm_moe_forward_shared on the (8, 2) block with tokens of sigma = 1 and of sigma = 0 (logit 32 / -128), `shared` in its own
buffer and in place; the router alone on logits whose k-th and (k+1)-th entries tie (E = 8 .. 256, k = 1 .. 8, both routers where
both apply: logits, ids and the three tables); tm_moe_forward_stages 1|2 then 4|8|16 against the same expectation.

Out of scope: e4m3 experts on the matrix cores (they re-quantise act per row with absmax / 448, not a power of two for these
values) and per-pick weight mix-ups (invisible when the picks tie; norm_topk = 0 and untied softmax weights go through expf and
cannot be exact) stay on the tolerance tests of test_gpu_geometry.py / test_gpu_moe_wide.py / test_gpu_moe_f16.py.

Comparisons (case x launch): blocks 30 x 76 = 2280 (T = 1: 2 routings x 4 tiles, T = 37 / 64: 3 x 4, T = 65 / 300: 3 x 1, twice
each), shared expert 6 x 16 = 96, stage split 3 x 4 = 12, router 30 (E, k, router) cases; one
negative control (a u4 code off by one must be noticed).
Configurations this module caught: none so far."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import moe_exact_reference as r
from tests.gpu_helpers import dev, host, release_all, st
from tests.test_gpu_moe_wide import _Router, _tables

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
AUTO, WIDE = 0, 1
WTYPE = {'u4': 0, 'f16': 1, 'fp8': 2}
SENT = 0x7DAD                                                   # an fp16 NaN pattern no kernel writes
TMAX = max(r.TOKENS)
CONFIGS = [(8, 2, 1.0, AUTO), (8, 2, 1.0, WIDE), (8, 1, 2.0, AUTO), (72, 8, 1.0, AUTO), (128, 4, 0.5, AUTO)]
CONFIG_IDS = ['E8-k2-serial', 'E8-k2-wide', 'E8-k1', 'E72-k8', 'E128-k4']
GEOMETRY_IDS = [f'H{H}-I{I}' for H, I in r.GEOMETRIES]

_CASES = {}


def _case(B, fam, T, routing, shared=False):
    """(x fp16, the reference's result, shared fp16 or None), computed once and shared by every format of the family and both routers"""
    key = (B.H, B.I, B.E, B.k, B.scale, fam, T, routing, shared)
    if key not in _CASES:
        x, ids = r.make_x(B, T, routing)
        sh = r.make_shared(B, T) if shared else None
        x16 = x.astype(f16)
        assert np.array_equal(x16.astype(np.int64), x)
        _CASES[key] = (x16, r.forward(B, fam, x, ids, shared=sh), sh)
    return _CASES[key]


def _bits_d(t):
    """int16 view on the device with -0 mapped to +0"""
    v = t.view(torch.int16)
    return torch.where(v == -32768, torch.zeros_like(v), v)


class _Moe:
    """one block on the device; one workspace, 0xFF once, never cleared"""

    def __init__(self, tm, monkeypatch, B, fmt, router=AUTO, shared=False, operands=None):
        self.tm, self.B, self.fmt, self.router, self.fam = tm, B, fmt, router, r.family(fmt)
        self.h = _ffi.C.c_void_p()
        _ffi.check(tm.tm_moe_create(_ffi.C.byref(self.h), B.H, B.I, B.E, B.k, WTYPE[fmt], 1, B.scale))
        try:
            _ffi.check(tm.tm_moe_set_gate(self.h, dev(B.gate()).data_ptr(), st()))
            if shared:
                _ffi.check(tm.tm_moe_set_shared_gate(self.h, dev(B.shared_gate()).data_ptr(), st()))
            for e in range(B.E):
                ops = [None if a is None else dev(a).data_ptr() for a in (operands or {}).get(e) or B.expert(e).operands(fmt)]
                _ffi.check(tm.tm_moe_set_expert(self.h, e, *ops, st()))
                if e % 16 == 15:
                    release_all()
            release_all()
            if fmt == 'fp8':
                monkeypatch.setenv('TM_FP8_MFMA', '0')          # weight-only: the path is chosen at the block's first forward
            self.ws = torch.full((tm.tm_moe_workspace(self.h, TMAX),), 0xFF, dtype=torch.uint8, device='cuda')
        except BaseException:
            tm.tm_moe_destroy(self.h)
            raise
        self.compared = 0

    def close(self):
        self.tm.tm_moe_destroy(self.h)
        release_all()

    def launch(self, call, rows):
        _ffi.check(self.tm.tm_debug_set_moe_router(self.router))
        _ffi.check(self.tm.tm_debug_set_grouped_rows(rows))
        try:
            call()
            torch.cuda.synchronize()
        finally:
            self.tm.tm_debug_set_grouped_rows(0)
            self.tm.tm_debug_set_moe_router(-1)

    def tile(self, T, rows):
        """the row tile launch_linear_grouped takes (no measured entry in a test process)"""
        if T > 64:
            return 64
        if rows:
            return rows
        want = min(T, max(1, 2 * self.B.hint(T)))
        return 16 if want <= 16 else 32 if want <= 32 else 64

    def verify(self, what, T, rows, res, out, ids=None, w=None):
        B = self.B
        if ids is not None:
            got_ids = host(ids)
            assert np.array_equal(got_ids, res.ids), f'{what}: ids differ, first at token {np.argwhere(got_ids != res.ids)[0][0]}'
            assert np.array_equal(host(w).view(np.uint32), res.w.view(np.uint32)), f'{what}: topk_w is not routed_scale / k = {B.w}'
        want_d = dev(r.bits(res.out).view(np.int16))
        bad = _bits_d(out) != want_d
        if bool(bad.any()):
            got = host(out)
            t, c = bad.nonzero()[0].tolist()
            tile = self.tile(T, rows)
            flat = res.en2f[:, t]
            where = ', '.join(f'expert {e} flat row {f} = row {f - res.offsets[e]} of {res.offsets[e + 1] - res.offsets[e]} '
                              f'(row block {(f - res.offsets[e]) // tile} of {tile})' for e, f in zip(res.ids[t].tolist(), flat.tolist()))
            pytest.fail(f'{what}: {int(bad.sum())} outputs on {int(bad.any(1).sum())} tokens differ, first at token {t} column {c} '
                        f'(column tile {c // 16}): got {float(got[t, c])!r} ({got.view(np.uint16)[t, c]:#06x}) want '
                        f'{float(res.out[t, c])!r} ({res.out.view(np.uint16)[t, c]:#06x}); {where}')
        self.compared += 1

    def forward(self, T, routing, rows, launches=2):
        x16, res, _ = _case(self.B, self.fam, T, routing)
        B = self.B
        xd = dev(x16)
        for rep in range(launches):
            out = torch.full((T, B.H), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
            ids = torch.full((T, B.k), -1, dtype=torch.int32, device='cuda')
            w = torch.full((T, B.k), float('nan'), dtype=torch.float32, device='cuda')
            self.launch(lambda: _ffi.check(self.tm.tm_moe_forward(self.h, out.data_ptr(), xd.data_ptr(), T, self.ws.data_ptr(), ids.data_ptr(),
                                                                  w.data_ptr(), st())), rows)
            what = (f'{self.fmt} H {B.H} I {B.I} E {B.E} k {B.k} {"wide" if self.router == WIDE or B.E > 64 else "serial"} router, '
                    f'{routing} T {T} rows {rows or "auto"} launch {rep}')
            self.verify(what, T, rows, res, out, ids, w)
        release_all()


@pytest.mark.parametrize('fmt', ['u4', 'f16', 'fp8'])
@pytest.mark.parametrize('E,k,scale,router', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('H,I', r.GEOMETRIES, ids=GEOMETRY_IDS)
def test_moe_forward(tm, cuda, monkeypatch, H, I, E, k, scale, router, fmt):
    """tm_moe_forward: every T, routing and row tile of the module docstring, twice each on the never-cleared workspace"""
    B = r.Block(H, I, E, k, scale)
    m = _Moe(tm, monkeypatch, B, fmt, router)
    try:
        for T in r.TOKENS:
            for routing in r.ROUTINGS:
                if not B.feasible(T, routing):
                    continue
                for rows in ((0, 16, 32, 64) if T <= 64 else (0,)):
                    m.forward(T, routing, rows)
        print(f'{fmt} H {H} I {I} E {E} k {k}: {m.compared} comparisons')
        assert m.compared == 76
    finally:
        m.close()


@pytest.mark.parametrize('fmt', ['u4', 'f16', 'fp8'])
@pytest.mark.parametrize('H,I', r.GEOMETRIES, ids=GEOMETRY_IDS)
def test_moe_forward_shared(tm, cuda, monkeypatch, H, I, fmt):
    """tm_moe_forward_shared on the (8, 2) block: tokens with sigma = 1 and with sigma = 0 in every forward, `shared` in a buffer of
    its own and `shared == out` (the in-place form), T = 37 on the 16- and 64-row tiles and T = 300 on the prefill tile"""
    E, k, scale, _ = CONFIGS[0]
    B = r.Block(H, I, E, k, scale)
    m = _Moe(tm, monkeypatch, B, fmt, AUTO, shared=True)
    try:
        for T, rows in ((37, 16), (37, 64), (64, 0), (300, 0)):
            x16, res, sh = _case(B, m.fam, T, 'random', shared=True)
            sig = r.sigma_of(x16.astype(np.int64))
            assert 0 < sig.sum() < T
            xd, shd = dev(x16), dev(sh)
            for in_place in (False, True):
                for rep in range(2):
                    out = shd.clone() if in_place else torch.full((T, H), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
                    src = out if in_place else shd
                    ids = torch.full((T, k), -1, dtype=torch.int32, device='cuda')
                    w = torch.full((T, k), float('nan'), dtype=torch.float32, device='cuda')
                    m.launch(lambda: _ffi.check(tm.tm_moe_forward_shared(m.h, out.data_ptr(), xd.data_ptr(), src.data_ptr(), T, m.ws.data_ptr(),
                                                                         ids.data_ptr(), w.data_ptr(), st())), rows)
                    m.verify(f'{fmt} H {H} I {I} shared {"in place" if in_place else "separate"} T {T} rows {rows or "auto"} launch {rep}',
                             T, rows, res, out, ids, w)
        assert m.compared == 16
    finally:
        m.close()


@pytest.mark.parametrize('fmt', ['u4', 'f16', 'fp8'])
def test_moe_forward_stages(tm, cuda, monkeypatch, fmt):
    """tm_moe_forward_stages with the router's stages (1 | 2) and then the experts' and the combine's (4 | 8 | 16) on one workspace:
    the expectation's bits, which are the whole forward's"""
    H, I = r.GEOMETRIES[0]
    E, k, scale, _ = CONFIGS[3]
    B = r.Block(H, I, E, k, scale)
    m = _Moe(tm, monkeypatch, B, fmt)
    try:
        for T in (37, 300):
            x16, res, _ = _case(B, m.fam, T, 'edge')
            xd = dev(x16)
            for rep in range(2):
                out = torch.full((T, H), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
                for stages in (1 | 2, 4 | 8 | 16):
                    m.launch(lambda: _ffi.check(tm.tm_moe_forward_stages(m.h, out.data_ptr(), xd.data_ptr(), T, m.ws.data_ptr(), stages, st())), 0)
                m.verify(f'{fmt} stages 3 then 28, T {T} launch {rep}', T, 0, res, out)
        assert m.compared == 4
    finally:
        m.close()


def test_one_code_off_by_one_is_noticed(tm, cuda, monkeypatch):
    """the comparison is sharp on the device too: expert 3 (it takes every token) is uploaded with ONE u4 code of w2 off by one.
    Column n of the output then differs from the expectation on some token, and every other column still equals it"""
    H, I = r.GEOMETRIES[0]
    E, k, scale, _ = CONFIGS[0]
    B = r.Block(H, I, E, k, scale)
    ex = B.expert(3)
    kk, n = 200, 77
    q2 = ex.b.q.copy()
    q2[kk, n] += 1 if q2[kk, n] < 15 else -1
    ops = list(ex.operands('u4'))
    ops[3] = o.pack_u4_row(q2)
    m = _Moe(tm, monkeypatch, B, 'u4', operands={3: ops})
    try:
        T = 37
        x16, res, _ = _case(B, 'w', T, 'one')
        assert (res.ids == 3).any(axis=1).all() and (res.act[res.offsets[3]:res.offsets[4], kk] != 0).any()
        out = torch.full((T, H), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        m.launch(lambda: _ffi.check(tm.tm_moe_forward(m.h, out.data_ptr(), dev(x16).data_ptr(), T, m.ws.data_ptr(), None, None, st())), 0)
        bad = r.bits(host(out)) != r.bits(res.out)
        assert bad[:, n].any(), 'a u4 code off by one went unnoticed'
        assert not np.delete(bad, n, axis=1).any()
    finally:
        m.close()


@pytest.mark.parametrize('E', [8, 64, 65, 72, 128, 256])
def test_router_ties_go_to_the_lower_id(tm, cuda, E):
    """tm_moe_router alone on the boundary pattern (the k-th and (k+1)-th logits tie; above 64 experts also inside one lane of
    the wide kernel across its 64-expert strides, and with the lower id in the higher lane): the logits are the integers, the ids
    o.moe_gate's, the tables the contract's; the serial and the wide router where both apply"""
    H, T = 384, 97
    gate = np.zeros((H, E), f16)
    gate[:E] = np.eye(E, dtype=f16)
    for k in (1, 2, 4, 8):
        if k >= E:
            continue
        x, ids = r.boundary_x(E, k, T, H)
        x16 = x.astype(f16)
        lg, oids, ow = o.moe_gate(x16, gate, k, True, 1.0)
        assert np.array_equal(oids, ids)
        rt = _Router(tm, gate, k, True, 1.0)
        try:
            for mode in ((AUTO, WIDE) if E <= 64 else (AUTO,)):
                got = rt(x16, mode)
                what = f'E {E} k {k} {"wide" if mode == WIDE or E > 64 else "serial"} router'
                assert np.array_equal(got['logits'].view(np.uint32), x[:, :E].astype(f32).view(np.uint32)), f'{what}: logits'
                bad = np.flatnonzero(np.any(got['ids'] != ids, axis=1))
                assert bad.size == 0, (f'{what}: ids differ on {bad.size} tokens, first token {bad[0]} (form {bad[0] % 4}): got '
                                       f'{got["ids"][bad[0]].tolist()} want {ids[bad[0]].tolist()}, tied experts '
                                       f'{np.flatnonzero(x[bad[0], :E] == x[bad[0], ids[bad[0], -1]]).tolist()}')
                assert np.abs(got['w'] - ow).max() <= 1e-5, what
                offsets, f2n, en2f = _tables(ids, E)
                assert np.array_equal(got['offsets'], offsets), f'{what}: offsets'
                assert np.array_equal(got['f2n'], f2n), f'{what}: f2n'
                assert np.array_equal(got['en2f'], en2f), f'{what}: en2f'
        finally:
            rt.close()
            release_all()
