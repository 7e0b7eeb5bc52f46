"""The wide MoE router (65 .. 256 experts, and every expert count with TM_MOE_ROUTER=wide) through the C-ABI: against the serial
router on the same inputs, against oracle.moe_gate and a numpy restatement of the routing tables, and the whole block
(tm_moe_forward) against oracle.moe_ffn / moe_ffn_fp8 at Qwen3-MoE's sizes, on skewed routings and under graph capture."""
import math

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.gpu_helpers import dev, host, release_all, st
from tests.test_gpu_geometry import _expert_ffn, _fp8_expert, _fp8_wo_dense, _u4_expert

gpu = pytest.mark.gpu
f16, f32 = np.float16, np.float32
AUTO, WIDE = 0, 1


class _Router:
    """a tm_moe with only its gate set: tm_moe_router needs no experts"""

    def __init__(self, tm, gate, k, norm_topk=True, scale=1.0, mode=AUTO):
        self.tm, self.k, self.mode = tm, k, mode
        self.H, self.E = gate.shape
        self.h = _ffi.C.c_void_p()
        _ffi.check(tm.tm_moe_create(_ffi.C.byref(self.h), self.H, 128, self.E, k, 0, int(norm_topk), scale))
        _ffi.check(tm.tm_moe_set_gate(self.h, dev(gate).data_ptr(), st()))

    def __call__(self, x, mode=None):
        T, E, k = len(x), self.E, self.k

        def buf(n, dt):      # 0xFF everywhere: an unwritten int is -1, an unwritten float a NaN
            return torch.full((n * 4,), 0xFF, dtype=torch.uint8, device='cuda').view(dt)
        ids, f2n, en2f, offs = buf(T * k, torch.int32), buf(T * k, torch.int32), buf(T * k, torch.int32), buf(E + 1, torch.int32)
        w, lg = buf(T * k, torch.float32), buf(T * E, torch.float32)
        _ffi.check(self.tm.tm_debug_set_moe_router(self.mode if mode is None else mode))
        try:
            _ffi.check(self.tm.tm_moe_router(self.h, dev(x).data_ptr(), T, ids.data_ptr(), w.data_ptr(), lg.data_ptr(), offs.data_ptr(),
                                             f2n.data_ptr(), en2f.data_ptr(), st()))
            torch.cuda.synchronize()
        finally:
            self.tm.tm_debug_set_moe_router(-1)
        return dict(ids=host(ids).reshape(T, k), w=host(w).reshape(T, k), offsets=host(offs), f2n=host(f2n),
                    en2f=host(en2f).reshape(k, T), logits=host(lg).reshape(T, E))

    def close(self):
        self.tm.tm_moe_destroy(self.h)


def _tables(ids, E):
    """the contract restated: the flat rows are the (token, choice) pairs sorted by expert, tokens ascending inside an expert
    (a stable sort of the token-major pair list); offsets the expert boundaries, f2n the row's token, en2f[j][t] the row"""
    T, k = ids.shape
    order = np.argsort(ids.ravel(), kind='stable')
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids.ravel(), minlength=E))]).astype(np.int32)
    inv = np.empty(T * k, np.int32)
    inv[order] = np.arange(T * k, dtype=np.int32)
    return offsets, (order // k).astype(np.int32), np.ascontiguousarray(inv.reshape(T, k).T)


def _check_tables(got, ids, E, what):
    offsets, f2n, en2f = _tables(ids, E)
    assert np.array_equal(got['offsets'], offsets), f'{what}: offsets'
    assert np.array_equal(got['f2n'], f2n), f'{what}: f2n'
    assert np.array_equal(got['en2f'], en2f), f'{what}: en2f'


def _separated(rng, T, H, E):
    """gate = identity over the first E channels plus small noise; x[:, :E] a permutation of a ladder per token, spaced min(0.25,
    8 / E) and centred on 0: adjacent logits differ by >= 0.03 less a noise of about 0.001, far above any fp32 reordering (1e-6),
    and |logit| <= 4 as in test_gpu_geometry._moe_x -- the 1e-5 bound on the weights is a bound for logits of that size (the
    fp32 rounding of a logit grows with its magnitude and passes into the weight through the exponential)"""
    assert H > E
    gate = (rng.standard_normal((H, E)) * 0.00005).astype(f16)
    gate[:E] = np.eye(E, dtype=f16)
    x = rng.standard_normal((T, H)).astype(f16)
    step = min(0.25, 8.0 / E)
    ladder = ((np.arange(E) - E / 2) * step).astype(f16)
    assert np.all(np.diff(ladder.astype(f32)) > 0.8 * step)
    x[:, :E] = np.stack([ladder[rng.permutation(E)] for _ in range(T)])
    return gate, x


@gpu
@pytest.mark.parametrize('E', [4, 8, 64])
def test_wide_router_equals_serial_router(tm, cuda, E):
    """TM_MOE_ROUTER=wide against auto on the same inputs (separated logits): ids and tables identical, weights within 1e-5"""
    rng = np.random.default_rng(E)
    for k in (1, 2, 8):
        if k > E:
            continue
        for norm in (True, False):
            for T in (1, 3, 64, 1500):
                gate, x = _separated(rng, T, 256, E)
                r = _Router(tm, gate, k, norm, 1.0)
                try:
                    old, new = r(x, AUTO), r(x, WIDE)
                finally:
                    r.close()
                what = f'E {E} k {k} T {T} norm {norm}'
                _, ids, w = o.moe_gate(x, gate, k, norm)
                assert np.array_equal(old['ids'], ids), what + ': serial router against the oracle'
                assert np.array_equal(new['ids'], old['ids']), what + ': ids'
                for n in ('offsets', 'f2n', 'en2f'):
                    assert np.array_equal(new[n], old[n]), f'{what}: {n}'
                assert np.abs(new['w'] - old['w']).max() <= 1e-5, what
                release_all()


@gpu
@pytest.mark.parametrize('E', [65, 72, 128, 160, 256])
def test_wide_router_separated_logits(tm, cuda, E):
    rng = np.random.default_rng(100 + E)
    for k in (1, 6, 8):
        for norm in (True, False):
            for T in (1, 5, 64, 257, 4096):
                gate, x = _separated(rng, T, 512, E)
                r = _Router(tm, gate, k, norm, 2.5)
                try:
                    got = r(x)
                finally:
                    r.close()
                what = f'E {E} k {k} T {T} norm {norm}'
                lg, ids, w = o.moe_gate(x, gate, k, norm, 2.5)
                assert np.array_equal(got['ids'], ids), f'{what}: ids differ on {np.sum(np.any(got["ids"] != ids, 1))} tokens'
                assert np.abs(got['w'] - w).max() <= 1e-5, what
                assert np.abs(got['logits'] - lg).max() <= 1e-3, what
                _check_tables(got, ids, E, what)
                release_all()


@gpu
@pytest.mark.parametrize('H,E,T', [(2048, 128, 1024), (4096, 128, 512), (2048, 256, 512)])
def test_wide_router_random_logits(tm, cuda, H, E, T):
    """x ~ N(0, 1), gate ~ 0.02 N(0, 1).  A token is decided when every adjacent gap among its k + 1 largest fp64 logits exceeds
    gap = 8 x max(error of the oracle's fp32 logits, error of a strictly sequential fp32 accumulation), both against fp64 and
    both computed here on the CPU.  Decided tokens: ids exact.  Undecided (at most 3 % of the tokens): k distinct experts, none
    below the (k+1)-th largest fp64 logit minus gap, in non-increasing order of the device's own logits."""
    k = 8
    rng = np.random.default_rng(11)
    x = rng.standard_normal((T, H)).astype(f16)
    gate = (0.02 * rng.standard_normal((H, E))).astype(f16)
    l64 = x.astype(np.float64) @ gate.astype(np.float64)
    lg, ids, w = o.moe_gate(x, gate, k, True, 1.0)
    seq = np.zeros((T, E), f32)
    xf, gf = x.astype(f32), gate.astype(f32)
    for h in range(H):
        seq += xf[:, h:h + 1] * gf[h:h + 1]
    gap = 8 * max(np.abs(lg - l64).max(), np.abs(seq - l64).max())
    top = -np.sort(-l64, axis=1)[:, :k + 1]
    decided = np.all(top[:, :-1] - top[:, 1:] > gap, axis=1)
    und = np.nonzero(~decided)[0]
    print(f'H {H} E {E} T {T}: gap {gap:.3e}, undecided {len(und)} of {T}')
    assert len(und) <= 0.03 * T, f'{len(und)} of {T} tokens undecided at gap {gap}'
    r = _Router(tm, gate, k, True, 1.0)
    try:
        got = r(x)
    finally:
        r.close()
    assert np.array_equal(got['ids'][decided], ids[decided]), 'ids of decided tokens'
    assert np.abs(got['w'][decided] - w[decided]).max() <= 1e-5
    for t in und:
        sel = got['ids'][t]
        assert len(set(sel.tolist())) == k and sel.min() >= 0 and sel.max() < E, f'token {t}: {sel}'
        assert np.all(l64[t, sel] >= top[t, k] - gap), f'token {t}: an expert below the (k+1)-th logit'
        dl = got['logits'][t, sel]
        assert np.all(dl[:-1] >= dl[1:]), f'token {t}: ids not in the order of the device logits'
    _check_tables(got, got['ids'], E, 'tables of the device ids')


# ---- the whole block ------------------------------------------------------------------------------------------------------------
def _picked_x(rng, gate_E, T, H, picks):
    """x whose first E channels route token t to picks[t] (in that order): 3.0, 2.875, ... on the picks, U(-1, 0) elsewhere"""
    x = rng.standard_normal((T, H)).astype(f16)
    x[:, :gate_E] = rng.uniform(-1.0, 0.0, (T, gate_E)).astype(f16)
    for t, p in enumerate(picks):
        for j, e in enumerate(p):
            x[t, e] = f16(3.0 - 0.125 * j)
    return x


def _skewed_picks(kind, T, E, k):
    hint = (T * k + E - 1) // E
    picks = [[] for _ in range(T)]
    if kind == 'one':          # expert 3 takes every token; the other choices walk over experts 8 ..
        for t in range(T):
            picks[t] = [3] + [8 + (t * (k - 1) + j) % (E - 8) for j in range(k - 1)]
        return picks, {3: T}
    a = 2 * hint               # 'edge': expert 1 exactly 2 * hint rows, expert 2 exactly 2 * hint + 1
    assert 2 * a + 1 <= 2 * T
    for t in range(a):
        picks[t].append(1)
    for t in range(T - a - 1, T):
        picks[t].append(2)
    i = 0
    for t in range(T):
        while len(picks[t]) < k:
            picks[t].append(8 + i % (E - 8))
            i += 1
    return picks, {1: a, 2: a + 1}


TILES = {'u4': (0, 16, 32, 64), 'fp8wo': (0, 16, 32, 64), 'fp8': (0, 32, 64)}


def _block(tm, monkeypatch, H, I, E, k, wtype, cases, seed, norm_topk=True, scale=1.0):
    """one block per expert format through tm_moe_create / _set_gate / _set_expert / _forward.  Experts are drawn one at a time
    (uploaded, their rows of every case computed by the oracle's expert arithmetic, dropped); the combine is o.moe_ffn's."""
    rng = np.random.default_rng(seed)
    gate = (rng.standard_normal((H, E)) * 0.00005).astype(f16)      # (noise of about 0.003 at H 4096 against steps of 0.125)
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
    kinds = ('fp8', 'fp8wo') if wtype == 'fp8' else ('u4',)
    y = {kd: [np.zeros((len(x), k, H), f32) for x in xs] for kd in kinds}
    handles = {}
    for kd in kinds:
        h = _ffi.C.c_void_p()
        _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E, k, 2 if wtype == 'fp8' else 0, int(norm_topk), scale))
        _ffi.check(tm.tm_moe_set_gate(h, dev(gate).data_ptr(), st()))
        handles[kd] = h
    s13_std, s2_std = (1.5, 0.05 if I > 1024 else 0.02) if wtype == 'fp8' else (1.5, 1.0)

    def add(e, kd, wts):
        for c, (x, (_, ids, _)) in enumerate(zip(xs, routing)):
            t, j = np.nonzero(ids == e)
            if len(t):
                y[kd][c][t, j] = _expert_ffn(kd, wts, x[t]).astype(f32)
    try:
        for e in range(E):
            if wtype == 'fp8':
                q13, s13 = _fp8_expert(rng, H, 2 * I, s13_std / math.sqrt(H))
                q2, s2 = _fp8_expert(rng, I, H, s2_std / math.sqrt(I))
                for kd in kinds:
                    _ffi.check(tm.tm_moe_set_expert(handles[kd], e, dev(q13).data_ptr(), dev(s13).data_ptr(), None, dev(q2).data_ptr(),
                                                    dev(s2).data_ptr(), None, st()))
                add(e, 'fp8', ((q13, s13), (q2, s2)))
                add(e, 'fp8wo', (_fp8_wo_dense(q13, s13, True), _fp8_wo_dense(q2, s2, False)))
            else:
                p13, s13, z13, w13, _ = _u4_expert(rng, H, 2 * I, 1.5 / math.sqrt(H))
                p2, s2, z2, w2, _ = _u4_expert(rng, I, H, 1.0 / math.sqrt(I))
                _ffi.check(tm.tm_moe_set_expert(handles['u4'], e, dev(p13).data_ptr(), dev(s13).data_ptr(), dev(z13).data_ptr(),
                                                dev(p2).data_ptr(), dev(s2).data_ptr(), dev(z2).data_ptr(), st()))
                add(e, 'u4', (w13, w2))
            release_all()
        for kd in kinds:     # fp8 first: the weight-only block takes its path at its first forward
            if kd == 'fp8wo':
                monkeypatch.setenv('TM_FP8_MFMA', '0')
            for c, x in enumerate(xs):
                _, ids, w = routing[c]
                ref = np.zeros((len(x), H), f32)
                for j in range(k):
                    ref += w[:, j:j + 1] * y[kd][c][:, j]
                ref = ref.astype(f16).astype(f32)
                tol = 4e-3 + 2.0**-6 * np.abs(ref)
                assert np.any(np.abs(ref) > tol) and np.any(0.25 * np.abs(ref) > tol), f'{kd} {labels[c]}: outputs too small to test'
                tiles = TILES[kd] if kd == 'fp8' or len(x) <= 64 else (0,)
                for rows in tiles:
                    out, gids, gw = _forward(tm, handles[kd], x, k, rows)
                    what = f'{kd} {labels[c]} rows {rows or "auto"}'
                    assert np.array_equal(gids, ids), f'{what}: routing differs'
                    assert np.abs(gw - w).max() <= 1e-5, what
                    err = np.abs(out - ref)
                    print(f'{what}: |ref| max {np.abs(ref).max():.4f}, worst err / tol {(err / tol).max():.3f}')
                    assert np.all(err <= tol), f'{what}: max err {err.max()} at {np.unravel_index(np.argmax(err - tol), err.shape)}'
    finally:
        for h in handles.values():
            tm.tm_moe_destroy(h)


def _forward(tm, h, x, k, rows=0, ws=None, bufs=None):
    T, H = x.shape
    ws = torch.full((tm.tm_moe_workspace(h, T),), 0xFF, dtype=torch.uint8, device='cuda')   # NaN in every unwritten fp16
    out = torch.zeros((T, H), dtype=torch.float16, device='cuda')
    ids = torch.zeros((T, k), dtype=torch.int32, device='cuda')
    w = torch.zeros((T, k), dtype=torch.float32, device='cuda')
    _ffi.check(tm.tm_debug_set_grouped_rows(rows))
    try:
        _ffi.check(tm.tm_moe_forward(h, out.data_ptr(), dev(x).data_ptr(), T, ws.data_ptr(), ids.data_ptr(), w.data_ptr(), st()))
        torch.cuda.synchronize()
    finally:
        tm.tm_debug_set_grouped_rows(0)
    return host(out).astype(f32), host(ids), host(w)


@gpu
@pytest.mark.parametrize('wtype', ['fp8', 'u4'])
def test_wide_moe_skewed_routing(tm, cuda, monkeypatch, wtype):
    """72 experts, top-8, H 256 / I 256: one expert takes every token (rows far past the launcher's tile), T = 1 (64 experts
    empty), an expert with exactly 2 * hint and one with 2 * hint + 1 rows; every forced row tile; routed_scale 2.5"""
    _block(tm, monkeypatch, 256, 256, 72, 8, wtype,
           [('random', 1), ('random', 37), ('one', 64), ('one', 300), ('edge', 64), ('edge', 300)], seed=7, scale=2.5)


@gpu
@pytest.mark.parametrize('wtype', ['fp8', 'u4'])
def test_wide_moe_hint_range(tm, cuda, monkeypatch, wtype):
    """the decode row tile comes from m_hint = ceil(T k / E): T = 9 .. 64 at 72 experts, top-8 gives m_hint 1 .. 8"""
    cases = [('random', T) for T in (9, 18, 27, 36, 45, 54, 63, 64)]
    assert [(T * 8 + 71) // 72 for _, T in cases] == [1, 2, 3, 4, 5, 6, 7, 8]
    _block(tm, monkeypatch, 256, 128, 72, 8, wtype, cases, seed=9)


@gpu
@pytest.mark.parametrize('wtype', ['fp8', 'u4'])
def test_wide_moe_qwen3_30b_a3b_size(tm, cuda, monkeypatch, wtype):
    """Qwen3-30B-A3B's block: H 2048, I 768 (w2: K = 768, six k-blocks), 128 experts, top-8; e4m3 experts on the matrix cores and
    weight-only, u4 experts; T = 1 / 64 / 200"""
    _block(tm, monkeypatch, 2048, 768, 128, 8, wtype, [('random', 1), ('random', 64), ('random', 200)], seed=30)


@gpu
def test_wide_moe_qwen3_235b_a22b_size(tm, cuda, monkeypatch):
    """Qwen3-235B-A22B's block: H 4096, I 1536, 128 experts, top-8, u4, T = 64"""
    _block(tm, monkeypatch, 4096, 1536, 128, 8, 'u4', [('random', 64)], seed=235)


@gpu
@pytest.mark.parametrize('E', [8, 128])
def test_wide_moe_forward_under_graph_capture(tm, cuda, E):
    """tm_moe_forward captured in a graph (no host synchronisation, allocation or memset inside) and replayed three times equals the
    eager result bit for bit; E = 8 runs the wide router by the switch"""
    H, I, k, T = 256, 128, min(8, E // 2), 48
    rng = np.random.default_rng(E)
    gate = (0.2 * rng.standard_normal((H, E))).astype(f16)
    x = rng.standard_normal((T, H)).astype(f16)
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E, k, 0, 1, 1.0))
    _ffi.check(tm.tm_debug_set_moe_router(WIDE))
    try:
        _ffi.check(tm.tm_moe_set_gate(h, dev(gate).data_ptr(), st()))
        for e in range(E):
            p13, s13, z13, _, _ = _u4_expert(rng, H, 2 * I, 1.5 / math.sqrt(H))
            p2, s2, z2, _, _ = _u4_expert(rng, I, H, 1.0 / math.sqrt(I))
            _ffi.check(tm.tm_moe_set_expert(h, e, dev(p13).data_ptr(), dev(s13).data_ptr(), dev(z13).data_ptr(), dev(p2).data_ptr(),
                                            dev(s2).data_ptr(), dev(z2).data_ptr(), st()))
        xd = dev(x)
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
        for i in range(3):
            out.zero_(), ids.zero_(), w.zero_()
            ws.fill_(0xFF)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(host(out).view(np.uint16), eager[0].view(np.uint16)), f'replay {i}: output'
            assert np.array_equal(host(ids), eager[1]) and np.array_equal(host(w).view(np.uint32), eager[2].view(np.uint32)), f'replay {i}'
    finally:
        tm.tm_debug_set_moe_router(-1)
        tm.tm_moe_destroy(h)


@gpu
def test_expert_count_bounds(tm, cuda):
    h = _ffi.C.c_void_p()
    assert tm.tm_moe_create(_ffi.C.byref(h), 256, 128, 257, 8, 0, 1, 1.0) != 0
    assert tm.tm_moe_create(_ffi.C.byref(h), 256, 128, 256, 9, 0, 1, 1.0) != 0
    _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), 256, 128, 256, 8, 0, 1, 1.0))
    tm.tm_moe_destroy(h)


def _small_u4_moe(tm, rng, H, I, E, k):
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E, k, 0, 1, 1.0))
    _ffi.check(tm.tm_moe_set_gate(h, dev((0.2 * rng.standard_normal((H, E))).astype(f16)).data_ptr(), st()))
    for e in range(E):
        p13, s13, z13, _, _ = _u4_expert(rng, H, 2 * I, 1.5 / math.sqrt(H))
        p2, s2, z2, _, _ = _u4_expert(rng, I, H, 1.0 / math.sqrt(I))
        _ffi.check(tm.tm_moe_set_expert(h, e, dev(p13).data_ptr(), dev(s13).data_ptr(), dev(z13).data_ptr(), dev(p2).data_ptr(),
                                        dev(s2).data_ptr(), dev(z2).data_ptr(), st()))
    return h


@gpu
def test_forward_stages_equal_the_whole_forward(tm, cuda):
    """tm_moe_forward_stages: the five launches enqueued one by one (gate 1, tables 2, w1w3 4, w2 8, combine 16) on one workspace
    give bit for bit what tm_moe_forward gives; an empty or unknown stage set is a status code"""
    H, I, E, k, T = 256, 128, 72, 8, 37
    rng = np.random.default_rng(5)
    h = _small_u4_moe(tm, rng, H, I, E, k)
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
        assert tm.tm_moe_forward_stages(h, whole.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), 0, st()) != 0
        assert tm.tm_moe_forward_stages(h, whole.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), 32, st()) != 0
    finally:
        tm.tm_moe_destroy(h)
        release_all()


@gpu
def test_grouped_gemm_grid_z_overflow_is_a_status_code(tm, cuda):
    """256 experts x ceil(16384 / 64) row blocks = 65536 > 65535: the grouped GEMM launcher returns a status with a message and
    launches nothing (the w1w3 stage alone is asked for, so no other kernel runs either); one row block fewer is accepted.
    tm_engine_create refuses the same product at creation instead of at the first large prefill."""
    from lmdeploy_amd.turbomind.engine import Engine
    from tests.qwen_moe_reference import QWEN3_MOE_CFG, QwenMoeConfig
    H, I, E, k = 128, 128, 256, 1
    rng = np.random.default_rng(6)
    h = _small_u4_moe(tm, rng, H, I, E, k)
    try:
        T = 16384
        xd = torch.zeros((T, H), dtype=torch.float16, device='cuda')
        out = torch.zeros((T, H), dtype=torch.float16, device='cuda')
        ws = torch.zeros((tm.tm_moe_workspace(h, T),), dtype=torch.uint8, device='cuda')
        _ffi.check(tm.tm_moe_forward_stages(h, out.data_ptr(), xd.data_ptr(), 64, ws.data_ptr(), 31, st()))   # prepares the block
        torch.cuda.synchronize()
        rc = tm.tm_moe_forward_stages(h, out.data_ptr(), xd.data_ptr(), T, ws.data_ptr(), 4, st())
        assert rc != 0 and 'grid.z' in _ffi.last_error()
        torch.cuda.synchronize()
        _ffi.check(tm.tm_moe_forward_stages(h, out.data_ptr(), xd.data_ptr(), T - 64, ws.data_ptr(), 31, st()))   # 255 x 256 blocks
        torch.cuda.synchronize()
    finally:
        tm.tm_moe_destroy(h)
        release_all()
    cfg = QwenMoeConfig(**dict(QWEN3_MOE_CFG, moe_experts=256), kv_bits=8, weight_format='u4')
    with pytest.raises(_ffi.TmError, match='grid.z'):
        Engine.from_model_config(cfg, max_batch_size=2, session_len=128, quant_policy=8, max_prefill_token_num=16384)
    Engine.from_model_config(cfg, max_batch_size=2, session_len=128, quant_policy=8, max_prefill_token_num=16320).close()
