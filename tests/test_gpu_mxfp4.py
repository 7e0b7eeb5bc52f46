"""MXFP4 experts and the gpt-oss MoE block through the C-ABI, against tests/mxfp4_reference.py.

  * tm_mxfp4_dequant_f16 (repack + the grouped GEMM's own dequant function) equals the reference bit for bit on a matrix holding
    every (code, scale byte) pair of the edge list: the flush, the clamp, -0, inf;
  * exactly summable blocks (mxfp4_reference.exact_block): router bias that decides the picks, both grouped GEMMs, the gated gpt-oss
    epilogue with its bias, the combine with the w2 bias -- every comparison an equality, for T in {1, 3, 17, 33, 65} (every decode row
    tile by the rule and forced, and the prefill form), 8 experts / top-2 on the serial router and 72 / top-8 on the wide one, run twice
    on one poisoned, never cleared workspace; the same blocks with their weights handed over as fp16 experts (the fp16 arm of the
    gpt-oss epilogue); a single code off by one must show;
  * random data against the reference under the bound of the fp16-expert operator tests (tests/test_gpu_moe_f16.py: 4e-3 + 2^-6 |ref|,
    ids exact, weights within 1e-5): the arithmetic after the exact dequantisation is theirs;
  * u4 and fp16 blocks given activation 0 and a NULL router bias produce the bits of blocks the new setters never touched."""
import math

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import mxfp4_reference as r
from tests.gpu_helpers import dev, host, release_all, st

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
U4, F16, MXFP4 = 0, 1, 3
H, I = 256, 128              # w1w3: two k-blocks (8 scale groups), w2: one
TILES = (0, 16, 32, 64)      # 0: the launcher's own rule


def _create(tm, E, k, wtype, norm_topk=1, scale=1.0):
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E, k, wtype, norm_topk, scale))
    return h


def _gptoss_block(tm, E, k, gate, gate_bias, experts, wtype=MXFP4):
    """experts: mxfp4_reference expert dicts (w1w3 / w2 = blocks + scales, w13 / w2d dequantised, b13, b2)"""
    h = _create(tm, E, k, wtype)
    _ffi.check(tm.tm_moe_set_gate(h, dev(gate).data_ptr(), st()))
    _ffi.check(tm.tm_moe_set_activation(h, 1))
    if gate_bias is not None:
        _ffi.check(tm.tm_moe_set_gate_bias(h, dev(np.asarray(gate_bias, f32)).data_ptr(), st()))
    for e, ex in enumerate(experts):
        if wtype == MXFP4:
            _ffi.check(tm.tm_moe_set_expert(h, e, dev(ex['w1w3']['blocks']).data_ptr(), dev(ex['w1w3']['scales']).data_ptr(), None,
                                            dev(ex['w2']['blocks']).data_ptr(), dev(ex['w2']['scales']).data_ptr(), None, st()))
        else:
            _ffi.check(tm.tm_moe_set_expert(h, e, dev(ex['w13']).data_ptr(), None, None, dev(ex['w2d']).data_ptr(), None, None, st()))
        if ex['b13'] is not None:
            _ffi.check(tm.tm_moe_set_expert_bias(h, e, dev(ex['b13']).data_ptr(), dev(ex['b2']).data_ptr(), st()))
    release_all()
    return h


def _forward(tm, h, x, k, rows=0, ws=None):
    """-> (out fp16, ids, w); ws: a workspace to reuse as it is (else a fresh one poisoned with 0xFF)"""
    T = len(x)
    if ws is None:
        ws = torch.full((tm.tm_moe_workspace(h, T),), 0xFF, dtype=torch.uint8, device='cuda')
    out = torch.zeros((T, H), dtype=torch.float16, device='cuda')
    ids = torch.zeros((T, k), dtype=torch.int32, device='cuda')
    w = torch.zeros((T, k), dtype=torch.float32, device='cuda')
    _ffi.check(tm.tm_debug_set_grouped_rows(rows))
    try:
        _ffi.check(tm.tm_moe_forward(h, out.data_ptr(), dev(x).data_ptr(), T, ws.data_ptr(), ids.data_ptr(), w.data_ptr(), st()))
        torch.cuda.synchronize()
    finally:
        tm.tm_debug_set_grouped_rows(0)
    return host(out), host(ids), host(w), ws


def test_dequant_every_code_and_scale_byte(tm, cuda):
    """K 256, N 32: column n's scale group g holds byte SCALE_BYTES[(g + n) % 8] and the codes (k + n) % 16 -- all 128 pairs, at
    every position of a lane's dword and in every k-step of both k-blocks"""
    K, N = 256, 32
    codes = ((np.arange(K)[None, :] + np.arange(N)[:, None]) % 16).astype(np.uint8)
    scales = np.array(r.SCALE_BYTES, np.uint8)[(np.arange(K // 32)[None, :] + np.arange(N)[:, None]) % 8]
    pairs = {(int(c), int(s)) for c, s in zip(codes.ravel(), np.repeat(scales, 32, axis=1).ravel())}
    assert len(pairs) == 16 * len(r.SCALE_BYTES)
    blocks = r.pack_codes(codes)
    ref = r.dequant(blocks, scales)
    assert np.isinf(ref.astype(f32)).any() and (ref.view(np.uint16) == 0x8000).any()
    out = torch.full((K, N), float('nan'), dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_mxfp4_dequant_f16(out.data_ptr(), dev(blocks).data_ptr(), dev(scales).data_ptr(), K, N, st()))
    torch.cuda.synchronize()
    got = host(out)
    bad = np.argwhere(got.view(np.uint16) != ref.view(np.uint16))
    assert len(bad) == 0, f'{len(bad)} weights differ, first (k, n) = {bad[0]}: code {codes[bad[0][1], bad[0][0]]} scale byte ' \
                          f'{scales[bad[0][1], bad[0][0] // 32]}: got {got[tuple(bad[0])]} want {ref[tuple(bad[0])]}'


@pytest.fixture(scope='module')
def exact_blocks():
    """the exact blocks, built once and shared (never modified): {(E, k, T): block}"""
    return {(E, k, T): r.exact_block(H, I, E, k, T) for E, k in ((8, 2), (72, 8)) for T in (1, 3, 17, 33, 65)}


def _check_exact(tm, h, b, k, what):
    ws = None
    for rows in (TILES if len(b.x) <= 64 else (0,)):
        for rep in range(2):      # the second run reads a workspace the first one left: nothing may depend on its contents
            out, ids, w, ws = _forward(tm, h, b.x, k, rows, ws)
            lab = f'{what} rows {rows or "auto"} run {rep}'
            assert np.array_equal(ids, b.ids), f'{lab}: routing'
            assert np.array_equal(w.view(np.uint32), b.w.view(np.uint32)), f'{lab}: routing weights'
            bad = np.argwhere(r.bits(out) != r.bits(b.out))
            assert len(bad) == 0, f'{lab}: {len(bad)} of {out.size} outputs differ, first at {bad[0]}: {out[tuple(bad[0])]} != {b.out[tuple(bad[0])]}'


@pytest.mark.parametrize('T', [1, 3, 17, 33, 65])
@pytest.mark.parametrize('E,k', [(8, 2), (72, 8)])
def test_exact_block_mxfp4(tm, cuda, exact_blocks, E, k, T):
    b = exact_blocks[(E, k, T)]
    h = _gptoss_block(tm, E, k, b.gate, b.gate_bias, b.experts)
    try:
        _check_exact(tm, h, b, k, f'mxfp4 E {E} k {k} T {T}')
    finally:
        tm.tm_moe_destroy(h)


@pytest.mark.parametrize('T', [17, 65])
def test_exact_block_f16_experts(tm, cuda, exact_blocks, T):
    """the same block with the (exactly) dequantised weights as fp16 experts: the gpt-oss epilogue, biases and combine on the fp16 arm"""
    b = exact_blocks[(8, 2, T)]
    h = _gptoss_block(tm, 8, 2, b.gate, b.gate_bias, b.experts, wtype=F16)
    try:
        _check_exact(tm, h, b, 2, f'f16 T {T}')
    finally:
        tm.tm_moe_destroy(h)


def test_a_code_off_by_one_shows(tm, cuda, exact_blocks):
    """negative control: one e2m1 code of one used expert's w2 changed by one step changes output bits"""
    b = exact_blocks[(8, 2, 17)]
    e0 = int(b.ids[0, 0])
    c = r.unpack_codes(b.experts[e0]['w2']['blocks'])
    c[5, 3] ^= 1
    experts = list(b.experts)
    experts[e0] = dict(b.experts[e0], w2=dict(blocks=r.pack_codes(c), scales=b.experts[e0]['w2']['scales']))
    h = _gptoss_block(tm, 8, 2, b.gate, b.gate_bias, experts)
    try:
        out, ids, _, _ = _forward(tm, h, b.x, 2)
        assert np.array_equal(ids, b.ids)
        diff = r.bits(out) != r.bits(b.out)
        assert diff[:, 5].any() and not diff[:, np.arange(H) != 5].any(), 'the changed weight feeds output column 5, and only it'
    finally:
        tm.tm_moe_destroy(h)


def _aimed(rng, E, k, T):
    """(x, gate, gate_bias): a router that sends token t to a random pick list in its order (3.0, 2.875, ... on the picks, U(-1, 0)
    elsewhere, tests/test_gpu_moe_wide._picked_x) under a bias of +-1/32 that cannot reorder them"""
    gate = (rng.standard_normal((H, E)) * 0.00005).astype(f16)
    gate[:E] = np.eye(E, dtype=f16)
    x = rng.standard_normal((T, H)).astype(f16)
    x[:, :E] = rng.uniform(-1.0, 0.0, (T, E)).astype(f16)
    picks = [rng.permutation(E)[:k].tolist() for _ in range(T)]
    for t, p in enumerate(picks):
        for j, e in enumerate(p):
            x[t, e] = f16(3.0 - 0.125 * j)
    return x, gate, (rng.integers(-1, 2, E) / 32.0).astype(f32), np.asarray(picks, np.int32)


@pytest.mark.parametrize('E,k,T,bias', [(8, 2, 17, True), (8, 2, 65, True), (72, 8, 33, True), (8, 2, 33, False)])
def test_random_block_within_the_f16_bound(tm, cuda, E, k, T, bias):
    """random codes, scales, biases and activations; with and without the biases (activation 1 alone)"""
    rng = np.random.default_rng([9, E, T])
    x, gate, gb, picks = _aimed(rng, E, k, T)
    experts = [r.random_expert(rng, H, I, bias=bias) for _ in range(E)]
    ref, ids, w = r.block_forward(x, gate, gb if bias else None, [r.dense(ex) for ex in experts], k)
    assert np.array_equal(ids, picks)
    ref = ref.astype(f32)
    tol = 4e-3 + 2.0**-6 * np.abs(ref)
    assert np.any(np.abs(ref) > tol) and np.any(0.25 * np.abs(ref) > tol), 'outputs too small to test'
    h = _gptoss_block(tm, E, k, gate, gb if bias else None, experts)
    try:
        for rows in (TILES if T <= 64 else (0,)):
            out, gids, gw, _ = _forward(tm, h, x, k, rows)
            what = f'E {E} T {T} bias {bias} rows {rows or "auto"}'
            assert np.array_equal(gids, ids), f'{what}: routing differs'
            assert np.abs(gw - w).max() <= 1e-5, what
            err = np.abs(out.astype(f32) - ref)
            print(f'{what}: |ref| max {np.abs(ref).max():.4f}, worst err / tol {(err / tol).max():.3f}')
            assert np.all(err <= tol), f'{what}: max err {err.max()} at {np.unravel_index(np.argmax(err - tol), err.shape)}'
    finally:
        tm.tm_moe_destroy(h)


def test_silu_block_on_mxfp4_experts(tm, cuda):
    """activation 0 on MXFP4 experts: the plain gated-SiLU epilogue of the other formats, same bound"""
    E, k, T = 8, 2, 33
    rng = np.random.default_rng(21)
    x, gate, _, picks = _aimed(rng, E, k, T)
    experts = [r.random_expert(rng, H, I, bias=False) for _ in range(E)]
    ref, ids, _ = r.block_forward(x, gate, None, [r.dense(ex) for ex in experts], k, act=0)
    ref = ref.astype(f32)
    tol = 4e-3 + 2.0**-6 * np.abs(ref)
    h = _create(tm, E, k, MXFP4)
    try:
        _ffi.check(tm.tm_moe_set_gate(h, dev(gate).data_ptr(), st()))
        for e, ex in enumerate(experts):
            _ffi.check(tm.tm_moe_set_expert(h, e, dev(ex['w1w3']['blocks']).data_ptr(), dev(ex['w1w3']['scales']).data_ptr(), None,
                                            dev(ex['w2']['blocks']).data_ptr(), dev(ex['w2']['scales']).data_ptr(), None, st()))
        out, gids, _, _ = _forward(tm, h, x, k)
        assert np.array_equal(gids, ids) and np.array_equal(ids, picks)
        assert np.all(np.abs(out.astype(f32) - ref) <= tol)
    finally:
        tm.tm_moe_destroy(h)


@pytest.mark.parametrize('wtype', [U4, F16])
def test_untouched_blocks_keep_their_bits(tm, cuda, wtype):
    """two blocks on the same u4 / fp16 weights: one never sees the new setters, the other is given activation 0 and a NULL router
    bias -- same routing, same output bits, for a decode and a prefill sized forward.  The gpt-oss activation and expert biases are
    refused on u4 experts with a message."""
    E, k = 8, 2
    rng = np.random.default_rng(33)
    gate = (0.2 * rng.standard_normal((H, E))).astype(f16)
    ws13 = [(rng.standard_normal((H, 2 * I)) * (1.5 / math.sqrt(H))).astype(f16) for _ in range(E)]
    ws2 = [(rng.standard_normal((I, H)) * (1.0 / math.sqrt(I))).astype(f16) for _ in range(E)]
    hs = [_create(tm, E, k, wtype) for _ in range(2)]
    try:
        for h in hs:
            _ffi.check(tm.tm_moe_set_gate(h, dev(gate).data_ptr(), st()))
            for e in range(E):
                if wtype == F16:
                    _ffi.check(tm.tm_moe_set_expert(h, e, dev(ws13[e]).data_ptr(), None, None, dev(ws2[e]).data_ptr(), None, None, st()))
                else:
                    (q13, s13, z13, _), (q2, s2, z2, _) = o.quantize_groupwise_u4(ws13[e]), o.quantize_groupwise_u4(ws2[e])
                    _ffi.check(tm.tm_moe_set_expert(h, e, dev(o.pack_u4_row(q13)).data_ptr(), dev(s13).data_ptr(), dev(z13).data_ptr(),
                                                    dev(o.pack_u4_row(q2)).data_ptr(), dev(s2).data_ptr(), dev(z2).data_ptr(), st()))
            release_all()
        _ffi.check(tm.tm_moe_set_activation(hs[1], 0))
        _ffi.check(tm.tm_moe_set_gate_bias(hs[1], None, st()))
        for T in (17, 65):
            x = rng.standard_normal((T, H)).astype(f16)
            a, b = _forward(tm, hs[0], x, k), _forward(tm, hs[1], x, k)
            assert np.isfinite(a[0].astype(f32)).all() and np.abs(a[0].astype(f32)).max() > 0
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
            assert np.array_equal(a[0].view(np.uint16), b[0].view(np.uint16)), f'T {T}: output bits differ'
        if wtype == U4:
            with pytest.raises(_ffi.TmError, match='fp16 and MXFP4 experts only'):
                _ffi.check(tm.tm_moe_set_activation(hs[1], 1))
            with pytest.raises(_ffi.TmError, match='fp16 and MXFP4 experts only'):
                _ffi.check(tm.tm_moe_set_expert_bias(hs[1], 0, dev(np.zeros(2 * I, f16)).data_ptr(), dev(np.zeros(H, f16)).data_ptr(), st()))
    finally:
        for h in hs:
            tm.tm_moe_destroy(h)
