"""Sliding-window attention and attention sinks on the GPU, operator level: tm_decode_attention_window (VALU decode kernel, head_dim
64 / 128, KV 16 / 8 / 4 bit, split-K) and tm_prefill_attention_window (MFMA prefill kernel) against tests/attention_window_reference.py.

Bound: the one these operators already carry against the oracle, err <= 1e-2 |ref| + 2e-3 (tests/test_gpu_head_dim64.py).  Everything
that is a statement about WHICH bytes are read (poisoned cache tokens before the window, NaN keys in skipped steps) or about a
degenerate parameter (window 0, window >= context, -inf sinks) is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.attention_window_reference import window_decode, window_prefill
from tests.gpu_helpers import DevCache, dev, host, st

pytestmark = pytest.mark.gpu
f16 = np.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KLEN = [1, 31, 33, 64, 65, 200, 330]
WINDOWS = [1, 33, 64, 100, 4096]
HEADS = [(8, 2), (6, 2), (2, 2)]             # heads per workgroup 4, 3, and no GQA
SPLITS = [1, 2, 5]
LAYER = 1
_CACHE = {}


def _tables(rng, klen, spare=2):
    nblk = [(k + 63) // 64 for k in klen]
    perm = rng.permutation(sum(nblk) + spare)
    tables, off = [], 0
    for nb in nblk:
        tables.append(perm[off:off + nb])
        off += nb
    return tables, sum(nblk) + spare


def _case(D, bits, Hkv):
    """filled cache + the dequantised K / V of every sequence, built once per (D, bits, Hkv) and left unchanged"""
    key = (D, bits, Hkv)
    if key not in _CACHE:
        rng = np.random.default_rng(D + bits + Hkv)
        L = o.BlockLayout(2, Hkv, D, 64, bits)
        tables, total = _tables(rng, KLEN)
        oc = o.PagedKVCache(L, total)
        for b, n in enumerate(KLEN):
            k = rng.standard_normal((n, Hkv, D)).astype(f16)
            v = rng.standard_normal((n, Hkv, D)).astype(f16)
            if n > 40:
                k[n // 3] *= f16(6.0)        # a dominant key OUTSIDE the small windows: leaking it would be seen
                k[n - 5] *= f16(4.0)         # and one inside: forces the online-softmax rescale
            o.process_kv(oc, tables[b], LAYER, k, v, None, None, 0)
        kv = []
        for b, n in enumerate(KLEN):
            pairs = [oc.load_dequant(tables[b], LAYER, hd, 0, n, 'decode') for hd in range(Hkv)]
            kv.append((np.stack([a for a, _ in pairs]), np.stack([c for _, c in pairs])))
        _CACHE[key] = (L, tables, total, oc, kv)
    return _CACHE[key]


def _queries(D, Hq):
    return np.random.default_rng(1000 + D + Hq).standard_normal((len(KLEN), Hq * D)).astype(f16)


def _run_decode(tm, D, bits, Hq, Hkv, splits, window, sinks=None, pool=None, plain=False):
    """one launch over all of KLEN -> fp16 [B, Hq, D]; pool: cache bytes to use instead of the case's; plain: tm_decode_attention"""
    L, tables, total, oc, _ = _case(D, bits, Hkv)
    B = len(KLEN)
    dc = DevCache(L, total, tables)
    if pool is None:
        dc.upload(oc)
    else:
        dc.pool.copy_(torch.from_numpy(pool).cuda())
    out = torch.zeros((B, Hq * D), dtype=torch.float16, device='cuda')
    ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
    head = (out.data_ptr(), dev(_queries(D, Hq)).data_ptr(), Hq * D, dev(np.asarray(KLEN, np.int32)).data_ptr(), B, Hq, 0.0, splits,
            ws.data_ptr(), dc.view(LAYER))
    if plain:
        _ffi.check(tm.tm_decode_attention(*head, st()))
    else:
        _ffi.check(tm.tm_decode_attention_window(*head, window, None if sinks is None else dev(sinks).data_ptr(), st()))
    return host(out).reshape(B, Hq, D)


def _assert_decode(got, D, bits, Hq, Hkv, window, sinks, what):
    kv = _case(D, bits, Hkv)[4]
    q = _queries(D, Hq)
    for b, n in enumerate(KLEN):
        ref = window_decode(q[b].reshape(Hq, D), kv[b][0], kv[b][1], window, None, sinks).astype(np.float32)
        err = np.abs(got[b].astype(np.float32) - ref)
        print(f'[{what}] D {D} bits {bits} heads {Hq}/{Hkv} W {window} k_len {n}: max err {err.max():.5f}')
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'{what}: k_len {n}: max err {err.max()}'


def _thinned():
    """every window, every head shape and every split count with every (head_dim, bits); splits 5 with W 33 (empty splits) always"""
    cases = []
    for di, D in enumerate((64, 128)):
        for bi, bits in enumerate((16, 8, 4)):
            for wi, W in enumerate(WINDOWS):
                Hq, Hkv = HEADS[(wi + bi + di) % 3]
                splits = 5 if W == 33 else SPLITS[(wi + 2 * bi + di) % 3]
                cases.append((D, bits, Hq, Hkv, splits, W))
            have = {c[4] for c in cases if c[:2] == (D, bits)}
            for s in SPLITS:                 # the rotation above may miss a split count for this (D, bits)
                if s not in have:
                    cases.append((D, bits, 8, 2, s, 64))
    return cases


def test_thinning_covers_every_axis():
    cases = _thinned()
    for D in (64, 128):
        for bits in (16, 8, 4):
            mine = [c for c in cases if c[:2] == (D, bits)]
            assert {c[5] for c in mine} == set(WINDOWS) and {c[2:4] for c in mine} == set(HEADS) and {c[4] for c in mine} == set(SPLITS)
            assert (5, 33) in {(c[4], c[5]) for c in mine}


@pytest.mark.parametrize('D,bits,Hq,Hkv,splits,W', _thinned())
def test_decode_window(tm, cuda, D, bits, Hq, Hkv, splits, W):
    """accuracy without sinks and with random sinks in [-2, 4]; a -inf sink is no sink, bit for bit"""
    got = _run_decode(tm, D, bits, Hq, Hkv, splits, W)
    _assert_decode(got, D, bits, Hq, Hkv, W, None, 'window')
    sinks = np.random.default_rng(Hq + W).uniform(-2.0, 4.0, Hq).astype(f16)
    got_s = _run_decode(tm, D, bits, Hq, Hkv, splits, W, sinks)
    _assert_decode(got_s, D, bits, Hq, Hkv, W, sinks, 'window + sinks')
    got_inf = _run_decode(tm, D, bits, Hq, Hkv, splits, W, np.full(Hq, -np.inf, f16))
    assert np.array_equal(got_inf.view(np.uint16), got.view(np.uint16)), 'a -inf sink must not change a bit'


@pytest.mark.parametrize('splits', [1, 2])
@pytest.mark.parametrize('bits', [16, 8, 4])
@pytest.mark.parametrize('D', [64, 128])
def test_decode_sinks_without_window(tm, cuda, D, bits, splits):
    """sinks alone (window 0): the epilogue (splits 1) and the reduce kernel (splits 2) each add the term once"""
    sinks = np.random.default_rng(bits).uniform(-2.0, 4.0, 6).astype(f16)
    _assert_decode(_run_decode(tm, D, bits, 6, 2, splits, 0, sinks), D, bits, 6, 2, 0, sinks, 'sinks')


def _equal_to_plain(tm, D, bits):
    for Hq, Hkv, splits in ((8, 2, 1), (6, 2, 2), (2, 2, 5)):
        plain = _run_decode(tm, D, bits, Hq, Hkv, splits, 0, plain=True)
        for W in (0, 330, 4096):             # none; exactly the longest context; beyond it
            got = _run_decode(tm, D, bits, Hq, Hkv, splits, W)
            assert np.array_equal(got.view(np.uint16), plain.view(np.uint16)), f'D {D} bits {bits} heads {Hq}/{Hkv} splits {splits} W {W}'


@pytest.mark.parametrize('D,bits', [(64, 16), (64, 8), (64, 4), (128, 16)])
def test_decode_window_covering_the_context_equals_plain(tm, cuda, D, bits):
    """W == 0 and W >= k_len are tm_decode_attention bit for bit (where that runs the VALU kernel in this process)"""
    _equal_to_plain(tm, D, bits)


@pytest.mark.parametrize('bits', [8, 4])
def test_decode_window_covering_the_context_equals_plain_valu_d128(tm, cuda, bits):
    """the same at head_dim 128 with int8 / int4 KV.  tm_decode_attention runs those on the MFMA kernel, a windowed call never does;
    the kernel a window >= k_len has to reproduce bit for bit is the VALU one, which tm_decode_attention reaches with TM_ATTN_VALU=1 --
    read once per process, so this comparison runs in a child process.  In this process: W == 0 is the old call, whatever it runs."""
    plain = _run_decode(tm, 128, bits, 8, 2, 2, 0, plain=True)
    assert np.array_equal(_run_decode(tm, 128, bits, 8, 2, 2, 0).view(np.uint16), plain.view(np.uint16))
    r = subprocess.run([sys.executable, '-m', 'tests.test_gpu_sliding_window', str(bits)], cwd=ROOT, env=dict(os.environ, TM_ATTN_VALU='1'),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'equal' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _poison(pool, L, table, t0, t1):
    """tokens [t0, t1) of one sequence, both K and V of every kv head: fp16 NaN data / 0xff codes with NaN (scale, zero) words"""
    base = L.layer_offset(LAYER)
    for t in range(t0, t1):
        blk, ti = int(table[t // 64]), t % 64
        for hd in range(L.kv_heads):
            for data, param in ((L.k_data, L.k_param), (L.v_data, L.v_param)):
                a = base + data(hd, ti)
                if L.bits == 16:
                    pool[blk, a:a + L.token_data_size] = np.tile(np.array([0x00, 0x7e], np.uint8), L.token_data_size // 2)
                else:
                    pool[blk, a:a + L.token_data_size] = 0xff
                    pa = base + param(hd, ti)
                    pool[blk, pa:pa + 4] = np.array([0x00, 0x7e, 0x00, 0x7e], np.uint8)     # 0x7e007e00


@pytest.mark.parametrize('W,splits', [(33, 5), (100, 2), (64, 1), (1, 1)])   # k_len - W mid-tile: 200 - 33, 330 - 100, 65 - 64, ...
@pytest.mark.parametrize('bits', [16, 8, 4])
@pytest.mark.parametrize('D', [64, 128])
def test_decode_window_never_reads_older_tokens(tm, cuda, D, bits, W, splits):
    """every cache token older than the window poisoned with NaN: not one output bit may move"""
    Hq, Hkv = 8, 2
    L, tables, total, oc, _ = _case(D, bits, Hkv)
    pool = oc.pool.copy()
    for b, n in enumerate(KLEN):
        _poison(pool, L, tables[b], 0, max(n - W, 0))
    assert not np.array_equal(pool, oc.pool)
    sinks = np.linspace(-2, 4, Hq).astype(f16)
    clean = _run_decode(tm, D, bits, Hq, Hkv, splits, W, sinks)
    dirty = _run_decode(tm, D, bits, Hq, Hkv, splits, W, sinks, pool=pool)
    assert not np.isnan(dirty.astype(np.float32)).any()
    assert np.array_equal(dirty.view(np.uint16), clean.view(np.uint16))
    _assert_decode(dirty, D, bits, Hq, Hkv, W, sinks, 'poisoned')


def test_decode_negative_window_is_invalid(tm, cuda):
    L, tables, total, oc, _ = _case(64, 8, 2)
    dc = DevCache(L, total, tables)
    out = torch.full((len(KLEN), 8 * 64), 0x7e00, dtype=torch.int16, device='cuda')
    rc = tm.tm_decode_attention_window(out.data_ptr(), dev(_queries(64, 8)).data_ptr(), 8 * 64, dev(np.asarray(KLEN, np.int32)).data_ptr(),
                                       len(KLEN), 8, 0.0, 1, None, dc.view(LAYER), -1, None, st())
    assert rc == 1 and 'window' in _ffi.last_error()
    torch.cuda.synchronize()
    assert (host(out) == 0x7e00).all()


def test_decode_fused_entry_point_stays_refused_at_head_dim_64(tm, cuda):
    L, tables, total, oc, _ = _case(64, 8, 2)
    dc = DevCache(L, total, tables)
    B, Hq = len(KLEN), 8
    out = torch.full((B, Hq * 64), 0x7e00, dtype=torch.int16, device='cuda')
    rc = tm.tm_decode_attention_fused(out.data_ptr(), dev(np.zeros((B, (Hq + 4) * 64), f16)).data_ptr(), 0, (Hq + 4) * 64, None, 0,
                                      dev(np.asarray(KLEN, np.int32)).data_ptr(), B, Hq, 0.0, 1, None, dc.view(LAYER), st())
    assert rc == 1 and 'head_dim' in _ffi.last_error()
    torch.cuda.synchronize()
    assert (host(out) == 0x7e00).all()


# ---- prefill -----------------------------------------------------------------------------------------------------------------------
PREFILL_CASES = [((1,), (0,)), ((16,), (7,)), ((63, 65), (0, 64)), ((130, 5), (100, 0)), ((70,), (200,))]
PREFILL_WINDOWS = [1, 16, 33, 64, 100]


def _prefill_inputs(D, Hq, Hkv, qlens, hist, nan_before=None):
    """nan_before: window W -> K is NaN past every context AND before the first row's window (keys no row may touch)"""
    rng = np.random.default_rng(D + Hq + sum(qlens))
    klen = [h + n for h, n in zip(hist, qlens)]
    koff = np.concatenate([[0], np.cumsum([((k + 63) // 64) * 64 for k in klen])]).astype(np.int32)
    stride = int(koff[-1])
    cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    q = rng.standard_normal((int(cu[-1]), Hq * D)).astype(f16)
    K = np.zeros((Hkv, stride, D), f16)
    Vt = np.zeros((Hkv, D, stride), f16)
    Ks, Vs = [], []
    for b, n in enumerate(klen):
        k = rng.standard_normal((Hkv, n, D)).astype(f16)
        v = rng.standard_normal((Hkv, n, D)).astype(f16)
        if n > 40:
            k[:, n // 4] *= f16(5.0)         # a dominant old key
        K[:, koff[b]:koff[b] + n] = k
        K[:, koff[b] + n:koff[b + 1]] = f16(np.nan)
        if nan_before:
            K[:, koff[b]:koff[b] + max(hist[b] - nan_before + 1, 0)] = f16(np.nan)
        Vt[:, :, koff[b]:koff[b] + n] = v.transpose(0, 2, 1)
        Ks.append(k)
        Vs.append(v)
    return klen, koff, stride, cu, q, K, Vt, Ks, Vs


def _run_prefill(tm, D, Hq, Hkv, qlens, inp, window, sinks=None, plain=False):
    klen, koff, stride, cu, q, K, Vt, _, _ = inp
    out = torch.zeros((int(cu[-1]), Hq * D), dtype=torch.float16, device='cuda')
    head = (out.data_ptr(), dev(q).data_ptr(), Hq * D, dev(K).data_ptr(), dev(Vt).data_ptr(), stride, dev(cu).data_ptr(),
            dev(koff).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), len(qlens), max(qlens), Hq, Hkv, D, 0.0)
    if plain:
        _ffi.check(tm.tm_prefill_attention_hd(*head, st()))
    else:
        _ffi.check(tm.tm_prefill_attention_window(*head, window, None if sinks is None else dev(sinks).data_ptr(), st()))
    return host(out)


def _assert_prefill(got, D, Hq, qlens, hist, inp, window, sinks, what):
    cu, q, Ks, Vs = inp[3], inp[4], inp[7], inp[8]
    for b, n in enumerate(qlens):
        ref = window_prefill(q[cu[b]:cu[b + 1]].reshape(n, Hq, D), Ks[b], Vs[b], hist[b], window, None, sinks)
        ref = ref.reshape(n, -1).astype(np.float32)
        err = np.abs(got[cu[b]:cu[b + 1]].astype(np.float32) - ref)
        print(f'[{what}] D {D} heads {Hq} W {window} seq {b} ({n} on {hist[b]}): max err {err.max():.5f}')
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'{what}: W {window} seq {b}: max err {err.max()}'


@pytest.mark.parametrize('qlens,hist', PREFILL_CASES)
@pytest.mark.parametrize('Hq,Hkv', [(8, 2), (6, 3), (14, 2)])        # G = 4, 2, 1 query heads per wave
@pytest.mark.parametrize('D', [64, 128])
def test_prefill_window(tm, cuda, D, Hq, Hkv, qlens, hist):
    """every window: accuracy without and with sinks; keys past the context and before every row's window are NaN and change nothing"""
    sinks = np.random.default_rng(Hq).uniform(-2.0, 4.0, Hq).astype(f16)
    clean = _prefill_inputs(D, Hq, Hkv, qlens, hist)
    for W in PREFILL_WINDOWS:
        got = _run_prefill(tm, D, Hq, Hkv, qlens, clean, W)
        _assert_prefill(got, D, Hq, qlens, hist, clean, W, None, 'window')
        got_s = _run_prefill(tm, D, Hq, Hkv, qlens, clean, W, sinks)
        _assert_prefill(got_s, D, Hq, qlens, hist, clean, W, sinks, 'window + sinks')
        dirty = _prefill_inputs(D, Hq, Hkv, qlens, hist, nan_before=W)
        got_d = _run_prefill(tm, D, Hq, Hkv, qlens, dirty, W, sinks)
        assert np.array_equal(got_d.view(np.uint16), got_s.view(np.uint16)), f'W {W}: NaN keys outside every window changed the output'


@pytest.mark.parametrize('qlens,hist', PREFILL_CASES)
@pytest.mark.parametrize('D', [64, 128])
def test_prefill_window_covering_the_context_equals_plain(tm, cuda, D, qlens, hist):
    """W == 0 and W >= klen are tm_prefill_attention_hd bit for bit; a -inf sink is no sink"""
    Hq, Hkv = 8, 2
    inp = _prefill_inputs(D, Hq, Hkv, qlens, hist)
    plain = _run_prefill(tm, D, Hq, Hkv, qlens, inp, 0, plain=True)
    for W in (0, max(inp[0]), 4096):
        got = _run_prefill(tm, D, Hq, Hkv, qlens, inp, W)
        assert np.array_equal(got.view(np.uint16), plain.view(np.uint16)), f'W {W}'
    got = _run_prefill(tm, D, Hq, Hkv, qlens, inp, 0, np.full(Hq, -np.inf, f16))
    assert np.array_equal(got.view(np.uint16), plain.view(np.uint16)), '-inf sinks'


def test_prefill_negative_window_is_invalid(tm, cuda):
    inp = _prefill_inputs(64, 8, 2, (16,), (7,))
    klen, koff, stride, cu, q, K, Vt, _, _ = inp
    out = torch.full((16, 8 * 64), 0x7e00, dtype=torch.int16, device='cuda')
    rc = tm.tm_prefill_attention_window(out.data_ptr(), dev(q).data_ptr(), 8 * 64, dev(K).data_ptr(), dev(Vt).data_ptr(), stride,
                                        dev(cu).data_ptr(), dev(koff).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), 1, 16, 8, 2,
                                        64, 0.0, -3, None, st())
    assert rc == 1 and 'window' in _ffi.last_error()
    torch.cuda.synchronize()
    assert (host(out) == 0x7e00).all()


if __name__ == '__main__':
    # child of test_decode_window_covering_the_context_equals_plain_valu_d128: TM_ATTN_VALU=1 is set, so tm_decode_attention runs
    # the VALU kernel at head_dim 128 with int8 / int4 KV
    assert os.environ.get('TM_ATTN_VALU') == '1'
    torch.cuda.set_device(0)
    _equal_to_plain(_ffi.load(), 128, int(sys.argv[1]))
    torch.cuda.synchronize()
    print('equal')
