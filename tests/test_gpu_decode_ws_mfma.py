"""tm_decode_attention_window_mfma (attention_decode_ws_mfma.hip: int8 / int4 KV, head_dim 64 / 128, sliding window and sinks on the
matrix cores) against tests/attention_window_reference.py in fp64.  One batch whose k_len cross every edge of the 64-token tile
(1, 63, 64, 65, 128, 200, 330); the cache is built the way tests/test_gpu_sliding_window.py builds it.

Bound: that file's, err <= 1e-2 |ref| + 2e-3.  Statements about WHICH bytes are read (poisoned tokens before the window) and about
degenerate parameters (a covering window, -inf sinks) are bit for bit."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.attention_window_reference import window_decode
from tests.gpu_helpers import DevCache, dev, host, st
from tests.test_gpu_gpt_oss import _engine_vs_oracle
from tests.test_gpu_sliding_window import _poison, _tables

pytestmark = pytest.mark.gpu
f16 = np.float16
KLEN = [1, 63, 64, 65, 128, 200, 330]
WINDOWS = [0, 1, 33, 64, 100, 330]
HEADS = [(2, 2), (8, 2), (16, 2), (16, 1)]   # GQA group 1, 4, 8, 16
SPLITS = [1, 2, 5]
LAYER = 1
_CACHE = {}


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
                k[n // 3] *= f16(6.0)        # a dominant key outside the small windows: leaking it would be seen
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


def _run(tm, D, bits, Hq, Hkv, splits, window, sinks=None, pool=None):
    """one launch over all of KLEN -> fp16 [B, Hq, D]; pool: cache bytes to use instead of the case's"""
    L, tables, total, oc, _ = _case(D, bits, Hkv)
    B = len(KLEN)
    dc = DevCache(L, total, tables)
    if pool is None:
        dc.upload(oc)
    else:
        dc.pool.copy_(torch.from_numpy(pool).cuda())
    out = torch.zeros((B, Hq * D), dtype=torch.float16, device='cuda')
    ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
    _ffi.check(tm.tm_decode_attention_window_mfma(out.data_ptr(), dev(_queries(D, Hq)).data_ptr(), Hq * D,
                                                  dev(np.asarray(KLEN, np.int32)).data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(),
                                                  dc.view(LAYER), window, None if sinks is None else dev(sinks).data_ptr(), st()))
    return host(out).reshape(B, Hq, D)


def _assert_close(got, D, bits, Hq, Hkv, window, sinks, what):
    kv = _case(D, bits, Hkv)[4]
    q = _queries(D, Hq)
    for b, n in enumerate(KLEN):
        ref = window_decode(q[b].reshape(Hq, D), kv[b][0], kv[b][1], window, None, sinks).astype(np.float32)
        err = np.abs(got[b].astype(np.float32) - ref)
        print(f'[{what}] D {D} bits {bits} heads {Hq}/{Hkv} W {window} k_len {n}: max err {err.max():.5f}')
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'{what}: k_len {n}: max err {err.max()}'


def _thinned():
    """every window, GQA group and split count with every (head_dim, bits); splits 5 with W 33 (empty splits) always"""
    cases = []
    for di, D in enumerate((64, 128)):
        for bi, bits in enumerate((8, 4)):
            for wi, W in enumerate(WINDOWS):
                Hq, Hkv = HEADS[(wi + bi + di) % 4]
                cases.append((D, bits, Hq, Hkv, 5 if W == 33 else SPLITS[(wi + 2 * bi + di) % 3], W))
    return cases


@pytest.mark.parametrize('D,bits,Hq,Hkv,splits,W', _thinned())
def test_accuracy(tm, cuda, D, bits, Hq, Hkv, splits, W):
    """without sinks and with random sinks in [-2, 4]"""
    _assert_close(_run(tm, D, bits, Hq, Hkv, splits, W), D, bits, Hq, Hkv, W, None, 'window')
    sinks = np.random.default_rng(Hq + W).uniform(-2.0, 4.0, Hq).astype(f16)
    _assert_close(_run(tm, D, bits, Hq, Hkv, splits, W, sinks), D, bits, Hq, Hkv, W, sinks, 'window + sinks')


@pytest.mark.parametrize('splits', SPLITS)
@pytest.mark.parametrize('D,bits', [(64, 8), (64, 4), (128, 8), (128, 4)])
def test_covering_window_and_minus_inf_sinks_change_no_bit(tm, cuda, D, bits, splits):
    """W >= the longest k_len walks the tiles of W = 0; a sink of -inf adds exactly +0 to the denominator"""
    Hq, Hkv = 8, 2
    plain = _run(tm, D, bits, Hq, Hkv, splits, 0).view(np.uint16)
    for W in (330, 4096):
        assert np.array_equal(_run(tm, D, bits, Hq, Hkv, splits, W).view(np.uint16), plain), f'W {W}'
    for W in (0, 100):
        got = _run(tm, D, bits, Hq, Hkv, splits, W).view(np.uint16)
        assert np.array_equal(_run(tm, D, bits, Hq, Hkv, splits, W, np.full(Hq, -np.inf, f16)).view(np.uint16), got), f'-inf sinks, W {W}'


@pytest.mark.parametrize('W,splits', [(33, 5), (100, 2), (64, 1), (1, 1)])
@pytest.mark.parametrize('D,bits', [(64, 8), (64, 4), (128, 8), (128, 4)])
def test_never_reads_older_tokens(tm, cuda, D, bits, W, splits):
    """every cache token older than the window: NaN (scale, zero) words and 0xff codes.  Not one output bit may move"""
    Hq, Hkv = 8, 2
    L, tables, total, oc, _ = _case(D, bits, Hkv)
    pool = oc.pool.copy()
    for b, n in enumerate(KLEN):
        _poison(pool, L, tables[b], 0, max(n - W, 0))
    assert not np.array_equal(pool, oc.pool)
    sinks = np.linspace(-2, 4, Hq).astype(f16)
    clean = _run(tm, D, bits, Hq, Hkv, splits, W, sinks)
    dirty = _run(tm, D, bits, Hq, Hkv, splits, W, sinks, pool=pool)
    assert not np.isnan(dirty.astype(np.float32)).any()
    assert np.array_equal(dirty.view(np.uint16), clean.view(np.uint16))


@pytest.mark.parametrize('bits,window,reason', [(16, 0, 'int8 / int4'), (8, -1, 'window')])
def test_refusals(tm, cuda, bits, window, reason):
    """fp16 KV and a negative window: TM_INVALID by name, the output untouched"""
    L, tables, total, oc, _ = _case(64, 8, 2)
    dc = DevCache(o.BlockLayout(2, 2, 64, 64, bits), total, tables)
    out = torch.full((len(KLEN), 8 * 64), 0x7e00, dtype=torch.int16, device='cuda')
    rc = tm.tm_decode_attention_window_mfma(out.data_ptr(), dev(_queries(64, 8)).data_ptr(), 8 * 64, dev(np.asarray(KLEN, np.int32)).data_ptr(),
                                            len(KLEN), 8, 0.0, 1, None, dc.view(LAYER), window, None, st())
    assert rc == 1 and reason in _ffi.last_error()
    torch.cuda.synchronize()
    assert (host(out) == 0x7e00).all()


def test_gpt_oss_engine_int8_kv_graph(cuda):
    """the gpt-oss toy ([sliding 8, full], sinks) with int8 KV, captured: prefill + 3 decode steps through the default dispatch, which
    runs this kernel in every layer, under the parity bound of tests.test_gpu_gpt_oss; contexts that cross a 64-token tile in decode"""
    _engine_vs_oracle('published', 8, 1, prompt_lens=(63, 12, 64))
