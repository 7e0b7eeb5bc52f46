"""FP8 KV cache (quant_policy 16, TM_KV_BITS_FP8) against tests/fp8_kv_reference.py: store and flatten bit for bit, decode attention
(attention_decode_fp8_mfma.hip) within 1e-2 |ref| + 2e-3 of the float64 reference (the int8 / int4 MFMA kernel's bound), masking bit
for bit, the engine's decode against its own prefill within 2 x the int8 engine's difference, and the refusals by name.  (Through
turbomind.engine.Engine: TurbomindEngineConfig, and with it pipeline(), still turns quant_policy=16 away.)"""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests import fp8_kv_reference as r
from tests.attention_window_reference import window_decode
from tests.gpu_helpers import DevCache, dev, host, rope_table, st
from tests.test_gpu_sliding_window import _tables

pytestmark = pytest.mark.gpu
f16 = np.float16
KLEN = [1, 63, 64, 65, 128, 200, 330]
WINDOWS = [0, 1, 33, 64, 100]
HEADS = [(2, 2), (8, 2), (16, 2), (16, 1)]
SPLITS = [1, 2, 5]
LAYER = 1
KS, VS = 0.37, 2.9
_CACHE = {}


def _case(D, Hkv):   # filled pool + the K / V codes of every sequence, built once per (D, Hkv) and left unchanged
    if (D, Hkv) not in _CACHE:
        rng = np.random.default_rng(D + Hkv)
        L = r.Fp8Layout(2, Hkv, D)
        tables, total = _tables(rng, KLEN)
        pool = np.zeros((total, L.block_size), np.uint8)
        kv = []
        for b, n in enumerate(KLEN):
            k = rng.standard_normal((n, Hkv, D)).astype(f16)
            v = (rng.standard_normal((n, Hkv, D)) * VS).astype(f16)
            if n > 40:
                k[n // 3] *= f16(6.0)        # a dominant key outside the small windows: leaking it would be seen
                k[n - 5] *= f16(4.0)         # and one inside: forces the online-softmax rescale
            kv.append(r.store(pool, L, tables[b], LAYER, 0, k, v, KS, VS))
        _CACHE[(D, Hkv)] = (L, tables, total, pool, kv)
    return _CACHE[(D, Hkv)]


def _queries(D, Hq):
    return np.random.default_rng(1000 + D + Hq).standard_normal((len(KLEN), Hq * D)).astype(f16)


def _run(tm, D, Hq, Hkv, splits, window, sinks=None, pool=None):   # one tm_decode_attention_window launch over KLEN -> fp16 [B, Hq, D]
    L, tables, total, clean, _ = _case(D, Hkv)
    B = len(KLEN)
    dc = DevCache(L, total, tables)
    dc.pool.copy_(torch.from_numpy(clean if pool is None else pool).cuda())
    out = torch.zeros((B, Hq * D), dtype=torch.float16, device='cuda')
    ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
    _ffi.check(tm.tm_decode_attention_window(out.data_ptr(), dev(_queries(D, Hq)).data_ptr(), Hq * D, dev(np.asarray(KLEN, np.int32)).data_ptr(),
                                             B, Hq, 0.0, splits, ws.data_ptr(), r.view(dc, LAYER, KS, VS), window,
                                             None if sinks is None else dev(sinks).data_ptr(), st()))
    return host(out).reshape(B, Hq, D)


def _thinned():   # every window, GQA group and split count with both head_dims; splits 5 with W 33 (empty splits) always
    return [(D, *HEADS[(wi + di) % 4], 5 if W == 33 else SPLITS[(wi + di) % 3], W)
            for di, D in enumerate((64, 128)) for wi, W in enumerate(WINDOWS)]


@pytest.mark.parametrize('D,Hq,Hkv,splits,W', _thinned())
def test_decode_accuracy(tm, cuda, D, Hq, Hkv, splits, W):   # without sinks and with random sinks in [-2, 4]
    kv, q = _case(D, Hkv)[4], _queries(D, Hq)
    for sinks in (None, np.random.default_rng(Hq + W).uniform(-2.0, 4.0, Hq).astype(f16)):
        got = _run(tm, D, Hq, Hkv, splits, W, sinks)
        for b, n in enumerate(KLEN):
            ref = window_decode(q[b].reshape(Hq, D), r.dequantise(kv[b][0], KS), r.dequantise(kv[b][1], VS), W, None, sinks).astype(np.float32)
            err = np.abs(got[b].astype(np.float32) - ref)
            print(f'[fp8 decode] D {D} heads {Hq}/{Hkv} W {W} splits {splits} sinks {sinks is not None} k_len {n}: max err {err.max():.5f}')
            assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'k_len {n}: max err {err.max()}'

@pytest.mark.parametrize('W,splits', [(33, 5), (100, 2), (64, 1), (0, 2)])
@pytest.mark.parametrize('D', [64, 128])
def test_masked_bytes_move_no_bit(tm, cuda, D, W, splits):
    """every byte of every token outside [wbeg, ctx) in the sequences' blocks, positions past ctx included, becomes 0xff (K) / 0x7f (V)"""
    Hq, Hkv = 8, 2
    L, tables, total, clean, _ = _case(D, Hkv)
    pool = clean.copy()
    for b, n in enumerate(KLEN):
        wbeg = max(n - W, 0) if W > 0 else 0
        for t in [t for t in range(len(tables[b]) * 64) if t < wbeg or t >= n]:
            for hd in range(Hkv):
                a, c = L.k_data(LAYER, hd, t % 64), L.v_data(LAYER, hd, t % 64)
                pool[tables[b][t // 64], a:a + D] = 0xff
                pool[tables[b][t // 64], c:c + D] = 0x7f
    sinks = np.linspace(-2, 4, Hq).astype(f16)
    want = _run(tm, D, Hq, Hkv, splits, W, sinks)
    dirty = _run(tm, D, Hq, Hkv, splits, W, sinks, pool=pool)
    assert not np.isnan(dirty.astype(np.float32)).any()
    assert np.array_equal(dirty.view(np.uint16), want.view(np.uint16))
    # a sink of -inf gives the bits of no sink; a covering window those of W = 0
    plain = _run(tm, D, Hq, Hkv, splits, W).view(np.uint16)
    assert np.array_equal(_run(tm, D, Hq, Hkv, splits, W, np.full(Hq, -np.inf, f16)).view(np.uint16), plain)
    if W == 0:
        assert all(np.array_equal(_run(tm, D, Hq, Hkv, splits, Wc).view(np.uint16), plain) for Wc in (330, 4096))


@pytest.mark.parametrize('ks,vs', [(1.0, 1.0), (KS, VS)])
@pytest.mark.parametrize('D', [64, 128])
def test_store_bit_for_bit(tm, cuda, D, ks, vs):
    """a prefill chunk over a block boundary (positions 50 .. 79) and a decode append (127); every 7th row is scaled past 448 * scale"""
    Hq, Hkv, hist, qlen = 4, 2, [50, 127], [30, 1]
    rng = np.random.default_rng(D)
    L = r.Fp8Layout(2, Hkv, D)
    tables, T, rp = [np.array([3, 1]), np.array([0, 4])], sum(qlen), o.RopeParam(D, 10000.0)
    qkv = rng.standard_normal((T, Hq + 2 * Hkv, D)).astype(f16)
    qkv[::7] *= f16(600.0)
    want = np.zeros((5, L.block_size), np.uint8)
    row = 0
    for b in range(2):
        cos, sin = o.rope_cos_sin(rp, np.arange(hist[b], hist[b] + qlen[b]))
        rows = qkv[row:row + qlen[b]]
        r.store(want, L, tables[b], LAYER, hist[b], o.rope_apply(rows[:, Hq:Hq + Hkv], cos, sin), rows[:, Hq + Hkv:], ks, vs)
        row += qlen[b]
    dc = DevCache(L, 5, tables)
    klen = np.asarray([h + n for h, n in zip(hist, qlen)], np.int32)
    _ffi.check(tm.tm_kv_rope_store(dev(qkv).data_ptr(), Hq, dev(np.asarray([0, 30, 31], np.int32)).data_ptr(), dev(klen).data_ptr(), 2, T,
                                   dev(rope_table(tm, 256, rp)).data_ptr(), 256, r.view(dc, LAYER, ks, vs), st()))
    got = dc.download()
    assert (want == 0x7e).any() or (want == 0xfe).any(), 'the clamp was not exercised'
    assert np.array_equal(got, want), f'{np.count_nonzero(got != want)} bytes differ'


@pytest.mark.parametrize('vt', [0, 1])
@pytest.mark.parametrize('D,window', [(64, 0), (128, 0), (64, 70), (128, 70)])
def test_flatten_bit_for_bit(tm, cuda, D, vt, window):
    """tm_flatten_kv / _window over KLEN; with the window (q_len 1) the tiles ending at or below k_len - 1 - 70 + 1 keep the sentinel"""
    Hkv, B = 2, len(KLEN)
    L, tables, total, pool, kv = _case(D, Hkv)
    dc = DevCache(L, total, tables)
    dc.pool.copy_(torch.from_numpy(pool).cuda())
    off = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in KLEN])]).astype(np.int32)
    stride = int(off[-1])
    ko = torch.full((Hkv, stride, D), 0x7e00, dtype=torch.int16, device='cuda')
    vo = torch.full((Hkv, D, stride) if vt else (Hkv, stride, D), 0x7e00, dtype=torch.int16, device='cuda')
    args = (ko.data_ptr(), vo.data_ptr(), vt, dev(off).data_ptr(), dev(np.asarray(KLEN, np.int32)).data_ptr(), B, max(KLEN), stride,
            r.view(dc, LAYER, KS, VS))
    if window:
        _ffi.check(tm.tm_flatten_kv_window(*args, dev(np.arange(B + 1, dtype=np.int32)).data_ptr(), window, st()))
    else:
        _ffi.check(tm.tm_flatten_kv(*args, st()))
    kg, vg = host(ko).view(np.uint16), host(vo).view(np.uint16)
    vg = vg.transpose(0, 2, 1) if vt else vg
    for b, n in enumerate(KLEN):
        lo = max(n - 1 - window + 1, 0) // 64 * 64 if window else 0       # first token of the first tile that is not skipped
        for got, codes, s in ((kg, kv[b][0], KS), (vg, kv[b][1], VS)):
            seq = got[:, off[b]:off[b] + n]
            assert np.array_equal(seq[:, lo:], r.dequantise(codes, s, f16).view(np.uint16)[:, lo:]), f'sequence {b}'
            assert (seq[:, :lo] == 0x7e00).all(), f'sequence {b}: a skipped tile was written'


def _last_logits(cfg, w, prompt, quant_policy, scales):
    out = []   # logits behind prefill(n) + decode(1), then the last row of prefill(n + 1) with the same n + 1 tokens
    eng = Engine.from_model_config(cfg, max_batch_size=2, session_len=256, quant_policy=quant_policy, max_prefill_token_num=96)
    if scales:
        eng.set_kv_scales(*scales)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill([prompt], max_new_tokens=2)
    eng.decode(1)
    out.append(eng.fetch_logits()[0].astype(np.float32))
    tok = int(eng.fetch()[0, 0])
    eng.release()
    eng.prefill([np.append(prompt, tok).astype(np.int32)], max_new_tokens=1)
    out.append(eng.fetch_logits()[0].astype(np.float32))
    eng.close()
    return out


@pytest.mark.parametrize('D', [128, 64])
def test_engine_decode_matches_prefill(cuda, D):
    """a tiny Llama, n = 70 (crosses the 64-token block): quant_policy 16 with non-unit scales next to quant_policy 8 as the yardstick"""
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4 * 128 // D, kv_heads=2, head_dim=D, inter=512, vocab=1024, kv_bits=8,
                        rope=o.RopeParam(D, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192))
    w = o.make_synthetic_weights(cfg, seed=5)
    prompt = np.random.default_rng(D).integers(0, cfg.vocab, 70).astype(np.int32)
    a, b = _last_logits(cfg, w, prompt, 16, ([0.05, 0.03], [0.02, 0.04]))
    c, d = _last_logits(cfg, w, prompt, 8, None)
    # the scales reach the kernels: at 64 the rows (|x| below 1) fall into e4m3's subnormals, step 64 * 2^-9; an engine that ignored the
    # setter would return the bits of the engine above
    coarse = _last_logits(cfg, w, prompt, 16, ([64.0, 64.0], [64.0, 64.0]))[0]
    print(f'[fp8 engine] head_dim {D}: max logit diff of scales 64 against the scales above: {np.abs(coarse - a).max():.5f}')
    assert not np.array_equal(coarse, a)
    fp8, int8 = float(np.abs(a - b).max()), float(np.abs(c - d).max())
    print(f'[fp8 engine] head_dim {D}: decode vs prefill max logit diff: quant_policy 16 {fp8:.5f}, quant_policy 8 {int8:.5f}')
    assert np.isfinite(a).all() and fp8 <= 2 * int8, f'FP8 {fp8} vs int8 {int8}'


def test_refusals_by_name(tm, cuda):
    L, tables, total, _, _ = _case(128, 2)
    c = r.view(DevCache(L, total, tables), LAYER, KS, VS)
    B, Hq, buf = len(KLEN), 8, torch.zeros(1 << 20, dtype=torch.uint8, device='cuda').data_ptr()
    kl, cu = dev(np.asarray(KLEN, np.int32)).data_ptr(), dev(np.arange(B + 1, dtype=np.int32)).data_ptr()
    for rc in (tm.tm_decode_attention_window_mfma(buf, buf, Hq * 128, kl, B, Hq, 0.0, 1, None, c, 0, None, st()),
               tm.tm_verify_attention(buf, buf, Hq * 128, cu, kl, B, Hq, 0.0, 1, None, c, st()),
               tm.tm_decode_attention_fused(buf, buf, 0, (Hq + 4) * 128, None, 0, kl, B, Hq, 0.0, 1, None, c, st()),
               tm.tm_kv_rope_store_mrope(buf, Hq, cu, kl, B, B, buf, 512, None, None, 16, 24, 24, None, None, None, 0.0, c, st())):
        assert rc == 1 and ('FP8' in _ffi.last_error() or 'int8 / int4' in _ffi.last_error()), _ffi.last_error()
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024)
    for kw, reason in ((dict(quant_policy=17), 'quant_policy 17'), (dict(quant_policy=16, tp=2), 'tp > 1')):
        with pytest.raises(_ffi.TmError, match=reason):
            Engine.from_model_config(cfg, max_batch_size=2, session_len=128, **kw)
    eng = Engine.from_model_config(cfg, max_batch_size=2, session_len=128, quant_policy=16)
    with pytest.raises(_ffi.TmError, match='FP8 KV'):
        eng.set_mrope_section((16, 24, 24))
    eng.load_weights(export_weights(cfg, o.make_synthetic_weights(cfg, seed=1)))
    eng.start()
    for call in (lambda: eng.set_speculative(3), lambda: eng.set_multimodal([dict(prompt_len=4)])):
        with pytest.raises(_ffi.TmError, match='FP8 KV'):
            call()
    eng.close()
