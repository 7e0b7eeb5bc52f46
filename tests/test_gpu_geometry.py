"""GPU parity at the geometries bench.py publishes but the rest of the suite only runs scaled down:

* decode attention at InternLM2-20B's heads (48 q / 8 kv, int8 KV, batch 128) and at one Llama-3-70B TP=8 rank (8 q / 1 kv,
  int4 KV, batch 64), for the split counts the engine picks and a few it does not, plain and with the fused prologue;
* contexts of up to 8192 tokens (128 blocks) against the oracle and the fp64 reference, ragged and rectangular block tables,
  with a spike row past block 64 (online-softmax rescale late in the context), and prefill attention at those heads;
* GQA groups above 16 (the MFMA decode kernel then splits a group over several workgroups);
* the MoE FFN at Mixtral's width (H 4096, I 14336 / 7168, 8 experts, top-2) for every expert format and every row tile of
  the grouped expert GEMMs, with skewed routings that put rows past the tile the launchers size for.

As in test_gpu_fullsize.py, cache and weight contents are drawn as random codes + random parameters (every byte pattern is a
legal state of the formats), and the oracle's gathers are restated vectorised (pinned on the oracle's own functions here), so
the CPU side stays in seconds per case.  Tolerances are the ones of test_gpu_ops.py / test_gpu_fullsize.py."""
import math

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.gpu_helpers import DevCache, dev, host, rope_table, st
from tests.test_gpu_fullsize import _random_cache

f16 = np.float16
gpu = pytest.mark.gpu        # every test here but the host-only restatement checks


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _seq_kv(oc, table, layer, n):
    """K, V fp16 [Hkv, n, 128] of one sequence in the decode kernel's dequantisation: oc.load_dequant(..., 'decode') for
    every kv head, gathered a block at a time instead of a token at a time (pinned by _check_seq_kv)."""
    L = oc.layout
    blk = oc.pool[np.asarray(table, np.int64)][:, L.layer_offset(layer):L.layer_offset(layer) + L.layer_size]
    rows = blk.shape[0] * L.block_len
    Ks, Vs = [], []
    for hd in range(L.kv_heads):
        kv = []
        for d0, p0 in ((L.k_data(hd, 0), L.k_param(hd, 0)), (L.v_data(hd, 0), L.v_param(hd, 0))):
            raw = np.ascontiguousarray(blk[:, d0:d0 + L.head_data_size]).reshape(rows, L.token_data_size)[:n]
            if L.bits == 16:
                kv.append(np.ascontiguousarray(raw).view(f16))
                continue
            q = raw if L.bits == 8 else o.kv_unpack_int4(raw)
            par = np.ascontiguousarray(blk[:, p0:p0 + L.head_param_size]).view(f16).reshape(rows, 2)[:n]
            kv.append(o.kv_dequant_decode(q, par[:, 0], par[:, 1]))
        Ks.append(kv[0])
        Vs.append(kv[1])
    return np.stack(Ks), np.stack(Vs)


def _check_seq_kv(oc, table, layer, n):
    K, V = _seq_kv(oc, table, layer, n)
    for hd in range(oc.layout.kv_heads):
        kr, vr = oc.load_dequant(table, layer, hd, 0, n, 'decode')
        assert np.array_equal(K[hd].view(np.uint16), kr.view(np.uint16)) and np.array_equal(V[hd].view(np.uint16), vr.view(np.uint16))


def _engine_splits(Hq, Hkv, bits, batch):
    """setup_decode (engine_forward.hip) restated: query heads per workgroup, then the split count that brings the decode
    launch to 256 (MFMA kernel, batch >= 32) or 512 workgroups, at most 16"""
    mfma = bits in (8, 4)
    group = Hq // Hkv
    if mfma:
        hpw = group
        while hpw > 16:
            d = 2
            while hpw % d:
                d += 1
            hpw //= d
    else:
        hpw = next(c for c in (4, 3, 2, 1) if group % c == 0)
    wgs = Hkv * (group // hpw) * batch
    splits = 1
    while wgs * splits < (256 if mfma and batch >= 32 else 512) and splits < 16:
        splits *= 2
    return splits


def _qkv_splits(tm, hidden, qkv_n, M):
    """the split-K count of the engine's w_qkv GEMM at the decode batch (the fused prologue then sums that many fp32 slabs)"""
    s, p = _ffi.C.c_int(0), _ffi.C.c_int(0)
    _ffi.check(tm.tm_debug_pick_tiling(hidden, qkv_n, M, 0x100, _ffi.C.byref(s), _ffi.C.byref(p)))
    return p.value if p.value > 1 else 0


def _decode(tm, dc, q, q_stride, klen_d, B, Hq, splits, layer):
    out = torch.zeros((B, Hq * 128), dtype=torch.float16, device='cuda')
    ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
    _ffi.check(tm.tm_decode_attention(out.data_ptr(), q.data_ptr(), q_stride, klen_d.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(),
                                      dc.view(layer), st()))
    return host(out).reshape(B, Hq, 128).astype(np.float32)


def _check_decode(got, refs64, refs, what):
    assert np.isfinite(got).all(), what
    for b, r64 in refs64.items():
        err = np.abs(got[b] - r64)
        assert np.all(err <= 1e-2 * np.abs(r64) + 3e-3), f'{what} seq {b}: max err {err.max()} vs fp64'
    for b, r in refs.items():
        err = np.abs(got[b] - r)
        assert np.all(err <= 1e-2 * np.abs(r) + 2e-3), f'{what} seq {b}: max err {err.max()} vs oracle'


def _refs(oc, tables, layer, klen, q, Hq, check):
    """fp64 unfused reference for every sequence, the oracle's tiled fp16-flow restatement for those in `check`"""
    refs64, refs = {}, {}
    for b, n in enumerate(klen):
        K, V = _seq_kv(oc, tables[b], layer, n)
        qb = q[b].reshape(Hq, 128)
        refs64[b] = o.attention_reference_unfused(qb, K, V).astype(np.float32)
        if b in check:
            refs[b] = o.decode_attention(qb, K, V, None, 1).astype(np.float32)
    return refs64, refs


def _ragged(rng, B):
    klen = rng.integers(1, 2048, B).tolist()
    klen[:4] = [1, 64, 65, 2047]
    return klen


# (Hq, Hkv, KV bits, batch): BASELINE config 3 (InternLM2-20B) and config 4 (Llama-3-70B, one TP = 8 rank)
GEOMETRIES = [(48, 8, 8, 128), (8, 1, 4, 64)]


# ------------------------------------------------------------------------------------------------
# A. decode attention at the published geometries
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('Hq,Hkv,bits,B', GEOMETRIES)
def test_engine_decode_splits_match_restatement(cuda, Hq, Hkv, bits, B):
    """a 1-layer engine with these heads reports the split count _engine_splits restates (what the tests below run)"""
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights

    cfg = o.ModelConfig(hidden=256, layers=1, q_heads=Hq, kv_heads=Hkv, head_dim=128, inter=256, vocab=256, kv_bits=bits)
    w = o.make_synthetic_weights(cfg, seed=3)
    eng = Engine.from_model_config(cfg, max_batch_size=B, session_len=64, quant_policy=bits, cache_blocks=B + 8,
                                   max_prefill_token_num=2 * B, use_graph=0)
    try:
        eng.load_weights(export_weights(cfg, w))
        eng.start()
        eng.prefill([[1 + b % 200, 7] for b in range(B)], max_new_tokens=2)
        got = eng.stats()['decode_splits']
    finally:
        eng.close()
    assert got == _engine_splits(Hq, Hkv, bits, B), (got, _engine_splits(Hq, Hkv, bits, B))


def test_engine_splits_restatement_values(tm):
    """host only: the published geometries' split counts -- decode attention 1 at InternLM2-20B x 128 (1024 workgroups), 4 at one
    Llama-3-70B rank x 64 -- and a split-K w_qkv GEMM at both, so the fused prologue's fp32-slab input runs in the tests below"""
    assert _engine_splits(48, 8, 8, 128) == 1
    assert _engine_splits(8, 1, 4, 64) == 4
    assert _qkv_splits(tm, 6144, (48 + 16) * 128, 128) > 1
    assert _qkv_splits(tm, 8192, (8 + 2) * 128, 64) > 1


@gpu
@pytest.mark.parametrize('Hq,Hkv,bits,B', GEOMETRIES)
def test_decode_attention_published_geometry(tm, cuda, Hq, Hkv, bits, B):
    """B sequences of 1..2047 cached tokens (1, 64, 65 and 2047 included), splits 1 / the engine's / 3 / 16: every sequence
    against the fp64 reference, eight (the four edges + four random) against the oracle's tiled restatement"""
    rng = np.random.default_rng(Hq * 7 + bits)
    layer = 1
    klen = _ragged(rng, B)
    L = o.BlockLayout(2, Hkv, 128, 64, bits)
    oc, tables, total = _random_cache(rng, L, klen)
    _check_seq_kv(oc, tables[3], layer, klen[3])
    q = rng.standard_normal((B, Hq * 128)).astype(f16)
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    klen_d = dev(np.asarray(klen, np.int32))
    check = [0, 1, 2, 3] + rng.choice(np.arange(4, B), 4, replace=False).tolist()
    refs64, refs = _refs(oc, tables, layer, klen, q, Hq, check)
    q_d = dev(q)
    for splits in sorted({1, _engine_splits(Hq, Hkv, bits, B), 3, 16}):
        got = _decode(tm, dc, q_d, Hq * 128, klen_d, B, Hq, splits, layer)
        _check_decode(got, refs64, refs, f'splits {splits}')


def _fused_case(tm, rng, Hq, Hkv, bits, klen):
    """history = random codes; the new token (position klen - 1) of every sequence through (a) kv_rope_store + the plain kernel
    and (b) the fused prologue; the oracle's process_kv writes it into the oracle pool.  Returns what the checks need."""
    B = len(klen)
    L = o.BlockLayout(2, Hkv, 128, 64, bits)
    oc, tables, total = _random_cache(rng, L, klen)
    qkv_n = (Hq + 2 * Hkv) * 128
    p = o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192)
    max_pos = max(klen) + 1
    tab_d = dev(rope_table(tm, max_pos, p))
    klen_d = dev(np.asarray(klen, np.int32))
    cu = dev(np.arange(B + 1, dtype=np.int32))
    return L, oc, tables, total, qkv_n, p, max_pos, tab_d, klen_d, cu


@gpu
@pytest.mark.parametrize('Hq,Hkv,bits,B,hidden', [(48, 8, 8, 128, 6144), (8, 1, 4, 64, 8192)])
def test_decode_attention_fused_published_geometry(tm, cuda, Hq, Hkv, bits, B, hidden):
    """fused prologue at the published geometries, qkv_splits 0 and the engine's qkv split-K, every decode split count of the
    plain test: cache bytes bit exact against the oracle's process_kv, output bit identical to kv_rope_store + the plain
    kernel (the rule of test_gpu_ops.test_decode_attention_fused_prologue), and within the attention tolerance of fp64"""
    rng = np.random.default_rng(Hq + bits + 1)
    layer = 1
    klen = _ragged(rng, B)
    L, oc, tables, total, qkv_n, p, max_pos, tab_d, klen_d, cu = _fused_case(tm, rng, Hq, Hkv, bits, klen)
    pool0 = torch.from_numpy(oc.pool.copy()).cuda()
    hist = [k - 1 for k in klen]
    assert _qkv_splits(tm, hidden, qkv_n, B) > 1
    for qkv_splits in sorted({0, _qkv_splits(tm, hidden, qkv_n, B)}):
        if qkv_splits:
            slabs = (rng.standard_normal((qkv_splits, B, qkv_n)) / np.sqrt(qkv_splits)).astype(np.float32)
            acc = np.zeros((B, qkv_n), np.float32)
            for s_ in slabs:
                acc = acc + s_                      # in-order fp32 sum, like splitk_reduce_kernel
            qkv = acc.astype(f16)
            qkv_in = dev(slabs)
        else:
            qkv = rng.standard_normal((B, qkv_n)).astype(f16)
            qkv_in = dev(qkv.copy())
        ocn = o.PagedKVCache(L, total)
        ocn.pool[:] = oc.pool
        for b in range(B):
            cos, sin = o.rope_cos_sin(p, np.arange(hist[b], hist[b] + 1))
            k = qkv[b:b + 1, Hq * 128:(Hq + Hkv) * 128].reshape(1, Hkv, 128)
            v = qkv[b:b + 1, (Hq + Hkv) * 128:].reshape(1, Hkv, 128)
            o.process_kv(ocn, tables[b], layer, k, v, cos, sin, hist[b])
        q_rope = o.rope_apply(qkv[:, :Hq * 128].reshape(B, Hq, 128), *o.rope_cos_sin(p, np.asarray(hist)))
        check = [0, 1, 2, 3]
        refs64, refs = _refs(ocn, tables, layer, klen, q_rope.reshape(B, Hq * 128), Hq, check)
        dc_a, dc_b = DevCache(L, total, tables), DevCache(L, total, tables)
        for splits in sorted({1, _engine_splits(Hq, Hkv, bits, B), 3, 16}):
            dc_a.pool.copy_(pool0)
            dc_b.pool.copy_(pool0)
            qkv_a = dev(qkv.copy())
            _ffi.check(tm.tm_kv_rope_store(qkv_a.data_ptr(), Hq, cu.data_ptr(), klen_d.data_ptr(), B, B, tab_d.data_ptr(), max_pos,
                                           dc_a.view(layer), st()))
            got_a = _decode(tm, dc_a, qkv_a, qkv_n, klen_d, B, Hq, splits, layer)
            out_b = torch.zeros((B, Hq * 128), dtype=torch.float16, device='cuda')
            ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
            _ffi.check(tm.tm_decode_attention_fused(out_b.data_ptr(), qkv_in.data_ptr(), qkv_splits, qkv_n, tab_d.data_ptr(), max_pos,
                                                    klen_d.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(), dc_b.view(layer), st()))
            what = f'qkv_splits {qkv_splits} splits {splits}'
            assert np.array_equal(dc_a.download(), ocn.pool), f'{what}: kv_rope_store cache bytes'
            pool_b = dc_b.download()
            assert np.array_equal(pool_b, ocn.pool), f'{what}: fused cache bytes differ in {np.count_nonzero(pool_b != ocn.pool)} positions'
            got_b = host(out_b).reshape(B, Hq, 128).astype(np.float32)
            assert np.array_equal(got_a.astype(f16).view(np.uint16), got_b.astype(f16).view(np.uint16)), f'{what}: fused != plain'
            _check_decode(got_b, refs64, refs, what)


# ------------------------------------------------------------------------------------------------
# B. long contexts against the reference
# ------------------------------------------------------------------------------------------------
LONG_KLEN = [1, 65, 4095, 4096, 4097, 8191, 8192]


def _spike(oc, tables, layer, klen, q, Hq):
    """K row of one token past block 64 (position 4096 + (ctx - 4096) // 2: the newest token at ctx 4097, block 95/96 at 8k)
    set to +-1.25 along the sign of the first query head of its group: ~11 above a typical logit for that head, most of its
    softmax mass, arriving after (newest first) dozens of tiles -- the rescale of the running sum and output late in the context"""
    L = oc.layout
    G = Hq // L.kv_heads
    for b, n in enumerate(klen):
        if n <= 4096:
            continue
        t = 4096 + (n - 4096) // 2
        blk = oc.pool[tables[b][t // 64]]
        base = L.layer_offset(layer)
        for hd in range(L.kv_heads):
            sgn = q[b].reshape(Hq, 128)[hd * G].astype(np.float32) > 0
            d0 = base + L.k_data(hd, t % 64)
            if L.bits == 16:
                blk[d0:d0 + 256] = np.where(sgn, f16(1.25), f16(-1.25)).astype(f16).view(np.uint8)
                continue
            qmax = (1 << L.bits) - 1
            codes = np.where(sgn, qmax, 0).astype(np.uint8)
            blk[d0:d0 + L.token_data_size] = codes if L.bits == 8 else o.kv_pack_int4(codes)
            p0 = base + L.k_param(hd, t % 64)
            blk[p0:p0 + 4] = np.array([2.5 / qmax, -1.25], f16).view(np.uint8)     # codes {0, qmax} -> about {-1.25, +1.25}


@gpu
@pytest.mark.parametrize('bits', [8, 4, 16])
def test_decode_attention_long_context(tm, cuda, bits):
    """contexts of 1 .. 8192 tokens (up to 128 blocks: the pointer walk past 64 blocks, per-split tile ranges at large tile counts),
    splits 1 / 4 / 16, ragged and rectangular block tables: every sequence against the fp64 reference and the oracle"""
    rng = np.random.default_rng(100 + bits)
    Hq, Hkv, layer = 16, 2, 1
    klen = LONG_KLEN
    B = len(klen)
    L = o.BlockLayout(2, Hkv, 128, 64, bits)
    oc, tables, total = _random_cache(rng, L, klen)
    q = rng.standard_normal((B, Hq * 128)).astype(f16)
    _spike(oc, tables, layer, klen, q, Hq)
    _check_seq_kv(oc, tables[4], layer, klen[4])
    refs64, refs = _refs(oc, tables, layer, klen, q, Hq, range(B))
    # the spike is where it was aimed: a visible share of the probability mass of at least one head per long sequence
    for b, n in enumerate(klen):
        if n > 4096:
            K, _ = _seq_kv(oc, tables[b], layer, n)
            t = 4096 + (n - 4096) // 2
            s = np.einsum('gd,gtd->gt', q[b].reshape(Hkv, Hq // Hkv, 128)[:, 0].astype(np.float64), K.astype(np.float64)) / math.sqrt(128)
            pm = np.exp(s - s.max(-1, keepdims=True))
            assert (pm[:, t] / pm.sum(-1)).min() > 0.3, f'seq {b}: spike too weak'
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    klen_d = dev(np.asarray(klen, np.int32))
    q_d = dev(q)
    stride = max((k + 63) // 64 for k in klen) + 2
    try:
        for mode in (0, stride):
            dc.set_tables(tables, stride=mode)
            _ffi.check(tm.tm_debug_set_block_stride(mode))
            for splits in (1, 4, 16):
                got = _decode(tm, dc, q_d, Hq * 128, klen_d, B, Hq, splits, layer)
                _check_decode(got, refs64, refs, f'{"rectangular" if mode else "ragged"} table, splits {splits}')
    finally:
        tm.tm_debug_set_block_stride(0)


def _prefill_ref64(q, K, V, hist):
    """causal attention in fp64: q [T, Hq, D], K / V [Hkv, hist + T, D]"""
    T, Hq, D = q.shape
    Hkv, n, _ = K.shape
    G = Hq // Hkv
    out = np.zeros((T, Hq, D))
    mask = np.arange(n)[None, :] > (hist + np.arange(T))[:, None]
    for hq in range(Hq):
        s = (q[:, hq].astype(np.float64) @ K[hq // G].astype(np.float64).T) / math.sqrt(D)
        s[mask] = -np.inf
        pr = np.exp(s - s.max(-1, keepdims=True))
        out[:, hq] = (pr / pr.sum(-1, keepdims=True)) @ V[hq // G].astype(np.float64)
    return out


@gpu
@pytest.mark.parametrize('Hq,Hkv,qlens,hist', [(48, 8, [1024, 700], [0, 324]), (8, 1, [2048], [6144])])
def test_prefill_attention_published_geometry(tm, cuda, Hq, Hkv, qlens, hist):
    """prefill attention at InternLM2-20B's heads (two chunks, one on a 324-token history) and at one Llama-3-70B rank (a
    2048-token chunk on a 6144-token history): every row against fp64, 24 rows per sequence against the oracle"""
    rng = np.random.default_rng(Hq + sum(qlens) + sum(hist))
    B = len(qlens)
    klen = [h + n for h, n in zip(hist, qlens)]
    koff = np.concatenate([[0], np.cumsum([((k + 63) // 64) * 64 for k in klen])]).astype(np.int32)
    stride = int(koff[-1])
    cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    T = int(cu[-1])
    q = rng.standard_normal((T, Hq * 128)).astype(f16)
    K = np.zeros((Hkv, stride, 128), f16)
    Vt = np.zeros((Hkv, 128, stride), f16)
    Ks, Vs = [], []
    for b, n in enumerate(klen):
        k = rng.standard_normal((Hkv, n, 128)).astype(f16)
        v = rng.standard_normal((Hkv, n, 128)).astype(f16)
        K[:, koff[b]:koff[b] + n] = k
        K[:, koff[b] + n:koff[b + 1]] = f16(np.nan)      # garbage past the context must be masked, not multiplied
        Vt[:, :, koff[b]:koff[b] + n] = v.transpose(0, 2, 1)
        Ks.append(k)
        Vs.append(v)
    out = torch.zeros((T, Hq * 128), dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_prefill_attention(out.data_ptr(), dev(q).data_ptr(), Hq * 128, dev(K).data_ptr(), dev(Vt).data_ptr(),
                                       stride, dev(cu).data_ptr(), dev(koff).data_ptr(),
                                       dev(np.asarray(klen, np.int32)).data_ptr(), B, max(qlens), Hq, Hkv, 0.0, st()))
    got = host(out).astype(np.float32)
    for b, n in enumerate(qlens):
        qb = q[cu[b]:cu[b + 1]].reshape(n, Hq, 128)
        g = got[cu[b]:cu[b + 1]].reshape(n, Hq, 128)
        r64 = _prefill_ref64(qb, Ks[b], Vs[b], hist[b])
        err = np.abs(g - r64)
        assert np.all(err <= 1e-2 * np.abs(r64) + 3e-3), f'seq {b}: max err {err.max()} vs fp64'
        rows = np.unique(np.concatenate([[0, 63, 64, n - 1], rng.integers(0, n, 20)]))
        for i in rows:
            ctx = hist[b] + i + 1
            ref = o.decode_attention(qb[i], Ks[b][:, :ctx], Vs[b][:, :ctx], None, 1).astype(np.float32)
            err = np.abs(g[i] - ref)
            assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'seq {b} row {i}: max err {err.max()} vs oracle'


# ------------------------------------------------------------------------------------------------
# C. GQA groups above 16: the MFMA decode kernel splits the group into `chunks` workgroups of hpw heads
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('Hq,Hkv', [(40, 2), (64, 2)])
@pytest.mark.parametrize('bits', [8, 4])
def test_decode_attention_gqa_above_16(tm, cuda, Hq, Hkv, bits):
    """group 20 (2 x 10 heads) and group 32 (2 x 16): plain kernel against fp64 / the oracle, fused prologue bit exact"""
    rng = np.random.default_rng(Hq * 3 + bits)
    layer = 1
    klen = [1, 64, 65, 300, 1000, 2047]
    B = len(klen)
    L, oc, tables, total, qkv_n, p, max_pos, tab_d, klen_d, cu = _fused_case(tm, rng, Hq, Hkv, bits, klen)
    # plain kernel on the random-code history
    q = rng.standard_normal((B, Hq * 128)).astype(f16)
    refs64, refs = _refs(oc, tables, layer, klen, q, Hq, range(B))
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    q_d = dev(q)
    for splits in (1, 3):
        got = _decode(tm, dc, q_d, Hq * 128, klen_d, B, Hq, splits, layer)
        _check_decode(got, refs64, refs, f'plain splits {splits}')
    # fused prologue: the new token of every sequence
    qkv = rng.standard_normal((B, qkv_n)).astype(f16)
    hist = [k - 1 for k in klen]
    for b in range(B):
        cos, sin = o.rope_cos_sin(p, np.arange(hist[b], hist[b] + 1))
        o.process_kv(oc, tables[b], layer, qkv[b:b + 1, Hq * 128:(Hq + Hkv) * 128].reshape(1, Hkv, 128),
                     qkv[b:b + 1, (Hq + Hkv) * 128:].reshape(1, Hkv, 128), cos, sin, hist[b])
    q_rope = o.rope_apply(qkv[:, :Hq * 128].reshape(B, Hq, 128), *o.rope_cos_sin(p, np.asarray(hist))).reshape(B, Hq * 128)
    refs64, refs = _refs(oc, tables, layer, klen, q_rope, Hq, [0, 2, 5])
    for splits in (1, 3):
        dc_a, dc_b = DevCache(L, total, tables), DevCache(L, total, tables)
        dc_a.pool.copy_(dc.pool)
        dc_b.pool.copy_(dc.pool)
        qkv_a = dev(qkv.copy())
        _ffi.check(tm.tm_kv_rope_store(qkv_a.data_ptr(), Hq, cu.data_ptr(), klen_d.data_ptr(), B, B, tab_d.data_ptr(), max_pos,
                                       dc_a.view(layer), st()))
        got_a = _decode(tm, dc_a, qkv_a, qkv_n, klen_d, B, Hq, splits, layer)
        out_b = torch.zeros((B, Hq * 128), dtype=torch.float16, device='cuda')
        ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
        _ffi.check(tm.tm_decode_attention_fused(out_b.data_ptr(), dev(qkv.copy()).data_ptr(), 0, qkv_n, tab_d.data_ptr(), max_pos,
                                                klen_d.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(), dc_b.view(layer), st()))
        assert np.array_equal(dc_a.download(), oc.pool), f'splits {splits}: kv_rope_store cache bytes'
        assert np.array_equal(dc_b.download(), oc.pool), f'splits {splits}: fused cache bytes'
        got_b = host(out_b).reshape(B, Hq, 128).astype(np.float32)
        assert np.array_equal(got_a.astype(f16).view(np.uint16), got_b.astype(f16).view(np.uint16)), f'splits {splits}: fused != plain'
        _check_decode(got_b, refs64, refs, f'fused splits {splits}')


# ------------------------------------------------------------------------------------------------
# D / E. MoE at Mixtral's width, every grouped row tile, skewed routings
# ------------------------------------------------------------------------------------------------
E_MOE, TOPK = 8, 2
_E4M3 = o.fp8_e4m3_to_f32(np.arange(256, dtype=np.uint8))          # code -> value (exact, NaN at 0x7F / 0xFF)
_E4M3_RMS = float(np.sqrt(np.mean(np.delete(_E4M3, [0x7F, 0xFF]) ** 2)))


def _moe_gate(rng, H):
    """the first 8 channels of x are the router logits (identity rows) plus a little of the rest: x decides the routing"""
    gate = (rng.standard_normal((H, E_MOE)) * 0.002).astype(f16)
    gate[:E_MOE] = np.eye(E_MOE, dtype=f16)
    return gate


def _moe_x(rng, T, H, kind):
    """x [T, H] and the expert histogram `kind` aims for:
    'random': any; 'one': expert 3 takes every token, experts 0 / 6 the second choices, the other five nothing;
    'edge': expert 1 exactly 2 * hint rows and expert 2 2 * hint + 1 (hint = ceil(T * top_k / E), the launchers' expected rows
    per expert: their row tile is sized for 2 * hint), the second choices spread over the other six"""
    x = rng.standard_normal((T, H)).astype(f16)
    if kind == 'random':
        return x, None
    x[:, :E_MOE] = rng.uniform(-1.0, 0.0, (T, E_MOE)).astype(f16)
    picks = [[] for _ in range(T)]
    if kind == 'one':
        for t in range(T):
            picks[t] = [3, (0, 6)[t % 2]]
    else:
        a = 2 * ((T * TOPK + E_MOE - 1) // E_MOE)
        assert 2 * a + 1 <= 2 * T
        for t in range(a):
            picks[t].append(1)
        for t in range(T - a - 1, T):
            picks[t].append(2)
        others = [0, 3, 4, 5, 6, 7]
        i = 0
        for t in range(T):
            while len(picks[t]) < TOPK:
                picks[t].append(others[i % len(others)])
                i += 1
    hist = np.zeros(E_MOE, np.int64)
    for t, (first, second) in enumerate(picks):
        x[t, first], x[t, second] = f16(3.0), f16(2.0)
        hist[[first, second]] += 1
    if kind == 'edge':
        assert hist[1] == a and hist[2] == a + 1
    return x, hist


def _fp8_expert(rng, K, N, std):
    """random e4m3 codes (never the NaN codes 0x7F / 0xFF), random fp32 128 x 128 block scales for entries of about `std`"""
    c = rng.integers(0, 254, (K, N), dtype=np.uint8)
    c += (c >= 0x7F).astype(np.uint8)
    s = (rng.uniform(0.5, 1.5, (K // 128, N // 128)) * std / _E4M3_RMS).astype(np.float32)
    return c, s


def _u4_expert(rng, K, N, std):
    """random u4 codes, fp16 scales, integer zero points; the packed boundary layout and the dequantised fp16 weights
    (the closed form of test_gpu_fullsize._random_awq, checked against o.w4a16_dequant at small size)"""
    q = rng.integers(0, 16, (K, N), dtype=np.uint8)
    s = (rng.uniform(0.5, 1.5, (K // 128, N)) * std / 5.0).astype(f16)
    z = rng.integers(4, 12, (K // 128, N)).astype(f16)
    packed = (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8).view('<i4')
    zs = ((-z.astype(np.float32)) * s.astype(np.float32)).astype(f16).astype(np.float32)
    wd = (q.reshape(K // 128, 128, N).astype(np.float32) * s.astype(np.float32)[:, None, :] + zs[:, None, :]).astype(f16)
    return packed, s, z, wd.reshape(K, N), q


def _fp8_act_linear(x, wf, sw, gated):
    """o.fp8_act_linear with the weight codes already decoded (wf = e4m3 values fp32, sw = o.fp8_block_scales_f32)"""
    xq, sx = o.fp8_quant_rows(x)
    a = _E4M3[xq]
    acc = np.zeros((a.shape[0], wf.shape[1]), np.float32)
    for g in range(wf.shape[0] // 128):
        acc += (a[:, g * 128:(g + 1) * 128] @ wf[g * 128:(g + 1) * 128]) * (sx[g][:, None] * sw[g][None, :])
    return o.gated_silu_epilogue(acc) if gated else acc.astype(f16)


def _expert_ffn(kind, wts, x):
    """one expert's FFN on the rows x, in the arithmetic of o.moe_ffn_fp8 ('fp8') / o.moe_ffn ('fp8wo', 'u4')"""
    if kind == 'fp8':
        (q13, s13), (q2, s2) = wts
        H, N13 = q13.shape
        act = _fp8_act_linear(x, _E4M3[q13], o.fp8_block_scales_f32(s13, H, N13, True), True)
        return _fp8_act_linear(act, _E4M3[q2], o.fp8_block_scales_f32(s2, q2.shape[0], q2.shape[1], False), False)
    w13, w2 = wts                                  # dequantised fp16
    act = o.gated_silu_epilogue(o.gemm_f16_f32acc(x, w13))
    return o.gemm_f16_f32acc(act, w2).astype(f16)


def _fp8_wo_dense(q, s, gated):
    """o.fp8_dequant with the code table: h(f16(e4m3) * s)"""
    K, N = q.shape
    sc = o.fp8_expand_block_scales(s, K, N, gated)
    return o.hmul(_E4M3[q].astype(f16), np.repeat(sc, 128, axis=0))


class _MoeCase:
    """the x of every case, its routing (o.moe_gate) and the oracle output accumulated expert by expert"""

    def __init__(self, gate, xs, kinds):
        self.xs = xs
        self.ids, self.w = [], []
        for x in xs:
            _, ids, w = o.moe_gate(x, gate, TOPK)
            self.ids.append(ids)
            self.w.append(w)
        self.y = {k: [np.zeros((len(x), TOPK, x.shape[1]), np.float32) for x in xs] for k in kinds}

    def add_expert(self, e, kind, wts, rowwise=False):
        """rowwise: one row per product, the oracle's own order (o.moe_ffn* run token by token) -- bit exact with it"""
        rows = [np.nonzero(ids == e) for ids in self.ids]
        xe = np.concatenate([x[r[0]] for x, r in zip(self.xs, rows)])
        if len(xe) == 0:
            return
        if rowwise:
            ye = np.concatenate([_expert_ffn(kind, wts, xe[i:i + 1]) for i in range(len(xe))]).astype(np.float32)
        else:
            ye = _expert_ffn(kind, wts, xe).astype(np.float32)
        off = 0
        for c, (t, j) in enumerate(rows):
            self.y[kind][c][t, j] = ye[off:off + len(t)]
            off += len(t)

    def ref(self, kind, c):
        """out[t] = fp16(sum_j w[t, j] * y_j) accumulated in fp32 in the order of j (o.moe_ffn's combine)"""
        out = np.zeros(self.y[kind][c].shape[::2], np.float32)
        for j in range(TOPK):
            out += self.w[c][:, j:j + 1] * self.y[kind][c][:, j]
        return out.astype(f16)


def _moe_run(tm, h, x, rows):
    T, H = x.shape
    ws = torch.full((tm.tm_moe_workspace(h, T),), 0xFF, dtype=torch.uint8, device='cuda')   # NaN in every unwritten fp16
    out = torch.zeros((T, H), dtype=torch.float16, device='cuda')
    ids = torch.zeros((T, TOPK), dtype=torch.int32, device='cuda')
    w = torch.zeros((T, TOPK), dtype=torch.float32, device='cuda')
    _ffi.check(tm.tm_debug_set_grouped_rows(rows))
    try:
        _ffi.check(tm.tm_moe_forward(h, out.data_ptr(), dev(x).data_ptr(), T, ws.data_ptr(), ids.data_ptr(), w.data_ptr(), st()))
        torch.cuda.synchronize()
    finally:
        tm.tm_debug_set_grouped_rows(0)
    return host(out).astype(np.float32), host(ids), host(w)


def _moe_check(tm, kind, h, case, labels, hists):
    """every (forced row tile, case): ids equal, weights within 1e-5, output within test_moe_ffn's tolerance -- a tolerance the
    zero output and 3/4 of the reference would both fail"""
    for c, x in enumerate(case.xs):
        if hists[c] is not None:
            got_hist = np.bincount(case.ids[c].ravel(), minlength=E_MOE)
            assert np.array_equal(got_hist, hists[c]), f'{labels[c]}: routing histogram {got_hist} is not the one aimed for {hists[c]}'
        ref = case.ref(kind, c).astype(np.float32)
        tol = (4e-3 + 2.0**-6 * np.abs(ref)) if kind == 'fp8' else (3e-3 + 2.0**-8 * np.abs(ref))
        assert np.any(np.abs(ref) > tol) and np.any(0.25 * np.abs(ref) > tol), f'{kind} {labels[c]}: outputs too small to test'
        # u4 / fp8 weight-only take a forced tile in decode-sized forwards only (tokens <= 64; larger ones run the prefill tile)
        tiles = TILES[kind] if kind == 'fp8' or len(x) <= 64 else (0,)
        worst = 0.0
        for rows in tiles:
            out, ids, w = _moe_run(tm, h, x, rows)
            what = f'{kind} {labels[c]} rows {rows or "auto"}'
            assert np.array_equal(ids, case.ids[c]), f'{what}: routing differs'
            assert np.abs(w - case.w[c]).max() <= 1e-5, what
            err = np.abs(out - ref)
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), f'{what}: max err {err.max()} at {np.unravel_index(np.argmax(err - tol), err.shape)}'
        print(f'{kind} {labels[c]}: |ref| max {np.abs(ref).max():.4f}, worst err / tol {worst:.3f}')


TILES = {'u4': (0, 16, 32, 64), 'fp8wo': (0, 16, 32, 64), 'fp8': (0, 32, 64)}


def _moe_block(tm, monkeypatch, H, I, wtype, cases, seed, pin=False):
    """one MoE block per expert format (fp8: on the matrix cores AND weight-only, the same codes), experts drawn one at a time
    (uploaded, their rows of every case computed, dropped), then every case through every row tile"""
    rng = np.random.default_rng(seed)
    gate = _moe_gate(rng, H)
    xs, hists, labels = [], [], []
    for kind, T in cases:
        x, hist = _moe_x(rng, T, H, kind)
        xs.append(x)
        hists.append(hist)
        labels.append(f'{kind} T={T}')
    kinds = ('fp8', 'fp8wo') if wtype == 'fp8' else ('u4',)
    case = _MoeCase(gate, xs, kinds)
    handles = {}
    for kind in kinds:
        h = _ffi.C.c_void_p()
        _ffi.check(tm.tm_moe_create(_ffi.C.byref(h), H, I, E_MOE, TOPK, 2 if wtype == 'fp8' else 0, 1, 1.0))
        _ffi.check(tm.tm_moe_set_gate(h, dev(gate).data_ptr(), st()))
        handles[kind] = h
    # gated-SiLU rows of about unit size.  Outputs: u4 about 1; e4m3 (both paths share the codes) up to about 0.3 at Mixtral
    # width and 0.2 at H 256.  The fp8 matrix-core path re-quantises the gated-SiLU rows to e4m3: about a fifth of the device's
    # fp16 entries differ from the oracle's by an ulp (fp32 accumulation order, SiLU), which moves 0.5 % of the codes and 6 % of
    # the row-group scales; through random e4m3 down-projection codes that alone is 2.5 % (I 14336) .. 3.7 % (I 384) of the
    # output rms (the oracle's own down projection of the device's rows against its rows, measured on MI355X).  A fixed
    # fraction of the output: test_moe_ffn's 4e-3 + 2^-6 |ref| holds below outputs of this size, and _moe_check asserts that it
    # still rejects a zero output and 3/4 of the reference.
    s13_std, s2_std = (1.5, 0.05 if I > 1024 else 0.02) if wtype == 'fp8' else (1.5, 1.0)
    small = []
    try:
        for e in range(E_MOE):
            if wtype == 'fp8':
                q13, s13 = _fp8_expert(rng, H, 2 * I, s13_std / math.sqrt(H))
                q2, s2 = _fp8_expert(rng, I, H, s2_std / math.sqrt(I))
                for kind in kinds:
                    _ffi.check(tm.tm_moe_set_expert(handles[kind], e, dev(q13).data_ptr(), dev(s13).data_ptr(), None,
                                                    dev(q2).data_ptr(), dev(s2).data_ptr(), None, st()))
                case.add_expert(e, 'fp8', ((q13, s13), (q2, s2)), pin)
                dense = (_fp8_wo_dense(q13, s13, True), _fp8_wo_dense(q2, s2, False))
                case.add_expert(e, 'fp8wo', dense, pin)
                if pin:
                    assert np.array_equal(dense[0].view(np.uint16), o.fp8_dequant(q13, s13, gated=True).view(np.uint16))
                    small.append((((q13, s13), (q2, s2)), dense))
            else:
                p13, s13, z13, w13, qq13 = _u4_expert(rng, H, 2 * I, 1.5 / math.sqrt(H))
                p2, s2, z2, w2, _ = _u4_expert(rng, I, H, 1.0 / math.sqrt(I))
                _ffi.check(tm.tm_moe_set_expert(handles['u4'], e, dev(p13).data_ptr(), dev(s13).data_ptr(), dev(z13).data_ptr(),
                                                dev(p2).data_ptr(), dev(s2).data_ptr(), dev(z2).data_ptr(), st()))
                case.add_expert(e, 'u4', (w13, w2), pin)
                if pin:
                    assert np.array_equal(o.unpack_u4_row(p13), qq13)
                    assert np.array_equal(w13.view(np.uint16), o.w4a16_dequant(qq13, s13, z13).view(np.uint16))
                    small.append((None, (w13, w2)))
            torch.cuda.synchronize()
            from tests import gpu_helpers
            gpu_helpers.release_all()                 # one expert's host-side upload buffers at a time
        if pin:     # the expert-by-expert restatement == the oracle's token-by-token moe_ffn / moe_ffn_fp8
            for c, x in enumerate(xs):
                if wtype == 'fp8':
                    r, _, _ = o.moe_ffn_fp8(x, gate, [s[0] for s in small], TOPK)
                    assert np.array_equal(case.ref('fp8', c).view(np.uint16), r.view(np.uint16)), labels[c]
                r, _, _ = o.moe_ffn(x, gate, [s[1] for s in small], TOPK)
                assert np.array_equal(case.ref('fp8wo' if wtype == 'fp8' else 'u4', c).view(np.uint16), r.view(np.uint16)), labels[c]
        for kind in kinds:     # fp8 first: the weight-only block then takes its path at its first forward (moe_prepare)
            if kind == 'fp8wo':
                monkeypatch.setenv('TM_FP8_MFMA', '0')
            _moe_check(tm, kind, handles[kind], case, labels, hists)
    finally:
        for h in handles.values():
            tm.tm_moe_destroy(h)


SKEWED = [('one', 64), ('one', 300), ('edge', 64), ('edge', 300)]


@gpu
@pytest.mark.parametrize('wtype', ['fp8', 'u4'])
def test_moe_skewed_routing_small(tm, cuda, monkeypatch, wtype):
    """test_moe_ffn's size (H 256, I 384): routings that give one expert every token and leave five empty, and experts with
    exactly 2 * hint and 2 * hint + 1 rows (a segment that ends on the launchers' tile boundary, one that overflows it),
    every row tile; the expert-by-expert oracle restatement is pinned here on o.moe_ffn_fp8 / o.moe_ffn"""
    _moe_block(tm, monkeypatch, 256, 384, wtype, [('random', 37)] + SKEWED, seed=5, pin=True)


@gpu
@pytest.mark.parametrize('I', [14336, 7168])
@pytest.mark.parametrize('wtype', ['fp8', 'u4'])
def test_moe_mixtral_size(tm, cuda, monkeypatch, wtype, I):
    """Mixtral-8x7B's MoE block (H 4096, I 14336; 7168 = one TP = 2 rank), 8 experts, top-2, e4m3 experts on the matrix cores
    and weight-only, u4 experts: T = 1 / 64 / 300 with the router's own routing plus the skewed routings, every row tile"""
    _moe_block(tm, monkeypatch, 4096, I, wtype, [('random', 1), ('random', 64), ('random', 300)] + SKEWED, seed=I + len(wtype))
