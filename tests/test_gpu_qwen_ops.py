"""GPU parity of the Qwen attention prologue (per-head q / k RMSNorm -> q / k / v bias -> RoPE) in its two kernels:
tm_kv_rope_store_qk (prefill, fp16-KV decode, TM_FUSE_QKV=0 / TM_ATTN_VALU=1) and tm_decode_attention_fused_qk (the fused
int8 / int4 decode path).  q / k / v after the prologue and the cache bytes are bit exact against the oracle restatement
written in the kernels' fp32 summation order (tests.qwen_reference.head_norm_kernel_order, itself within 1 ulp of
o.rmsnorm); with no prologue tensor the new entry points are byte-identical to the existing ones."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.gpu_helpers import DevCache, dev, host, rope_table, st, ulp_diff_f16
from tests.qwen_reference import head_norm, head_norm_kernel_order, prologue

pytestmark = pytest.mark.gpu
f16 = np.float16
EPS = 1e-6


def _tensors(rng, Hq, Hkv, mode):
    Lw = {}
    if mode in ('bias', 'both'):
        Lw['qkv_bias'] = (0.5 * rng.standard_normal((Hq + 2 * Hkv) * 128)).astype(f16)
    if mode in ('norm', 'both'):
        Lw['q_norm'] = (1 + 0.05 * rng.standard_normal(128)).astype(f16)
        Lw['k_norm'] = (1 + 0.05 * rng.standard_normal(128)).astype(f16)
    return Lw


def _ptrs(Lw):
    return tuple(dev(Lw[k]).data_ptr() if k in Lw else None for k in ('qkv_bias', 'q_norm', 'k_norm'))


def test_kernel_order_norm_is_within_one_ulp_of_oracle():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((64, 8, 128)) * 3).astype(f16)
    w = (1 + 0.05 * rng.standard_normal(128)).astype(f16)
    d = ulp_diff_f16(head_norm_kernel_order(x, w, EPS), head_norm(x, w, EPS))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3


@pytest.mark.parametrize('mode', ['none', 'bias', 'norm', 'both'])
@pytest.mark.parametrize('bits', [16, 8, 4])
def test_kv_rope_store_qk(tm, cuda, bits, mode):
    rng = np.random.default_rng(bits * 7 + len(mode))
    Hq, Hkv, layer = 7, 1, 1
    lens_new, hist = [70, 1, 5], [0, 63, 200]
    L = o.BlockLayout(2, Hkv, 128, 64, bits)
    klen = [h + n for h, n in zip(hist, lens_new)]
    nblk = [(k + 63) // 64 for k in klen]
    total = sum(nblk) + 3
    perm = rng.permutation(total)
    tables = [perm[sum(nblk[:b]):sum(nblk[:b + 1])] for b in range(len(nblk))]
    T = sum(lens_new)
    qkv = (rng.standard_normal((T, (Hq + 2 * Hkv) * 128)) * 1.5).astype(f16)
    Lw = _tensors(rng, Hq, Hkv, mode)
    p = o.RopeParam(128, 1e6)
    max_pos = max(klen) + 1
    tab = rope_table(tm, max_pos, p)
    cu = np.concatenate([[0], np.cumsum(lens_new)]).astype(np.int32)
    oc = o.PagedKVCache(L, total)
    q_ref = np.zeros((T, Hq, 128), f16)
    for b, n in enumerate(lens_new):
        sl = slice(cu[b], cu[b + 1])
        cos, sin = o.rope_cos_sin(p, np.arange(hist[b], hist[b] + n))
        q, k, v = prologue(qkv[sl, :Hq * 128].reshape(n, Hq, 128), qkv[sl, Hq * 128:(Hq + Hkv) * 128].reshape(n, Hkv, 128),
                           qkv[sl, (Hq + Hkv) * 128:].reshape(n, Hkv, 128), Lw, EPS, norm=head_norm_kernel_order)
        q_ref[sl] = o.rope_apply(q, cos, sin)
        o.process_kv(oc, tables[b], layer, k, v, cos, sin, hist[b])
    cu_d, kl_d, tab_d = dev(cu), dev(np.asarray(klen, np.int32)), dev(tab)
    dc = DevCache(L, total, tables)
    qkv_d = dev(qkv.copy())
    _ffi.check(tm.tm_kv_rope_store_qk(qkv_d.data_ptr(), Hq, cu_d.data_ptr(), kl_d.data_ptr(), len(lens_new), T, tab_d.data_ptr(),
                                      max_pos, *_ptrs(Lw), EPS, dc.view(layer), st()))
    got = dc.download()
    assert np.array_equal(got, oc.pool), f'cache bytes differ in {np.count_nonzero(got != oc.pool)} positions'
    q_got = host(qkv_d)[:, :Hq * 128].reshape(T, Hq, 128)
    assert np.array_equal(q_got.view(np.uint16), q_ref.view(np.uint16)), 'q after the prologue + RoPE must be bit exact'
    dc2 = DevCache(L, total, tables)
    qkv2 = dev(qkv.copy())
    _ffi.check(tm.tm_kv_rope_store(qkv2.data_ptr(), Hq, cu_d.data_ptr(), kl_d.data_ptr(), len(lens_new), T, tab_d.data_ptr(),
                                   max_pos, dc2.view(layer), st()))
    same = np.array_equal(dc2.download(), got) and np.array_equal(host(qkv2), host(qkv_d))
    assert same == (mode == 'none')     # byte-identical to the existing entry point without a prologue tensor, different with one


@pytest.mark.parametrize('mode', ['bias', 'norm', 'both'])
@pytest.mark.parametrize('bits,Hq,Hkv,klen,splits,qkv_splits', [
    (8, 28, 4, [1, 64, 200], 1, 0),
    (8, 28, 4, [65, 130], 2, 1),
    (4, 28, 4, [300, 7], 4, 2),
    (8, 32, 8, [129, 1000], 4, 4),
    (4, 32, 8, [64, 33, 511], 1, 0),
])
def test_decode_attention_fused_qk(tm, cuda, mode, bits, Hq, Hkv, klen, splits, qkv_splits):
    """Fused prologue with bias / norm == tm_kv_rope_store_qk + tm_decode_attention on the same input: new token's cache bytes bit
    exact against the oracle (process_kv of the transformed K / V), output bit-identical to the unfused device sequence and within the
    decode-attention bound of the oracle."""
    rng = np.random.default_rng(Hq + sum(klen) + splits + qkv_splits + len(mode))
    layer = 1
    L = o.BlockLayout(2, Hkv, 128, 64, bits)
    B = len(klen)
    hist = [k - 1 for k in klen]
    nblk = [(k + 63) // 64 for k in klen]
    total = sum(nblk) + 2
    perm = rng.permutation(total)
    tables = [perm[sum(nblk[:b]):sum(nblk[:b + 1])] for b in range(B)]
    oc = o.PagedKVCache(L, total)
    for b, n in enumerate(hist):
        if n:
            o.process_kv(oc, tables[b], layer, rng.standard_normal((n, Hkv, 128)).astype(f16),
                         rng.standard_normal((n, Hkv, 128)).astype(f16), None, None, 0)
    qkv_n = (Hq + 2 * Hkv) * 128
    if qkv_splits:
        slabs = (rng.standard_normal((qkv_splits, B, qkv_n)) / np.sqrt(qkv_splits)).astype(np.float32)
        acc = np.zeros((B, qkv_n), np.float32)
        for s_ in slabs:
            acc = acc + s_
        qkv = acc.astype(f16)
        qkv_in = dev(slabs)
    else:
        qkv = rng.standard_normal((B, qkv_n)).astype(f16)
        qkv_in = dev(qkv.copy())
    Lw = _tensors(rng, Hq, Hkv, mode)
    ptrs = _ptrs(Lw)
    p = o.RopeParam(128, 1e6)
    max_pos = max(klen) + 1
    tab_d = dev(rope_table(tm, max_pos, p))
    klen_d = dev(np.asarray(klen, np.int32))
    cu = dev(np.arange(B + 1, dtype=np.int32))

    dc_a = DevCache(L, total, tables)
    dc_a.upload(oc)
    qkv_a = dev(qkv.copy())
    _ffi.check(tm.tm_kv_rope_store_qk(qkv_a.data_ptr(), Hq, cu.data_ptr(), klen_d.data_ptr(), B, B, tab_d.data_ptr(), max_pos, *ptrs,
                                      EPS, dc_a.view(layer), st()))
    out_a = torch.zeros((B, Hq * 128), dtype=torch.float16, device='cuda')
    ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
    _ffi.check(tm.tm_decode_attention(out_a.data_ptr(), qkv_a.data_ptr(), qkv_n, klen_d.data_ptr(), B, Hq, 0.0, splits, ws.data_ptr(),
                                      dc_a.view(layer), st()))
    dc_b = DevCache(L, total, tables)
    dc_b.upload(oc)
    out_b = torch.zeros((B, Hq * 128), dtype=torch.float16, device='cuda')
    ws_b = torch.zeros_like(ws)
    _ffi.check(tm.tm_decode_attention_fused_qk(out_b.data_ptr(), qkv_in.data_ptr(), qkv_splits, qkv_n, tab_d.data_ptr(), max_pos,
                                               *ptrs, EPS, klen_d.data_ptr(), B, Hq, 0.0, splits, ws_b.data_ptr(), dc_b.view(layer), st()))
    qs = []
    for b in range(B):
        cos, sin = o.rope_cos_sin(p, np.arange(hist[b], hist[b] + 1))
        q, k, v = prologue(qkv[b:b + 1, :Hq * 128].reshape(1, Hq, 128), qkv[b:b + 1, Hq * 128:(Hq + Hkv) * 128].reshape(1, Hkv, 128),
                           qkv[b:b + 1, (Hq + Hkv) * 128:].reshape(1, Hkv, 128), Lw, EPS, norm=head_norm_kernel_order)
        qs.append(o.rope_apply(q, cos, sin)[0])
        o.process_kv(oc, tables[b], layer, k, v, cos, sin, hist[b])
    pool_a, pool_b = dc_a.download(), dc_b.download()
    assert np.array_equal(pool_a, oc.pool), f'kv_rope_store_qk cache bytes differ in {np.count_nonzero(pool_a != oc.pool)} positions'
    assert np.array_equal(pool_b, oc.pool), f'fused cache bytes differ in {np.count_nonzero(pool_b != oc.pool)} positions'
    ga, gb = host(out_a), host(out_b)
    assert np.array_equal(ga.view(np.uint16), gb.view(np.uint16)), f'max diff {np.abs(ga.astype(np.float32) - gb.astype(np.float32)).max()}'
    for b in range(B):
        kv = [oc.load_dequant(tables[b], layer, hd, 0, klen[b], 'decode') for hd in range(Hkv)]
        ref = o.decode_attention(qs[b], np.stack([a for a, _ in kv]), np.stack([c for _, c in kv]), 1 / np.sqrt(128.0), 1)
        ref = ref.reshape(-1).astype(np.float32)
        assert np.all(np.abs(gb[b].astype(np.float32) - ref) <= 1e-2 * np.abs(ref) + 2e-3)

