"""head_dim 64 (Llama-3.2-1B class models) on the GPU: the four attention / KV-cache kernels through the C-ABI against the oracle
with BlockLayout(head_dim=64), then whole engines (synthetic weights, a Qwen-style qkv bias, chunked prefill, mixed
continuous-batching steps, fabricated checkpoints through pipeline(path)) against OracleModel.

Bounds are the project's own: cache bytes and RoPE(q) bit exact, flatten bit exact (tests/test_gpu_ops.py), attention
err <= 1e-2 |ref| + 2e-3 (test_decode_attention / test_prefill_attention), engine logits <= 3e-2 at every step and greedy tokens equal
where the oracle's top-2 margin exceeds 6e-2 (tests/test_gpu_engine.py::test_engine_matches_oracle)."""
import json
import os

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests.gpu_helpers import DevCache, dev, host, rope_table, st
from tests.qwen_reference import QwenConfig, QwenOracleModel, hf_qwen_tensors, make_qwen_weights, prologue, tm_weights_from_hf

pytestmark = pytest.mark.gpu
f16 = np.float16
D = 64
ROPE = o.RopeParam(64, 500000.0, 'llama3', 32.0, 1.0, 4.0, 8192)     # Llama-3.2-1B


def _tables(rng, klen, spare=3):
    nblk = [(k + 63) // 64 for k in klen]
    total = sum(nblk) + spare
    perm = rng.permutation(total)            # shuffled block tables
    tables, off = [], 0
    for nb in nblk:
        tables.append(perm[off:off + nb])
        off += nb
    return tables, total


# ---- kv_rope_store ---------------------------------------------------------------------------------------------------------------
LENS_NEW, HIST = (1, 17, 70), (0, 63, 5)     # 88 tokens: the third workgroup of 32 token rows is not full; positions cross block ends


def _store_case(bits, seed):
    rng = np.random.default_rng(seed)
    Hq, Hkv = 3, 2
    L = o.BlockLayout(2, Hkv, D, 64, bits)
    klen = [h + n for h, n in zip(HIST, LENS_NEW)]
    tables, total = _tables(rng, klen)
    qkv = (rng.standard_normal((sum(LENS_NEW), (Hq + 2 * Hkv) * D)) * 1.5).astype(f16)
    qkv[1, Hq * D:(Hq + 1) * D] = f16(0.75)              # a constant K row (scale 0)
    qkv[2, (Hq + Hkv) * D + 5] = f16(300.0)              # a V row with an outlier
    return rng, Hq, Hkv, L, klen, tables, total, qkv


def _store_reference(L, total, tables, qkv, Hq, Hkv, layer, cos_sin_of, Lw):
    """oracle cache pool + rotated q; cos_sin_of(b, positions) -> (cos, sin) or (None, None)"""
    oc = o.PagedKVCache(L, total)
    cu = np.concatenate([[0], np.cumsum(LENS_NEW)]).astype(np.int32)
    q_ref = np.zeros((len(qkv), Hq, D), f16)
    for b, n in enumerate(LENS_NEW):
        sl = slice(cu[b], cu[b + 1])
        cos, sin = cos_sin_of(b, np.arange(HIST[b], HIST[b] + n))
        q, k, v = prologue(qkv[sl, :Hq * D].reshape(n, Hq, D), qkv[sl, Hq * D:(Hq + Hkv) * D].reshape(n, Hkv, D),
                           qkv[sl, (Hq + Hkv) * D:].reshape(n, Hkv, D), Lw, 0.0)
        q_ref[sl] = o.rope_apply(q, cos, sin) if cos is not None else q
        o.process_kv(oc, tables[b], layer, k, v, cos, sin, HIST[b])
    return oc, cu, q_ref


def _assert_store(dc, qkv_d, oc, q_ref, Hq):
    got = dc.download()
    assert np.array_equal(got, oc.pool), f'cache bytes differ in {np.count_nonzero(got != oc.pool)} positions'
    q_got = host(qkv_d)[:, :Hq * D].reshape(-1, Hq, D)
    assert np.array_equal(q_got.view(np.uint16), q_ref.view(np.uint16)), 'RoPE(q) must be bit exact'


@pytest.mark.parametrize('bias', [0, 1])
@pytest.mark.parametrize('bits', [16, 8, 4])
def test_kv_rope_store_bit_exact(tm, cuda, bits, bias):
    layer = 1
    rng, Hq, Hkv, L, klen, tables, total, qkv = _store_case(bits, 10 * bits + bias)
    Lw = {'qkv_bias': (0.1 * rng.standard_normal((Hq + 2 * Hkv) * D)).astype(f16)} if bias else {}
    max_pos = max(klen) + 1
    tab = rope_table(tm, max_pos, ROPE)
    oc, cu, q_ref = _store_reference(L, total, tables, qkv, Hq, Hkv, layer, lambda b, pos: o.rope_cos_sin(ROPE, pos), Lw)
    dc = DevCache(L, total, tables)
    qkv_d = dev(qkv)
    args = (Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), len(LENS_NEW), len(qkv), dev(tab).data_ptr(), max_pos)
    if bias:
        _ffi.check(tm.tm_kv_rope_store_qk(qkv_d.data_ptr(), *args, dev(Lw['qkv_bias']).data_ptr(), None, None, 0.0, dc.view(layer), st()))
    else:
        _ffi.check(tm.tm_kv_rope_store(qkv_d.data_ptr(), *args, dc.view(layer), st()))
    _assert_store(dc, qkv_d, oc, q_ref, Hq)


def test_kv_rope_store_without_table(tm, cuda):
    """cos_sin = NULL: no rotation, q untouched"""
    layer = 0
    rng, Hq, Hkv, L, klen, tables, total, qkv = _store_case(8, 77)
    oc, cu, q_ref = _store_reference(L, total, tables, qkv, Hq, Hkv, layer, lambda b, pos: (None, None), {})
    dc = DevCache(L, total, tables)
    qkv_d = dev(qkv)
    _ffi.check(tm.tm_kv_rope_store(qkv_d.data_ptr(), Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), len(LENS_NEW),
                                   len(qkv), None, 0, dc.view(layer), st()))
    _assert_store(dc, qkv_d, oc, q_ref, Hq)


def test_kv_rope_store_per_sequence_tables(tm, cuda):
    """tm_kv_rope_store_seq: three regions of max_pos rows of 32 pairs, one base each; the last sequence clamps inside its own"""
    layer, max_pos = 1, 72                   # sequence 2 ends at position 74: rows 72, 73, 74 clamp to 71
    rng, Hq, Hkv, L, klen, tables, total, qkv = _store_case(4, 78)
    row0 = np.array([max_pos, 0, 2 * max_pos], np.int32)
    bases = {0: 10000.0, max_pos: 37646.7734375, 2 * max_pos: 1e6}
    tab = np.concatenate([rope_table(tm, max_pos, o.RopeParam(64, bases[r])) for r in (0, max_pos, 2 * max_pos)])
    assert tab.shape == (3 * max_pos, 32, 2)
    oc, cu, q_ref = _store_reference(L, total, tables, qkv, Hq, Hkv, layer,
                                     lambda b, pos: o.rope_cos_sin(o.RopeParam(64, bases[int(row0[b])]), np.minimum(pos, max_pos - 1)), {})
    dc = DevCache(L, total, tables)
    qkv_d = dev(qkv)
    _ffi.check(tm.tm_kv_rope_store_seq(qkv_d.data_ptr(), Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), len(LENS_NEW),
                                       len(qkv), dev(tab).data_ptr(), max_pos, dev(row0).data_ptr(), None, None, None, 0.0,
                                       dc.view(layer), st()))
    _assert_store(dc, qkv_d, oc, q_ref, Hq)


def test_kv_rope_store_refuses_qk_norm(tm, cuda):
    rng, Hq, Hkv, L, klen, tables, total, qkv = _store_case(8, 79)
    dc = DevCache(L, total, tables)
    w = dev(np.ones(D, f16))
    cu = np.concatenate([[0], np.cumsum(LENS_NEW)]).astype(np.int32)
    rc = tm.tm_kv_rope_store_qk(dev(qkv).data_ptr(), Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), len(LENS_NEW),
                                len(qkv), None, 0, None, w.data_ptr(), w.data_ptr(), 1e-6, dc.view(0), st())
    assert rc == 1 and 'head_dim' in _ffi.last_error()
    assert not dc.download().any()


# ---- flatten_kv ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('transpose_v', [0, 1])
@pytest.mark.parametrize('bits', [16, 8, 4])
def test_flatten_kv_bit_exact(tm, cuda, bits, transpose_v):
    rng = np.random.default_rng(bits * 2 + transpose_v)
    Hkv, layer = 2, 1
    klen = [1, 64, 65, 130]
    L = o.BlockLayout(2, Hkv, D, 64, bits)
    tables, total = _tables(rng, klen)
    oc = o.PagedKVCache(L, total)
    for b, n in enumerate(klen):
        o.process_kv(oc, tables[b], layer, rng.standard_normal((n, Hkv, D)).astype(f16), rng.standard_normal((n, Hkv, D)).astype(f16),
                     None, None, 0)
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    pad = [(k + 63) // 64 * 64 for k in klen]
    koff = np.concatenate([[0], np.cumsum(pad)]).astype(np.int32)
    stride = int(koff[-1]) + 64              # one region behind the sequences belongs to nobody
    # poisoned scratch (fp16 NaN): whatever the kernel is relied on to write, this call has to write
    kf = torch.full((Hkv, stride, D), 0x7e00, dtype=torch.int16, device='cuda').view(torch.float16)
    vf = torch.full((Hkv, D, stride) if transpose_v else (Hkv, stride, D), 0x7e00, dtype=torch.int16, device='cuda').view(torch.float16)
    _ffi.check(tm.tm_flatten_kv(kf.data_ptr(), vf.data_ptr(), transpose_v, dev(koff).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(),
                                len(klen), max(klen), stride, dc.view(layer), st()))
    K, V = host(kf), host(vf)
    if transpose_v:
        V = V.transpose(0, 2, 1)
    k_written, v_written = np.zeros(stride, bool), np.zeros(stride, bool)
    for b, n in enumerate(klen):
        kr, vr = o.flatten_kv(oc, tables[b], layer, n)
        assert np.array_equal(K[:, koff[b]:koff[b] + n].view(np.uint16), kr.view(np.uint16))
        assert np.array_equal(V[:, koff[b]:koff[b] + n].view(np.uint16), vr.view(np.uint16))
        if transpose_v:                      # columns [n, ceil64(n)) of every V^T row are zero: the prefill kernel relies on it
            assert not V[:, koff[b] + n:koff[b] + pad[b]].view(np.uint16).any()
        k_written[koff[b]:koff[b] + n] = True
        v_written[koff[b]:koff[b] + (pad[b] if transpose_v else n)] = True
    assert (K[:, ~k_written].view(np.uint16) == 0x7e00).all(), 'K rows outside [0, klen) of a flattened sequence were written'
    assert (V[:, ~v_written].view(np.uint16) == 0x7e00).all(), 'V outside the flattened sequences\' regions was written'


# ---- decode attention ------------------------------------------------------------------------------------------------------------
KLEN = [1, 31, 32, 33, 64, 65, 200]
_DECODE_CACHE = {}


def _decode_case(bits, Hkv):
    """filled cache + the dequantised K / V of every sequence, built once per (bits, Hkv) and left unchanged"""
    if (bits, Hkv) not in _DECODE_CACHE:
        rng = np.random.default_rng(bits + Hkv)
        L = o.BlockLayout(2, Hkv, D, 64, bits)
        tables, total = _tables(rng, KLEN, spare=2)
        oc = o.PagedKVCache(L, total)
        for b, n in enumerate(KLEN):
            k = rng.standard_normal((n, Hkv, D)).astype(f16)
            v = rng.standard_normal((n, Hkv, D)).astype(f16)
            if n > 40:
                k[n // 3] *= f16(6.0)        # forces the online-softmax rescale at a chosen tile
            o.process_kv(oc, tables[b], 1, k, v, None, None, 0)
        kv = []
        for b, n in enumerate(KLEN):
            pairs = [oc.load_dequant(tables[b], 1, hd, 0, n, 'decode') for hd in range(Hkv)]
            kv.append((np.stack([a for a, _ in pairs]), np.stack([c for _, c in pairs])))
        _DECODE_CACHE[(bits, Hkv)] = (L, tables, total, oc, kv)
    return _DECODE_CACHE[(bits, Hkv)]


def _check_decode(tm, bits, Hq, Hkv, splits, scale):
    L, tables, total, oc, kv = _decode_case(bits, Hkv)
    rng = np.random.default_rng(Hq + splits)
    B = len(KLEN)
    q = rng.standard_normal((B, Hq * D)).astype(f16)
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    out = torch.zeros((B, Hq * D), dtype=torch.float16, device='cuda')
    ws = torch.zeros(max(1, tm.tm_decode_attention_workspace(B, Hq, splits)), dtype=torch.uint8, device='cuda')
    _ffi.check(tm.tm_decode_attention(out.data_ptr(), dev(q).data_ptr(), Hq * D, dev(np.asarray(KLEN, np.int32)).data_ptr(), B, Hq,
                                      0.0 if scale is None else scale, splits, ws.data_ptr(), dc.view(1), st()))
    got = host(out).reshape(B, Hq, D).astype(np.float32)
    for b in range(B):
        ref = o.decode_attention(q[b].reshape(Hq, D), kv[b][0], kv[b][1], scale, 1).astype(np.float32)   # scale None: 1 / sqrt(64)
        err = np.abs(got[b] - ref)
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'seq {b} (k_len {KLEN[b]}): max err {err.max()}'


@pytest.mark.parametrize('splits', [1, 2, 5])                        # 5 leaves empty splits on the short contexts
@pytest.mark.parametrize('Hq,Hkv', [(8, 2), (6, 2), (14, 2), (2, 2)])   # heads per workgroup 4, 3, 1 (7 chunks), and no GQA
@pytest.mark.parametrize('bits', [16, 8, 4])
def test_decode_attention(tm, cuda, bits, Hq, Hkv, splits):
    _check_decode(tm, bits, Hq, Hkv, splits, None)                   # softmax_scale = 0 -> the oracle's 1 / sqrt(64)


def test_decode_attention_softmax_scale(tm, cuda):
    _check_decode(tm, 8, 8, 2, 2, 0.2)


def test_decode_attention_fused_refused(tm, cuda):
    """the fused-prologue entry point has no head_dim 64 kernel: status 1, nothing launched (out and cache untouched)"""
    L, tables, total, oc, kv = _decode_case(8, 2)
    Hq, B = 8, len(KLEN)
    dc = DevCache(L, total, tables)
    dc.upload(oc)
    qkv = dev(np.zeros((B, (Hq + 4) * D), f16))
    out = torch.full((B, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
    rc = tm.tm_decode_attention_fused(out.data_ptr(), qkv.data_ptr(), 0, (Hq + 4) * D, None, 0, dev(np.asarray(KLEN, np.int32)).data_ptr(),
                                      B, Hq, 0.0, 1, None, dc.view(1), st())
    assert rc == 1 and 'head_dim' in _ffi.last_error()
    torch.cuda.synchronize()
    assert (host(out) == 0x7e00).all() and np.array_equal(dc.download(), oc.pool)


# ---- prefill attention -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('qlens,hist', [((1,), (0,)), ((16,), (7,)), ((63, 65), (0, 64)), ((130, 5), (100, 0))])
@pytest.mark.parametrize('Hq,Hkv', [(8, 2), (6, 3), (14, 2)])        # G = 4, 2, 1 query heads per wave
def test_prefill_attention(tm, cuda, Hq, Hkv, qlens, hist):
    rng = np.random.default_rng(Hq + sum(qlens))
    B = len(qlens)
    klen = [h + n for h, n in zip(hist, qlens)]
    koff = np.concatenate([[0], np.cumsum([((k + 63) // 64) * 64 for k in klen])]).astype(np.int32)
    stride = int(koff[-1])
    cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    T = int(cu[-1])
    q = rng.standard_normal((T, Hq * D)).astype(f16)
    K = np.zeros((Hkv, stride, D), f16)
    Vt = np.zeros((Hkv, D, stride), f16)
    Ks, Vs = [], []
    for b, n in enumerate(klen):
        k = rng.standard_normal((Hkv, n, D)).astype(f16)
        v = rng.standard_normal((Hkv, n, D)).astype(f16)
        K[:, koff[b]:koff[b] + n] = k
        K[:, koff[b] + n:koff[b + 1]] = f16(np.nan)      # garbage past the context must be masked, not multiplied
        Vt[:, :, koff[b]:koff[b] + n] = v.transpose(0, 2, 1)
        Ks.append(k)
        Vs.append(v)
    out = torch.zeros((T, Hq * D), dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_prefill_attention_hd(out.data_ptr(), dev(q).data_ptr(), Hq * D, dev(K).data_ptr(), dev(Vt).data_ptr(), stride,
                                          dev(cu).data_ptr(), dev(koff).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), B,
                                          max(qlens), Hq, Hkv, D, 0.0, st()))
    got = host(out)
    for b, n in enumerate(qlens):
        ref = o.prefill_attention(q[cu[b]:cu[b + 1]].reshape(n, Hq, D), Ks[b], Vs[b], hist[b], None).reshape(n, -1).astype(np.float32)
        err = np.abs(got[cu[b]:cu[b + 1]].astype(np.float32) - ref)
        assert np.all(err <= 1e-2 * np.abs(ref) + 2e-3), f'seq {b}: max err {err.max()}'


def test_prefill_attention_refuses_other_head_dims(tm, cuda):
    z = dev(np.zeros(64 * 96, f16))
    i = dev(np.zeros(2, np.int32))
    rc = tm.tm_prefill_attention_hd(z.data_ptr(), z.data_ptr(), 96, z.data_ptr(), z.data_ptr(), 64, i.data_ptr(), i.data_ptr(), i.data_ptr(),
                                    1, 1, 1, 1, 96, 0.0, st())
    assert rc == 1 and 'head_dim' in _ffi.last_error()


# ---- engine ----------------------------------------------------------------------------------------------------------------------
def _cfg(kv_bits, **over):
    base = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=D, inter=512, vocab=1024, kv_bits=kv_bits, rope=ROPE)
    base.update(over)
    return base


def _engine_vs_oracle(cfg, w, oracle_cls, use_graph, prompt_lens=(70, 5, 64), steps=6, max_prefill=96, session_len=256):
    """prefill + `steps` decode steps against the oracle, teacher-forced with the engine's tokens; returns the worst logit difference"""
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in prompt_lens]
    eng = Engine.from_model_config(cfg, max_batch_size=len(prompts), session_len=session_len,
                                   quant_policy=0 if cfg.kv_bits == 16 else cfg.kv_bits, max_prefill_token_num=max_prefill,
                                   use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits().copy()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    eng.close()
    om = oracle_cls(cfg, w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    ref_logits, ref_toks = [lg], [ids]
    cur = toks[:, 0]
    for s in range(steps):
        ids, lg = om.forward([[int(t)] for t in cur])
        ref_logits.append(lg)
        ref_toks.append(ids)
        cur = toks[:, s + 1]
    worst = 0.0
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(np.float32) - ref_logits[s].astype(np.float32))
        worst = max(worst, float(d.max()))
        assert d.max() <= 3e-2, f'step {s}: max logit diff {d.max()}'
        top2 = np.sort(ref_logits[s].astype(np.float32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ref_toks[s][safe]), f'step {s}: greedy tokens differ'
    return worst


@pytest.mark.parametrize('use_graph', [0, 1])
@pytest.mark.parametrize('kv_bits', [8, 4, 16])
def test_engine_matches_oracle(cuda, kv_bits, use_graph):
    cfg = o.ModelConfig(**_cfg(kv_bits))
    worst = _engine_vs_oracle(cfg, o.make_synthetic_weights(cfg, seed=3), o.OracleModel, use_graph)
    print(f'[head_dim 64 engine vs oracle] kv_bits {kv_bits} graph {use_graph}: max logit diff {worst:.5f}')


def test_engine_qwen05b_attention_geometry(cuda):
    """14 query heads over 2 kv heads, hidden 896 (Qwen2.5-0.5B's attention geometry; Llama weights): GQA group 7"""
    cfg = o.ModelConfig(**_cfg(8, hidden=896, q_heads=14, inter=1024))
    _engine_vs_oracle(cfg, o.make_synthetic_weights(cfg, seed=4), o.OracleModel, 1)


def test_engine_qkv_bias(cuda):
    """the qkv bias at head_dim 64 (kv_rope_store applies it in prefill and decode): what lifting the Qwen readers' refusal needs"""
    cfg = QwenConfig(**_cfg(8, rms_eps=1e-6, rope=o.RopeParam(64, 1e6)), attn_bias=1)
    _engine_vs_oracle(cfg, make_qwen_weights(cfg, seed=5), QwenOracleModel, 1)


def test_engine_chunked_prefill(cuda):
    """a 150-token prompt over a 96-token budget: the second chunk runs the prefill kernel with history"""
    cfg = o.ModelConfig(**_cfg(8))
    _engine_vs_oracle(cfg, o.make_synthetic_weights(cfg, seed=6), o.OracleModel, 1, prompt_lens=(150, 9), steps=3)


@pytest.mark.parametrize('kv_bits', [8, 16])
def test_continuous_batching_mixed_steps(cuda, monkeypatch, kv_bits):
    """the scheduler with mixed steps (decode rows of the running requests + an admission's prefill in one forward), every request's
    tokens against the oracle alone, as tests/test_gpu_qwen_engine.py::test_qwen_continuous_batching_mixed_steps does it"""
    monkeypatch.setenv('TM_MIXED_STEP', '1')
    cfg = o.ModelConfig(**_cfg(kv_bits))
    w = o.make_synthetic_weights(cfg, seed=13)
    rng = np.random.default_rng(6)
    lens = [70, 5, 64, 33, 150, 9]
    news = [6, 12, 3, 9, 5, 8]
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in lens]
    eng = Engine.from_model_config(cfg, max_batch_size=3, session_len=256, quant_policy=0 if kv_bits == 16 else kv_bits,
                                   max_prefill_token_num=96)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    ids = [eng.submit(p, n, -1, None, None) for p, n in zip(prompts, news)]
    done, steps = {}, 0
    while len(done) < len(ids):
        eng.step()
        steps += 1
        assert steps < 400, 'scheduler does not make progress'
        for i, rid in enumerate(ids):
            if i not in done:
                status, toks = eng.poll(rid)
                if status != 0:
                    done[i] = (status, toks.copy())
    n_mixed = eng.mixed_steps()
    eng.close()
    assert n_mixed >= 3, f'{n_mixed} mixed steps'
    checked = 0
    for i, (status, toks) in done.items():
        assert status == 7 and len(toks) == news[i], f'request {i}: status {status}, {len(toks)} tokens'
        om = o.OracleModel(cfg, w, batch=1, max_ctx=256)
        feed = [prompts[i]]
        for k in range(news[i]):
            _, lg = om.forward(feed)
            row = lg[0].astype(np.float32)
            top2 = np.sort(row)[-2:]
            if top2[1] - top2[0] > 1.5e-2:
                assert int(toks[k]) == int(np.argmax(row)), f'request {i} token {k}: engine {toks[k]} oracle {np.argmax(row)}'
                checked += 1
            else:
                assert row[int(toks[k])] >= top2[1] - 1e-2
            feed = [[int(toks[k])]]
    assert checked >= sum(news) // 3


# ---- checkpoint on disk ----------------------------------------------------------------------------------------------------------
def _write_llama_checkpoint(path, hf, H, Hq, Hkv, I, V, layers, awq):
    """Llama-3.2-1B-style checkpoint: no head_dim key, llama3 rope scaling, tied embeddings (no lm_head tensor).  Returns the AWQ
    tensors written, {linear prefix: (q uint8 [K, N], s, z)}."""
    from safetensors.numpy import save_file
    tensors, quant = {}, {}
    for k, v in hf.items():
        if awq and k.endswith('_proj.weight'):
            pre = k[:-len('.weight')]
            q, s, z, _ = o.quantize_groupwise_u4(np.ascontiguousarray(v.T), 128)
            tensors[pre + '.qweight'] = o.pack_awq_gemm(q)
            tensors[pre + '.qzeros'] = o.pack_awq_gemm(z.astype(np.uint8))
            tensors[pre + '.scales'] = s
            quant[pre] = (q, s, z)
        else:
            tensors[k] = v
    save_file(tensors, os.path.join(path, 'model.safetensors'))
    c = {'architectures': ['LlamaForCausalLM'], 'hidden_size': H, 'num_hidden_layers': layers, 'num_attention_heads': Hq,
         'num_key_value_heads': Hkv, 'intermediate_size': I, 'vocab_size': V, 'rms_norm_eps': 1e-5, 'rope_theta': 500000.0,
         'max_position_embeddings': 131072, 'tie_word_embeddings': True, 'eos_token_id': 2, 'torch_dtype': 'float16',
         'rope_scaling': {'rope_type': 'llama3', 'factor': 32.0, 'low_freq_factor': 1.0, 'high_freq_factor': 4.0,
                          'original_max_position_embeddings': 8192}}
    if awq:
        c['quantization_config'] = {'quant_method': 'awq', 'bits': 4, 'group_size': 128, 'zero_point': True, 'version': 'gemm'}
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)
    return quant


@pytest.mark.parametrize('awq,kv_bits', [(False, 8), (True, 4)])
def test_checkpoint_through_pipeline(cuda, tmp_path, awq, kv_bits):
    """fabricated fp16 / AWQ Llama-3.2-1B-style checkpoint -> pipeline(path) -> greedy tokens and first-step logits against OracleModel
    on weights assembled here from the HF tensors (not by checkpoint.py)"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    rng = np.random.default_rng(21 + kv_bits)
    H, Hq, Hkv, I, V = 256, 4, 2, 512, 640
    hf = hf_qwen_tensors(rng, 'qwen2', H, Hq, Hkv, I, V, layers=2, D=D, bias=False, tie=True)   # Llama's tensor names, no biases
    quant = _write_llama_checkpoint(str(tmp_path), hf, H, Hq, Hkv, I, V, 2, awq)
    cfg = o.ModelConfig(hidden=H, layers=2, q_heads=Hq, kv_heads=Hkv, head_dim=D, inter=I, vocab=V, rms_eps=1e-5, kv_bits=kv_bits, rope=ROPE)
    w = tm_weights_from_hf(hf, cfg, quant if awq else None)
    prompts = [rng.integers(3, V, n).astype(np.int32).tolist() for n in (19, 5, 40)]
    N = 6
    pipe = pipeline(str(tmp_path), backend_config=TurbomindEngineConfig(model_format='awq' if awq else 'hf', quant_policy=kv_bits,
                                                                        max_batch_size=3, session_len=128))
    assert pipe.model_cfg.arch == 'llama' and pipe.model_cfg.head_dim == 64 and pipe.model_cfg.quantized == awq
    g = GenerationConfig(max_new_tokens=N, ignore_eos=True)
    got = [r.token_ids for r in pipe(prompts, g)]
    pipe.engine.prefill(prompts, max_new_tokens=2)
    lg0 = pipe.engine.fetch_logits().astype(np.float32)
    pipe.engine.release()
    pipe.close()
    om = o.OracleModel(cfg, w, batch=3, max_ctx=128)
    _, ref = om.forward([np.asarray(p) for p in prompts])
    ref = ref.astype(np.float32)
    assert np.abs(lg0 - ref).max() <= 3e-2, np.abs(lg0 - ref).max()
    for s in range(N):
        for b in range(3):
            top = np.argsort(ref[b])[::-1][:2]
            margin = ref[b][top[0]] - ref[b][top[1]]
            assert got[b][s] == top[0] or (margin <= 6e-2 and got[b][s] == top[1]), (b, s, got[b][s], top, margin)
        if s + 1 < N:
            _, ref = om.forward([[got[b][s]] for b in range(3)])
            ref = ref.astype(np.float32)
