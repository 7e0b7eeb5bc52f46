"""Dynamic-NTK and YaRN RoPE on the GPU: the device table builder against the host one, the per-sequence table rows of the K/V store
kernel bit for bit against the oracle, and the engine (static batch, continuous batching, scoring, a checkpoint on disk) against the
oracle run one sequence at a time with that sequence's own RoPE (tests/rope_scaling_reference.py).

Bounds: logits 3e-2 (tests/test_gpu_engine.py, same geometry), per-token NLL 6e-2 (tests/test_gpu_ppl.py), int8 KV codes within one
step on < 3 % of the entries and (scale, zero) within one fp16 ulp (tests/test_gpu_fullsize.py).  fp16 KV (no gate in the repository
yet): the engine's and the oracle's qkv GEMM outputs differ by at most one fp16 ulp (accumulation order), 2^-10 max|row| per element of a
head row; the rotation adds two such terms with |cos|, |sin| <= 1 and the result's own rounding may fall one ulp apart, so
|got - ref| <= 2^-9 max|ref row| + 2^-10 |ref| per element of a (head, token) row.

The synthetic weights of the oracle give nearly uniform attention (q . k ~ 1e-2), so their logits hardly move with the RoPE base
(measured 2e-4): a test on them would pass with the feature ignored.  The engine tests therefore scale the q / k columns of w_qkv by
32 and the v columns by 8 (through the AWQ scales: an exact change of the quantised model), which makes the oracle's logits differ by
0.34 .. 0.61 between a sequence's own base and the model's for the 150-token prompt and by 0.07 .. 0.27 for the 70-token one, whose base
moves least (logit sigma 0.1); the power check below asserts it on the oracle alone."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests import rope_scaling_reference as R
from tests.gpu_helpers import DevCache, dev, host, st, ulp_diff_f16

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32

LOGIT_BOUND = 3e-2
BASE, FACTOR, MAX_POS_EMB = 10000.0, 2.0, 64


def rope_param(**kw):
    p = _ffi.RopeParam(dim=128, base=BASE, type=0, factor=1.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position=8192,
                       max_position_embeddings=0, yarn_beta_fast=32.0, yarn_beta_slow=1.0, yarn_attention_factor=1.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def host_table(tm, max_pos, p):
    tab = np.zeros((max_pos, p.dim // 2, 2), f16)
    _ffi.check(tm.tm_rope_table_ex(tab.ctypes.data, max_pos, ctypes.byref(p)))
    return tab


# ---- 1. device table = host table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_pos', [300, 4097])
def test_device_table_equals_host_table(tm, cuda, max_pos):
    """both sides take double sin / cos of the same fp32 angle and round twice: equal up to a double-rounding boundary case"""
    af = R.yarn_attention_factor(dict(factor=4.0))
    total = differ = 0
    for p in (rope_param(type=4, base=37646.7734375, factor=2.0, max_position_embeddings=64), rope_param(type=4, base=1e6),
              rope_param(type=3, base=1e6, factor=4.0, max_position_embeddings=131072, yarn_attention_factor=af)):
        ref = host_table(tm, max_pos, p)
        out = torch.full((max_pos + 1, 64, 2), 7.0, dtype=torch.float16, device='cuda')     # one guard row behind the table
        _ffi.check(tm.tm_rope_table_device(out.data_ptr(), max_pos, ctypes.byref(p), st()))
        got = host(out)
        assert np.all(got[max_pos] == f16(7.0)), 'the kernel wrote behind the table'
        d = ulp_diff_f16(got[:max_pos], ref)
        assert d.max() <= 1
        total += d.size
        differ += int((d > 0).sum())
    print(f'[rope table] max_pos {max_pos}: {differ} of {total} entries differ from the host table')
    assert differ <= total / 1e5


# ---- 2. per-sequence rows, operator level -------------------------------------------------------------------------------------
def _kv_case(bits, lens_new, hist, Hq, Hkv, seed):
    rng = np.random.default_rng(seed)
    L = o.BlockLayout(2, Hkv, 128, 64, bits)
    klen = [h + n for h, n in zip(hist, lens_new)]
    nblk = [(k + 63) // 64 for k in klen]
    total = sum(nblk) + 3
    perm = rng.permutation(total)
    tables, off = [], 0
    for nb in nblk:
        tables.append(perm[off:off + nb])
        off += nb
    qkv = (rng.standard_normal((sum(lens_new), (Hq + 2 * Hkv) * 128)) * 1.5).astype(f16)
    qkv[1, Hq * 128:(Hq + 1) * 128] = f16(0.75)          # a constant row (scale 0), a row with an outlier
    qkv[2, (Hq + Hkv) * 128 + 5] = f16(300.0)
    return L, tables, total, klen, qkv


@pytest.mark.parametrize('bits', [16, 8, 4])
@pytest.mark.parametrize('lens_new,hist', [([70, 5, 1], [0, 130, 63]),     # (1, 63): the last position of a block
                                           ([70, 5, 1], [0, 130, 259])])   # position 259 = max_pos + 3: clamps inside its OWN region
def test_kv_rope_store_per_sequence_rows(tm, cuda, bits, lens_new, hist):
    Hq, Hkv, layer, max_pos = 4, 2, 1, 256
    L, tables, total, klen, qkv = _kv_case(bits, lens_new, hist, Hq, Hkv, seed=bits + hist[2])
    row0 = np.array([256, 0, 512], np.int32)             # not in sequence order; 0 = the shared (first) region
    bases = {0: 10000.0, 256: 37646.7734375, 512: 1e6}
    tab = np.concatenate([host_table(tm, max_pos, rope_param(type=4, base=bases[r])) for r in (0, 256, 512)])
    assert tab.shape == (768, 64, 2)
    # oracle: every sequence with the default RoPE of its base, positions clamped to the table's last row
    oc = o.PagedKVCache(L, total)
    cu = np.concatenate([[0], np.cumsum(lens_new)]).astype(np.int32)
    q_ref = np.zeros((len(qkv), Hq, 128), f16)
    for b, n in enumerate(lens_new):
        sl = slice(cu[b], cu[b + 1])
        pos = np.arange(hist[b], hist[b] + n)
        cos, sin = o.rope_cos_sin(o.RopeParam(128, bases[int(row0[b])]), np.minimum(pos, max_pos - 1))
        q_ref[sl] = o.rope_apply(qkv[sl, :Hq * 128].reshape(n, Hq, 128), cos, sin)
        o.process_kv(oc, tables[b], layer, qkv[sl, Hq * 128:(Hq + Hkv) * 128].reshape(n, Hkv, 128),
                     qkv[sl, (Hq + Hkv) * 128:].reshape(n, Hkv, 128), cos, sin, hist[b])
    args = (Hq, dev(cu).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), len(lens_new), len(qkv), dev(tab).data_ptr(), max_pos)
    dc = DevCache(L, total, tables)
    qkv_d = dev(qkv)
    _ffi.check(tm.tm_kv_rope_store_seq(qkv_d.data_ptr(), *args, dev(row0).data_ptr(), None, None, None, 0.0, dc.view(layer), st()))
    got = dc.download()
    assert np.array_equal(got, oc.pool), f'cache bytes differ in {np.count_nonzero(got != oc.pool)} positions'
    q_got = host(qkv_d)[:, :Hq * 128].reshape(-1, Hq, 128)
    assert np.array_equal(q_got.view(np.uint16), q_ref.view(np.uint16)), 'RoPE(q) must be bit exact'
    # rope_row0 = NULL is tm_kv_rope_store_qk: every sequence on the first region
    d1, d2 = DevCache(L, total, tables), DevCache(L, total, tables)
    q1, q2 = dev(qkv), dev(qkv)
    _ffi.check(tm.tm_kv_rope_store_seq(q1.data_ptr(), *args, None, None, None, None, 0.0, d1.view(layer), st()))
    _ffi.check(tm.tm_kv_rope_store_qk(q2.data_ptr(), *args, None, None, None, 0.0, d2.view(layer), st()))
    assert np.array_equal(d1.download(), d2.download()) and torch.equal(q1, q2)
    assert not np.array_equal(d1.download(), got), 'the three bases must give different K bytes'


# ---- engine ---------------------------------------------------------------------------------------------------------------------
def tiny_cfg(kv_bits):
    return o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, kv_bits=kv_bits,
                         rope=o.RopeParam(128, BASE))


def rope_sensitive_weights(cfg, seed=3):
    """the oracle's synthetic weights with q / k scaled by 32 and v by 8 through the AWQ scales (see the module docstring)"""
    w = o.make_synthetic_weights(cfg, seed=seed)
    nqk = (cfg.q_heads + cfg.kv_heads) * cfg.head_dim
    for L in w['layers']:
        s = L['w_qkv']['s']
        s[:, :nqk] = (s[:, :nqk].astype(f32) * f32(32)).astype(f16)
        s[:, nqk:] = (s[:, nqk:].astype(f32) * f32(8)).astype(f16)
    return w


def engine_cfg(cfg, rope):
    return dataclasses.replace(cfg, rope=rope)


def dynamic_rope(max_pos_emb=MAX_POS_EMB):
    return checkpoint.RopeConfig(128, BASE, 'dynamic', FACTOR, max_position_embeddings=max_pos_emb)


def seq_rope(tm, n):
    """the oracle's RoPE of a sequence admitted with an n-token prompt: the default recipe at the base the engine computes"""
    return o.RopeParam(128, float(f32(tm.tm_rope_dynamic_base(BASE, FACTOR, 128, MAX_POS_EMB, n))))


def max_diff(a, b):
    return np.abs(np.asarray(a).astype(f32) - np.asarray(b).astype(f32)).max(axis=-1)


def check_kv_blocks(eng, oracle, lens, new_tokens, kv_bits):
    """KV bytes of layer 0 of every static-batch sequence against the oracle's cache of that sequence"""
    for b, n in enumerate(lens):
        om = oracle.models[b]
        L = om.layout
        data = L.kv_heads * 2 * L.head_data_size
        for i in range((n + new_tokens + 63) // 64):
            got, ref = eng.fetch_kv_block(b, i), om.cache.pool[om.tables[0][i]]
            valid = min(64, n + new_tokens - 64 * i)
            if kv_bits == 16:
                g = got[:data].view(f16).reshape(L.kv_heads * 2, 64, 128)[:, :valid].astype(f32)
                r = ref[:data].view(f16).reshape(L.kv_heads * 2, 64, 128)[:, :valid].astype(f32)
                tol = 2.0**-9 * np.abs(r).max(axis=-1, keepdims=True) + 2.0**-10 * np.abs(r)
                assert np.all(np.abs(g - r) <= tol), f'seq {b} block {i}: K/V differ by {np.abs(g - r).max()}'
                continue
            gc = got[:data].reshape(L.kv_heads * 2, 64, 128)[:, :valid].astype(np.int32)
            rc = ref[:data].reshape(L.kv_heads * 2, 64, 128)[:, :valid].astype(np.int32)
            assert np.abs(gc - rc).max() <= 1 and (gc != rc).mean() < 0.03, f'seq {b} block {i}: codes differ ({(gc != rc).mean():.4f})'
            gp = got[data:data + L.kv_heads * 2 * 256].view(f16).reshape(L.kv_heads * 2, 64, 2)[:, :valid]
            rp = ref[data:data + L.kv_heads * 2 * 256].view(f16).reshape(L.kv_heads * 2, 64, 2)[:, :valid]
            assert ulp_diff_f16(gp, rp).max() <= 1, f'seq {b} block {i}: (scale, zero) differ'


def run_static_wave(tm, eng, cfg, w, prompts, steps, kv_bits, what):
    """prefill + `steps` decode steps against the per-sequence oracle (teacher-forced with the engine's tokens); returns the
    oracle's logits of every step and the per-sequence oracle"""
    lens = [len(p) for p in prompts]
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits())
    toks = eng.fetch()
    oracle = R.PerSequenceOracle(cfg, w, [seq_rope(tm, n) for n in lens], 256)
    _, lg = oracle.forward(prompts)
    ref = [lg]
    for s in range(steps):
        _, lg = oracle.forward([[int(t)] for t in toks[:, s]])
        ref.append(lg)
    worst = max(float(max_diff(logits[s], ref[s]).max()) for s in range(steps + 1))
    print(f'[dynamic rope] {what}: lens {lens} max logit diff over {steps + 1} steps {worst:.5f}')
    for s in range(steps + 1):
        d = max_diff(logits[s], ref[s])
        assert d.max() <= LOGIT_BOUND, f'{what} step {s}: max logit diff per sequence {d}'
    check_kv_blocks(eng, oracle, lens, steps, kv_bits)
    return ref, toks, oracle


@pytest.mark.parametrize('use_graph', [1, 0])
@pytest.mark.parametrize('kv_bits', [8, 16])
def test_engine_dynamic_static_batch(tm, cuda, kv_bits, use_graph):
    """prompts of 150, 70 and 5 tokens over max_position_embeddings 64: two sequences with a base of their own, one on the shared
    table; then the slots are reused by (5, 150, 100) -- a stale offset (slot 0: own -> shared), a stale table (slot 1: another base)
    or a missing one (slot 2: shared -> own) would show; then the 150-token prompt is scored."""
    cfg = tiny_cfg(kv_bits)
    w = rope_sensitive_weights(cfg)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (150, 70, 5)]
    wave2 = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (5, 150, 100)]
    steps = 3
    eng = Engine.from_model_config(engine_cfg(cfg, dynamic_rope()), max_batch_size=3, session_len=256,
                                   quant_policy=0 if kv_bits == 16 else kv_bits, max_prefill_token_num=96, use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    info = eng.rope_info()
    assert info['per_seq_tables'] and info['table_bytes'] == 3 * 257 * 128 * 2
    ref, toks, _ = run_static_wave(tm, eng, cfg, w, prompts, steps, kv_bits, f'kv {kv_bits} graph {use_graph} wave 1')
    eng.release()
    run_static_wave(tm, eng, cfg, w, wave2, steps, kv_bits, f'kv {kv_bits} graph {use_graph} wave 2')
    eng.release()
    nll = eng.score([prompts[0]])[0]
    eng.close()

    # power check, on the oracle alone: the same sequences on the MODEL's base differ by more than 10 x the bound, and each
    # sequence with a base of its own by more than 2 x the bound at some step -- the test cannot pass with the feature ignored for either
    plain = R.PerSequenceOracle(cfg, w, [o.RopeParam(128, BASE)] * 3, 256)
    _, lg = plain.forward(prompts)
    gaps = [max_diff(lg, ref[0])]
    for s in range(steps):
        _, lg = plain.forward([[int(t)] for t in toks[:, s]])
        gaps.append(max_diff(lg, ref[s + 1]))
    gaps = np.stack(gaps)
    print(f'[dynamic rope] oracle, own base vs model base, per step x sequence:\n{gaps}')
    assert gaps.max() > 10 * LOGIT_BOUND and gaps[:, :2].max(axis=0).min() > 2 * LOGIT_BOUND and gaps[:, 2].max() == 0

    # scoring: per-row NLL of the 150-token prompt against the oracle with that prompt's base (test_gpu_ppl.py's bound)
    from tests.test_gpu_ppl import nll_rows
    om = R.PerSequenceOracle(cfg, w, [seq_rope(tm, 150)], 256).models[0]
    om.forward([prompts[0]])
    lg = o.lm_head(o.rmsnorm(om.last_resid, w['norm'], cfg.rms_eps), w['output'])
    ref_nll = nll_rows(lg[:149], prompts[0][1:])
    d = float(np.abs(nll.astype(np.float64) - ref_nll).max())
    print(f'[dynamic rope] kv {kv_bits}: max per-token NLL diff {d:.4f}')
    assert len(nll) == 149 and d <= 6e-2


@pytest.mark.parametrize('use_graph', [1, 0])
@pytest.mark.parametrize('kv_bits', [8, 16])
def test_engine_dynamic_continuous_batching(tm, cuda, kv_bits, use_graph):
    """six requests through three slots (tm_engine_submit): admissions join a running batch, slots are reused by prompts of other
    lengths (own base -> shared, shared -> own, one base -> another), the 150-token prompts are chunked.  Every request is replayed
    through the oracle alone with ITS base, as tests/test_gpu_engine.py::test_continuous_batching_matches_oracle does."""
    cfg = tiny_cfg(kv_bits)
    w = rope_sensitive_weights(cfg)
    rng = np.random.default_rng(6)
    lens = [150, 70, 5, 100, 9, 150]
    news = [4, 6, 3, 5, 7, 4]
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in lens]
    eng = Engine.from_model_config(engine_cfg(cfg, dynamic_rope()), max_batch_size=3, session_len=256,
                                   quant_policy=0 if kv_bits == 16 else kv_bits, max_prefill_token_num=96, use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    ids = [eng.submit(p, n, -1) for p, n in zip(prompts, news)]
    done, steps = {}, 0
    while len(done) < len(ids):
        eng.step()
        steps += 1
        assert steps < 200, 'scheduler does not make progress'
        for i, rid in enumerate(ids):
            if i not in done:
                s_, toks = eng.poll(rid)
                if s_ != 0:
                    done[i] = (s_, toks.copy())
    assert eng.rope_info()['per_seq_tables']
    eng.close()
    checked = 0
    for i, (s_, toks) in done.items():
        assert s_ == 7 and len(toks) == news[i], f'request {i}: status {s_}, {len(toks)} tokens'
        om = R.PerSequenceOracle(cfg, w, [seq_rope(tm, lens[i])], 256)
        feed = [prompts[i]]
        for k in range(news[i]):
            _, lg = om.forward(feed)
            row = lg[0].astype(f32)
            top2 = np.sort(row)[-2:]
            if top2[1] - top2[0] > 1.5e-2:
                assert int(toks[k]) == int(np.argmax(row)), f'request {i} token {k}: engine {toks[k]} oracle {np.argmax(row)}'
                checked += 1
            else:
                assert row[int(toks[k])] >= top2[1] - 1e-2
            feed = [[int(toks[k])]]
    assert checked >= sum(news) // 3


# ---- 4. dynamic inert ----------------------------------------------------------------------------------------------------------
def test_engine_dynamic_inert_is_the_default_engine(cuda):
    """session_len <= max_position_embeddings: no sequence can take a base of its own -- one table, no extra memory, the fused
    decode prologue, and logits bitwise equal to rope_type 0"""
    cfg = tiny_cfg(8)
    w = rope_sensitive_weights(cfg)
    rng = np.random.default_rng(1)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (40, 5, 17)]
    out = {}
    for name, rope in (('dynamic', dynamic_rope(64)), ('default', checkpoint.RopeConfig(128, BASE))):
        eng = Engine.from_model_config(engine_cfg(cfg, rope), max_batch_size=3, session_len=64, quant_policy=8, max_prefill_token_num=96)
        eng.load_weights(export_weights(cfg, w))
        eng.start()
        info = eng.rope_info()
        assert not info['per_seq_tables'] and info['table_bytes'] == 0
        eng.prefill(prompts, max_new_tokens=4)
        lg = [eng.fetch_logits()]
        for _ in range(3):
            eng.decode(1)
            lg.append(eng.fetch_logits())
        out[name] = (np.stack(lg), eng.fetch())
        # the fused prologue is in use: a decode step launches no separate K/V store
        eng.release()
        eng.prefill(prompts, max_new_tokens=4)
        prof = eng.profile_decode(1)
        assert prof['kv_store'][1] == 0, f'{name}: {prof["kv_store"][1]} kv_store launches in a decode step'
        eng.close()
    assert np.array_equal(out['dynamic'][0].view(np.uint16), out['default'][0].view(np.uint16))
    assert np.array_equal(out['dynamic'][1], out['default'][1])


# ---- 5. YaRN engine ---------------------------------------------------------------------------------------------------------------
def test_engine_yarn_static_batch(tm, cuda):
    rs = dict(factor=4.0)
    af = R.yarn_attention_factor(rs)
    cfg = tiny_cfg(8)
    w = rope_sensitive_weights(cfg)
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (150, 70, 5)]
    rope = checkpoint.RopeConfig(128, BASE, 'yarn', 4.0, max_position_embeddings=256, attention_factor=af)
    eng = Engine.from_model_config(engine_cfg(cfg, rope), max_batch_size=3, session_len=256, quant_policy=8, max_prefill_token_num=96)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    assert not eng.rope_info()['per_seq_tables']
    eng.prefill(prompts, max_new_tokens=4)
    logits = [eng.fetch_logits()]
    for _ in range(3):
        eng.decode(1)
        logits.append(eng.fetch_logits())
    toks = eng.fetch()
    eng.close()
    tab = R.table_packed(R.yarn_inv_freq(128, BASE, 4.0, 256), 257, af)
    oracle = R.PerSequenceOracle(cfg, w, [tab] * 3, 256)
    plain = R.PerSequenceOracle(cfg, w, [o.RopeParam(128, BASE)] * 3, 256)
    feed, gap = prompts, 0.0
    for s in range(4):
        _, lg = oracle.forward(feed)
        _, lp = plain.forward(feed)
        d = max_diff(logits[s], lg)
        gap = max(gap, float(max_diff(lp, lg).max()))
        print(f'[yarn] step {s}: max logit diff per sequence {d}')
        assert d.max() <= LOGIT_BOUND
        feed = [[int(t)] for t in toks[:, s]]
    assert gap > 10 * LOGIT_BOUND, f'yarn vs default on the oracle: {gap}'


# ---- 6. checkpoint round trip -----------------------------------------------------------------------------------------------------
def test_internlm2_dynamic_checkpoint_through_pipeline(tm, cuda, tmp_path):
    """a tiny InternLM2 AWQ checkpoint with rope_scaling dynamic and max_position_embeddings 64 -> pipeline() with session_len 256:
    greedy tokens of a 100-token prompt (a base of its own) and a 19-token one against the per-sequence oracle.  The plumbing test
    (config.json -> RopeConfig -> engine with per-sequence tables); the fabricated weights are the insensitive kind, the numeric power
    sits in the engine tests above."""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    from tests.test_gpu_checkpoint import _fabricate
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=640, kv_bits=8,
                        rope=o.RopeParam(128, BASE), rms_eps=1e-6)
    rng = np.random.default_rng(11)
    w = _fabricate(str(tmp_path), 'internlm2', cfg, rng)
    path = os.path.join(str(tmp_path), 'config.json')
    hf = json.load(open(path))
    hf.update(max_position_embeddings=MAX_POS_EMB, rope_scaling={'type': 'dynamic', 'factor': FACTOR})
    json.dump(hf, open(path, 'w'))
    lens = (100, 19)
    prompts = [rng.integers(3, cfg.vocab, n).astype(np.int32).tolist() for n in lens]
    N = 5
    pipe = pipeline(str(tmp_path), backend_config=TurbomindEngineConfig(model_format='awq', quant_policy=8, max_batch_size=2, session_len=256))
    r = pipe.model_cfg.rope
    assert (pipe.model_cfg.arch, r.type, r.factor, r.max_position_embeddings) == ('internlm2', 'dynamic', FACTOR, MAX_POS_EMB)
    assert pipe.engine.rope_info()['per_seq_tables']
    got = [x.token_ids for x in pipe(prompts, GenerationConfig(max_new_tokens=N, ignore_eos=True))]
    pipe.engine.prefill(prompts, max_new_tokens=2)
    lg0 = pipe.engine.fetch_logits().astype(f32)
    pipe.engine.release()
    pipe.close()
    oracle = R.PerSequenceOracle(cfg, w, [seq_rope(tm, n) for n in lens], 256)
    _, ref = oracle.forward([np.asarray(p) for p in prompts])
    ref = ref.astype(f32)
    assert np.abs(lg0 - ref).max() <= LOGIT_BOUND, np.abs(lg0 - ref).max()
    for s in range(N):
        for b in range(2):
            top = np.argsort(ref[b])[::-1][:2]
            margin = ref[b][top[0]] - ref[b][top[1]]
            assert got[b][s] == top[0] or (margin <= 6e-2 and got[b][s] == top[1]), (b, s, got[b][s], top, margin)
        if s + 1 < N:
            _, ref = oracle.forward([[got[b][s]] for b in range(2)])
            ref = ref.astype(f32)
