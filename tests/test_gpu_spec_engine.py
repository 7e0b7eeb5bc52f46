"""Speculative decoding by prompt lookup, kernel to pipeline(), on the GPU:

(a) the proposer and acceptance kernels (csrc/speculative.hip, through tm_spec_propose / tm_spec_accept) against the integers of
    tests/spec_reference.py on random low-entropy histories and the hand-made cases of tests/test_host_spec.py;
(b) Engine.verify with injected drafts -- right ones (the engine's own plain greedy run), the same with position 1 replaced by the
    oracle's arg-min token, all wrong, none -- on the `tiny` geometry of tests/test_gpu_engine.py, prompts (70, 5, 64), k = 3, int8 /
    int4 KV (the verify attention kernel) and fp16 KV (flatten + prefill attention): the emitted tokens are teacher-forced into the
    oracle model, every emitted position's logits stay within its 3e-2 and tokens are equal wherever the oracle's top-2 gap exceeds its
    6e-2 -- which also holds the cache of rejected rows to being overwritten by the following steps -- and the accepted counts are
    what the drafts allow;
(c) decode_spec end to end on a model whose next token is a function of the current token alone (wo = w2 = 0, fp16 weights): the
    per-step emitted counts and the tokens equal the pure-Python simulation, which reaches k + 1 tokens per step inside the cycle and
    ends at max_new inside an accepted run; eager and graph replay;
(d) pipeline(..., speculative_config=SpeculativeConfig('ngram', ...)): token counts, finish reasons, truncation at a stop id inside an
    accepted run, the statistics' identity, and a sampling call that runs the plain path."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import GenerationConfig, SpeculativeConfig, TurbomindEngineConfig, _ffi, pipeline
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests import spec_reference as sr
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
ROPE = o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192)
TINY = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, rope=ROPE)


# ---- (a) kernels ---------------------------------------------------------------------------------------------------------------------
def _propose(tm, hist, hist_len, emitted, max_new, k, n_max, n_min):
    B = len(hist_len)
    drafts = torch.full((B, k), -7, dtype=torch.int32, device='cuda')
    nd = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    _ffi.check(tm.tm_spec_propose(drafts.data_ptr(), nd.data_ptr(), dev(hist.astype(np.int32)).data_ptr(), hist.shape[1],
                                  dev(np.asarray(hist_len, np.int32)).data_ptr(), dev(np.asarray(emitted, np.int32)).data_ptr(), max_new, B, k,
                                  n_max, n_min, st()))
    return host(drafts), host(nd)


def test_spec_propose_kernel(tm, cuda):
    rng = np.random.default_rng(0)
    B, stride, max_new = 64, 700, 24
    hist = rng.integers(0, 3, (B, stride))                          # three symbols: every n-gram size finds matches
    hist[:8] = rng.integers(0, 1000, (8, stride))                   # ... and rows that find none
    hist[8] = 5                                                     # "a a a a ...": overlap
    hist[12:20] = np.arange(stride)[None, :] % 11 + np.arange(8)[:, None]      # period 11: the 8-grams find their match too
    hist_len = rng.integers(1, stride + 1, B)
    hist_len[:6] = (1, 2, 3, stride, 257, 256)                      # nothing in front of the suffix; more than one pass of the 256 threads
    hist_len[8] = 4
    emitted = rng.integers(1, max_new + 1, B)                       # remaining 0 .. max_new - 1
    emitted[9:12] = (max_new, max_new - 1, max_new - 2)
    for k, n_max, n_min in ((1, 1, 1), (3, 3, 1), (7, 8, 2), (4, 8, 8), (7, 3, 3)):
        d, nd = _propose(tm, hist, hist_len, emitted, max_new, k, n_max, n_min)
        ed, end = sr.propose_batch(hist, hist_len, emitted, max_new, k, n_max, n_min)
        assert np.array_equal(nd, end), (k, n_max, n_min, np.flatnonzero(nd != end)[:5])
        assert np.array_equal(d, ed), (k, n_max, n_min)
        assert nd.max() > 0 and (nd == 0).any()
    # the hand-made cases of tests/test_host_spec.py
    cases = [([1, 2, 3, 4, 5], 3, 3, 1, 10), ([7], 3, 3, 1, 10), ([9, 9, 9, 9], 3, 3, 1, 10), ([9, 9, 9, 9], 3, 1, 1, 10),
             ([1, 2, 3, 50, 9, 3, 60, 1, 2, 3], 2, 3, 1, 10), ([1, 2, 3, 50, 9, 3, 60, 1, 2, 3], 2, 1, 1, 10),
             ([4, 5, 10, 4, 5, 20, 4, 5], 3, 2, 2, 10), ([4, 5, 6, 4, 5], 5, 2, 1, 10), ([4, 5, 10, 11, 12, 4, 5], 3, 2, 1, 3),
             ([4, 5, 10, 11, 12, 4, 5], 3, 2, 1, 1)]
    for h, k, n_max, n_min, remaining in cases:
        row = np.zeros((1, 16), np.int64)
        row[0, :len(h)] = h
        d, nd = _propose(tm, row, [len(h)], [20 - remaining], 20, k, n_max, n_min)
        want = sr.ngram_propose(h, k, n_max, n_min, remaining)
        assert nd[0] == len(want) and d[0, :nd[0]].tolist() == want and not d[0, nd[0]:].any(), (h, k, n_max, n_min, remaining)


@pytest.mark.parametrize('k', [1, 3, 7])
def test_spec_accept_kernel(tm, cuda, k):
    rng = np.random.default_rng(k)
    B, stride, max_new = 96, 64, 12
    prompt = rng.integers(1, 20, B)
    emitted = rng.integers(1, max_new + 1, B)
    emitted[:4] = (max_new, max_new - 1, max_new - 2, 1)
    hist_len = prompt + emitted
    hist = rng.integers(0, 50, (B, stride)).astype(np.int32)
    gen = rng.integers(0, 50, (B, max_new)).astype(np.int32)
    k_len = (hist_len - 1).astype(np.int32)
    next_id = rng.integers(0, 50, B).astype(np.int32)
    drafts = rng.integers(0, 50, (B, k)).astype(np.int32)
    n_draft = rng.integers(0, k + 1, B).astype(np.int32)
    ids = rng.integers(0, 50, (B, k + 1)).astype(np.int32)
    right = rng.integers(0, k + 2, B)                               # the first `right` ids agree with the drafts
    right[3], n_draft[3] = k + 1, k                                 # row 3 (emitted = 1): every draft right, k + 1 tokens
    for b in range(B):
        ids[b, :min(right[b], k)] = drafts[b, :min(right[b], k)]
    totals0 = np.asarray([5, 6, 7, 8], np.int64)
    d = {n: torch.from_numpy(np.ascontiguousarray(a)).cuda() for n, a in dict(hist=hist, hist_len=hist_len.astype(np.int32),
         emitted=emitted.astype(np.int32), gen=gen, k_len=k_len, next_id=next_id, totals=totals0).items()}
    step = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    _ffi.check(tm.tm_spec_accept(dev(ids).data_ptr(), dev(drafts).data_ptr(), dev(n_draft).data_ptr(), d['hist'].data_ptr(), stride,
                                 d['hist_len'].data_ptr(), d['emitted'].data_ptr(), d['gen'].data_ptr(), max_new, d['k_len'].data_ptr(),
                                 d['next_id'].data_ptr(), d['totals'].data_ptr(), step.data_ptr(), B, k, st()))
    e_hist, e_gen, e_emitted, e_len, e_klen, e_next = hist.copy(), gen.copy(), emitted.copy(), hist_len.copy(), k_len.copy(), next_id.copy()
    e_step, tot = np.zeros(B, np.int32), totals0.copy()
    for b in range(B):
        new = sr.accept(ids[b], drafts[b], int(n_draft[b]), max_new - int(emitted[b]))
        e_step[b] = len(new)
        if not new:
            continue
        e_gen[b, emitted[b]:emitted[b] + len(new)] = new
        e_hist[b, hist_len[b]:hist_len[b] + len(new)] = new
        e_emitted[b] += len(new)
        e_len[b] += len(new)
        e_klen[b] += len(new)
        e_next[b] = new[-1]
        tot += (1, int(n_draft[b]), len(new) - 1, len(new))
    assert np.array_equal(host(step), e_step) and e_step[0] == 0 and e_step.max() == min(k + 1, max_new - 1)
    for name, want in dict(hist=e_hist, gen=e_gen, emitted=e_emitted, hist_len=e_len, k_len=e_klen, next_id=e_next, totals=tot).items():
        assert np.array_equal(host(d[name]), want), name


# ---- (b) injected drafts against the oracle ------------------------------------------------------------------------------------------
K, MAX_NEW = 3, 14
_ORACLE = {}      # (kv_bits, emitted tokens) -> teacher-forced oracle logits [B, MAX_NEW, V]


def _oracle_logits(cfg, w, prompts, toks):
    key = (cfg.kv_bits, toks.tobytes())
    if key not in _ORACLE:
        om = o.OracleModel(cfg, w, batch=len(prompts), max_ctx=256)
        _, lg = om.forward(prompts)
        ref = [lg]
        for p in range(1, toks.shape[1]):
            _, lg = om.forward([[int(t)] for t in toks[:, p - 1]])
            ref.append(lg)
        _ORACLE[key] = np.stack(ref, 1).astype(np.float32)
    return _ORACLE[key]


@pytest.mark.parametrize('kv_bits,use_graph', [(8, 1), (8, 0), (4, 1), (4, 0), (16, 1), (16, 0)])
def test_engine_verify_matches_oracle(cuda, kv_bits, use_graph):
    cfg = o.ModelConfig(kv_bits=kv_bits, **TINY)
    w = o.make_synthetic_weights(cfg, seed=3)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (70, 5, 64)]
    B = len(prompts)
    eng = Engine.from_model_config(cfg, max_batch_size=4, session_len=256, quant_policy=0 if kv_bits == 16 else kv_bits,
                                   max_prefill_token_num=96, use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    try:
        # the plain greedy run of the same engine: the right drafts
        eng.prefill(prompts, max_new_tokens=MAX_NEW)
        eng.decode(MAX_NEW - 1)
        G = eng.fetch().copy()
        eng.release()
        ref_g = _oracle_logits(cfg, w, prompts, G)
        top2 = np.sort(ref_g, -1)[..., -2:]
        safe = (top2[..., 1] - top2[..., 0]) > 6e-2                  # [B, MAX_NEW]
        argmin = ref_g.argmin(-1)

        eng.set_speculative(K, 3, 1)
        with pytest.raises(_ffi.TmError, match='session_len'):
            eng.prefill(prompts, max_new_tokens=256 - 70 - K + 1)    # no room for the k rows behind the last allowed token
        eng.prefill(prompts, max_new_tokens=MAX_NEW)
        with pytest.raises(_ffi.TmError, match='decode_spec'):
            eng.decode(1)                                            # a batch admitted with speculation armed does not run plain steps
        logits = np.zeros((B, MAX_NEW, cfg.vocab), np.float32)
        logits[:, 0] = eng.fetch_logits()
        toks, counts = eng.fetch_spec()
        assert counts.tolist() == [1] * B and np.array_equal(toks[:, 0], G[:, 0])
        kinds, step = ('right', 'corrupted', 'wrong', 'none'), 0
        n_checked = dict.fromkeys(kinds, 0)
        while (counts < MAX_NEW).any():
            kind = kinds[step % 4]
            drafts, nd = np.zeros((B, K), np.int32), np.zeros(B, np.int32)
            for b in range(B):
                c = int(counts[b])
                avail = min(K, MAX_NEW - c)
                if kind == 'none' or avail == 0:
                    continue
                nd[b] = avail
                drafts[b, :avail] = argmin[b, c:c + avail] if kind == 'wrong' else G[b, c:c + avail]
                if kind == 'corrupted' and avail >= 2:
                    drafts[b, 1] = argmin[b, c + 1]
            eng.verify(drafts, nd)
            new_toks, new_counts = eng.fetch_spec()
            lg = eng.fetch_spec_logits()
            for b in range(B):
                c, n = int(counts[b]), int(new_counts[b] - counts[b])
                logits[b, c:c + n] = lg[b, :n]
                assert np.array_equal(new_toks[b, :c], toks[b, :c])          # what was emitted stays
                if c == MAX_NEW:
                    assert n == 0
                    continue
                assert 1 <= n <= min(int(nd[b]) + 1, MAX_NEW - c)
                if not np.array_equal(toks[b, :c], G[b, :c]):                 # a near-tie took this sequence off the plain run: the
                    continue                                                  # drafts are no longer what their kind says
                lead = 0
                while lead < nd[b] and safe[b, c + lead]:
                    lead += 1
                if kind == 'right':
                    assert n - 1 >= min(lead, MAX_NEW - c - 1), (kind, b, c, n, lead)
                elif kind == 'corrupted' and nd[b] >= 2 and lead >= 2:
                    assert n - 1 == 1, (kind, b, c, n)
                elif kind in ('wrong', 'none'):
                    assert n - 1 == 0, (kind, b, c, n)
                n_checked[kind] += 1
            toks, counts, step = new_toks, new_counts, step + 1
        assert counts.tolist() == [MAX_NEW] * B and all(v > 0 for v in n_checked.values()), n_checked
        stats = eng.spec_stats()
        assert stats['emitted'] == B * (MAX_NEW - 1) == stats['accepted'] + stats['steps']
        eng.release()
    finally:
        eng.close()
    ref = ref_g if np.array_equal(toks, G) else _oracle_logits(cfg, w, prompts, toks)      # teacher-forced on the EMITTED tokens
    d = np.abs(logits - ref).max(-1)
    print(f'[spec engine vs oracle] kv_bits {kv_bits} graph {use_graph}: {step} steps, max logit diff {d.max():.5f}, '
          f'emitted == plain greedy: {np.array_equal(toks, G)}')
    assert d.max() <= 3e-2, f'max logit diff {d.max()} at (sequence, position) {np.unravel_index(d.argmax(), d.shape)}'
    top2 = np.sort(ref, -1)[..., -2:]
    ok = (top2[..., 1] - top2[..., 0]) > 6e-2
    assert np.array_equal(toks[ok], ref.argmax(-1)[ok])


# ---- (c) end to end on a cyclic model ------------------------------------------------------------------------------------------------
CYC_SEED, CYC_SCALE, CYC_STARTS, CYC_MAX_NEW = 7, 16.0, (514, 203), 47
_CYCLIC = {}


def _cyclic_model():
    """wo = w2 = 0: the residual stream is the embedding, so the next token is a function of the current one.  The lm_head is scaled
    by 16 so that the top-2 gap of every visited position is far above the engine-vs-oracle logit bound.  Seed, scale and start tokens
    were searched on the CPU; everything the test relies on is asserted here, before any GPU work."""
    if not _CYCLIC:
        cfg = o.ModelConfig(kv_bits=8, **TINY)
        w = o.make_synthetic_weights(cfg, seed=CYC_SEED, quantized=False)
        for L in w['layers']:
            L['wo']['w'][:] = 0
            L['w2']['w'][:] = 0
        w['output'] = (w['output'].astype(np.float32) * CYC_SCALE).astype(np.float16)
        lg = o.lm_head(o.rmsnorm(w['tok_embeddings'], w['norm'], cfg.rms_eps), w['output']).astype(np.float32)
        nxt = lg.argmax(-1)
        top2 = np.sort(lg, -1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
        rng = np.random.default_rng(5)
        prompts = [np.concatenate([rng.integers(0, cfg.vocab, n), [s]]).astype(np.int32) for n, s in zip((4, 9), CYC_STARTS)]
        for p in prompts:
            seen, t, path = {}, int(p[-1]), []
            while t not in seen:
                seen[t] = len(path)
                path.append(t)
                t = int(nxt[t])
            tail, cyc = seen[t], len(path) - seen[t]
            assert tail <= 24 and cyc >= 8, (tail, cyc)                       # the cycle is entered within 24 tokens; a draft of 7 fits a period
            assert gap[path].min() > 6e-2, gap[path].min()
            assert not set(p[:-1].tolist()) & set(path)                       # the random prompt prefix is no part of the walk
        _CYCLIC.update(cfg=cfg, w=w, nxt=nxt, prompts=prompts)
    return _CYCLIC


@pytest.mark.parametrize('k,use_graph', [(1, 1), (3, 1), (3, 0), (7, 1)])
def test_decode_spec_cyclic_model(cuda, k, use_graph):
    m = _cyclic_model()
    cfg, nxt, prompts = m['cfg'], m['nxt'], m['prompts']
    sims = [sr.simulate(lambda h: nxt[h[-1]], p, nxt[p[-1]], CYC_MAX_NEW, k, 3, 1) for p in prompts]
    for out, per_step, drafted in sims:
        assert len(out) == CYC_MAX_NEW and max(per_step) == k + 1             # k + 1 tokens per step inside the cycle
    if k == 3:
        assert any(per_step[-1] >= 2 and drafted[-1] < k for _, per_step, drafted in sims)     # the run ends at max_new inside an accepted run
    eng = Engine.from_model_config(cfg, weight_type=1, max_batch_size=2, session_len=128, quant_policy=8, max_prefill_token_num=64,
                                   use_graph=use_graph)
    eng.load_weights(export_weights(cfg, m['w']))
    eng.start()
    try:
        eng.set_speculative(k, 3, 1)
        eng.prefill(prompts, max_new_tokens=CYC_MAX_NEW)
        toks, counts = eng.fetch_spec()
        per_step = [[] for _ in prompts]
        steps = max(len(s[1]) for s in sims)
        for _ in range(steps + 1):                                            # one step more: nothing is emitted past max_new
            eng.decode_spec(1)
            toks, new_counts = eng.fetch_spec()
            for b in range(len(prompts)):
                per_step[b].append(int(new_counts[b] - counts[b]))
            counts = new_counts
        stats = eng.spec_stats()
        eng.release()
    finally:
        eng.close()
    for b, (out, want_steps, drafted) in enumerate(sims):
        assert toks[b].tolist() == out, f'sequence {b}: tokens differ from the simulation'
        assert per_step[b] == want_steps + [0] * (steps + 1 - len(want_steps)), (b, per_step[b], want_steps)
    assert stats == dict(steps=sum(len(s[1]) for s in sims), drafted=sum(sum(s[2]) for s in sims),
                         accepted=sum(sum(s[1]) - len(s[1]) for s in sims), emitted=sum(sum(s[1]) for s in sims))
    print(f'[spec cyclic] k {k} graph {use_graph}: per-step emitted {per_step}')


def test_engine_spec_refusals(cuda):
    cfg = o.ModelConfig(kv_bits=8, **TINY)
    eng = Engine.from_model_config(cfg, max_batch_size=4, session_len=128, quant_policy=8, max_prefill_token_num=64)
    eng.init_synthetic(seed=1)
    eng.start()
    try:
        for bad in ((8, 3, 1), (-1, 3, 1), (3, 9, 1), (3, 2, 3), (3, 3, 0)):
            with pytest.raises(_ffi.TmError):
                eng.set_speculative(*bad)
        eng.set_speculative(3, 3, 1)
        prompts = [[1, 2, 3], [4, 5]]
        eng.set_sampling([(0.8, 40, 0.9, 0.0, 1)] * 2)
        with pytest.raises(_ffi.TmError, match='sampling'):
            eng.prefill(prompts, 8)
        eng.set_sampling(None)
        eng.set_logits_params([dict(repetition_penalty=1.2)] * 2)
        with pytest.raises(_ffi.TmError, match='logits processors'):
            eng.prefill(prompts, 8)
        eng.set_logits_params(None)
        eng.set_logprobs(2)
        with pytest.raises(_ffi.TmError, match='logprobs'):
            eng.prefill(prompts, 8)
        eng.set_logprobs(0)
        with pytest.raises(_ffi.TmError, match='continuous batching'):
            eng.submit([1, 2, 3], 4)
        with pytest.raises(_ffi.TmError, match='continuous batching'):
            eng.serve_start()
        eng.prefill(prompts, 8)
        with pytest.raises(_ffi.TmError):
            eng.set_speculative(0)                                            # a batch is admitted
        with pytest.raises(_ffi.TmError, match='n_draft'):
            eng.verify(np.zeros((2, 3), np.int32), [4, 0])
        with pytest.raises(_ffi.TmError, match='vocab'):
            eng.verify(np.full((2, 3), 1024, np.int32), [1, 1])
        eng.release()
        eng.set_speculative(0)                                                # off: the plain path again
        eng.prefill(prompts, 4)
        eng.decode(3)
        assert eng.fetch().shape == (2, 4)
        with pytest.raises(_ffi.TmError, match='without speculation'):
            eng.decode_spec(1)
        eng.release()
    finally:
        eng.close()
    cfg_w = o.ModelConfig(kv_bits=8, **TINY)
    mc = Engine.from_model_config(cfg_w, max_batch_size=2, session_len=128, quant_policy=42, max_prefill_token_num=64)
    mc.init_synthetic(seed=1)
    mc.start()
    try:
        with pytest.raises(_ffi.TmError, match='42'):
            mc.set_speculative(3, 3, 1)
    finally:
        mc.close()


# ---- (d) pipeline --------------------------------------------------------------------------------------------------------------------
def test_pipeline_speculative(cuda):
    cfg = TurbomindEngineConfig(max_batch_size=4, session_len=256, quant_policy=8)
    rng = np.random.default_rng(11)
    prompts = [(rng.integers(0, 1024, 6).tolist() * 6)[:n] for n in (36, 30, 24, 33)]      # repeated 6-grams: the lookup finds drafts
    max_new, k = 48, 3
    pipe = pipeline('synthetic:tiny', cfg, speculative_config=SpeculativeConfig('ngram', num_speculative_tokens=k))
    plain = pipeline('synthetic:tiny', cfg)
    try:
        g = GenerationConfig(max_new_tokens=max_new, ignore_eos=True)
        out = pipe(prompts, g)
        toks = [r.token_ids for r in out]
        assert all(r.generate_token_len == max_new == len(r.token_ids) and r.finish_reason == 'length' and r.input_token_len == len(p)
                   for r, p in zip(out, prompts))
        s1 = pipe.speculative_stats()
        assert s1['emitted'] == len(prompts) * (max_new - 1) == s1['accepted'] + s1['steps'] and s1['speculated_calls'] == 1
        assert s1['drafted'] >= s1['accepted'] > 0, s1                        # some drafts were accepted: there are accepted runs

        # the same batch step by step on the pipeline's engine: where the steps' boundaries are
        eng = pipe.engine
        eng.set_speculative(k, 3, 1)
        eng.prefill(prompts, max_new_tokens=max_new)
        counts, bounds = np.ones(len(prompts), np.int32), [[1] for _ in prompts]
        while (counts < max_new).any():
            eng.decode_spec(1)
            rep, counts = eng.fetch_spec()
            for b in range(len(prompts)):
                if bounds[b][-1] != counts[b]:
                    bounds[b].append(int(counts[b]))
        eng.release()
        assert [row.tolist() for row in rep] == toks                          # the kernels are deterministic
        # a stop id inside an accepted run: not the first token of its step, and seen for the first time there
        pick = [(b, p) for b in range(len(prompts)) for lo, hi in zip(bounds[b][:-1], bounds[b][1:]) for p in range(lo + 1, hi)
                if toks[b][p] not in toks[b][:p]]
        assert pick, 'no accepted run with a fresh token in it'
        b0, p0 = pick[0]
        stop = toks[b0][p0]
        out = pipe(prompts, GenerationConfig(max_new_tokens=max_new, ignore_eos=True, stop_token_ids=[stop]))
        for r, t in zip(out, toks):
            cut = t.index(stop) if stop in t else None
            assert r.token_ids == (t if cut is None else t[:cut]) and r.generate_token_len == len(r.token_ids)
            assert r.finish_reason == ('length' if cut is None else 'stop')
        assert out[b0].generate_token_len == p0

        # a sampling call runs the plain path: what the pipeline without speculation returns for the same seed
        gs = GenerationConfig(max_new_tokens=12, ignore_eos=True, do_sample=True, top_k=20, temperature=0.9, random_seed=3)
        before = pipe.speculative_stats()
        assert [r.token_ids for r in pipe(prompts, gs)] == [r.token_ids for r in plain(prompts, gs)]
        after = pipe.speculative_stats()
        assert after['steps'] == before['steps'] and after['plain_calls'] == before['plain_calls'] + 1
    finally:
        pipe.close()
        plain.close()
