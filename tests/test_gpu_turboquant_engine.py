"""quant_policy 42 (TurboQuant KV cache) end to end: the engine against the oracle model running on the reference's TurboQuant cache
(tests/turboquant_reference.py), continuous batching against the static batch, and pipeline().

The engine's K / V rows differ from the oracle's by fp16 ulps (GEMM accumulation order), so a value next to a decision boundary may
take the neighbouring code in one of the two -- and a flipped 2-bit code moves a value further (cell width about 1.0 sigma) than a
flipped int4 code (step about 0.37 sigma).  The test prints the worst logit difference of the int4 arm of the same run next to it."""
import numpy as np
import pytest

import lmdeploy_amd
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests import turboquant_reference as tq

pytestmark = pytest.mark.gpu


def _run(cfg, w, prompts, steps, quant_policy, use_graph, tq_cache):
    """test_engine_matches_oracle's procedure: teacher-forced, worst logit difference and the greedy-token check"""
    eng = Engine.from_model_config(cfg, max_batch_size=4, session_len=256, quant_policy=quant_policy, max_prefill_token_num=96,
                                    use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits())
    toks = eng.fetch()
    eng.close()

    om = o.OracleModel(cfg, w, batch=len(prompts), max_ctx=256)
    if tq_cache:    # the oracle's data flow on the TurboQuant cache: it only duck-types store_token / load_dequant / layout
        om.cache = tq.TqPagedKVCache(tq.TqBlockLayout(cfg.layers, cfg.kv_heads), om.cache.pool.shape[0])
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
        top2 = np.sort(ref_logits[s].astype(np.float32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ref_toks[s][safe]), f'step {s}: greedy tokens differ'
    return worst


@pytest.mark.parametrize('use_graph', [0, 1])
def test_engine_matches_oracle_turboquant(cuda, use_graph):
    """3 ragged prompts (70, 5, 64), 6 decode steps, eager and graph-replayed; bound: the project's 3e-2 on O(1) logits"""
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024,
                        kv_bits=4, rope=o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192))
    w = o.make_synthetic_weights(cfg, seed=3)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (70, 5, 64)]
    worst42 = _run(cfg, w, prompts, 6, 42, use_graph, True)
    worst4 = _run(cfg, w, prompts, 6, 4, use_graph, False)
    print(f'[engine vs oracle] graph {use_graph}: max logit diff over 7 steps: quant_policy 42 {worst42:.5f}, quant_policy 4 {worst4:.5f}')
    assert worst42 <= 3e-2, f'max logit diff {worst42} (int4 arm of the same run: {worst4})'


def test_continuous_batching_matches_static_turboquant(cuda):
    """5 requests through 2 batch slots: tokens equal the static single-prompt run up to the first position whose top-2 margin is below
    5e-2 (prompts share prefill iterations, so GEMM shapes differ in the last fp32 bits)"""
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024,
                        kv_bits=4, rope=o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192))
    w = o.make_synthetic_weights(cfg, seed=11)
    rng = np.random.default_rng(4)
    lens, news = [70, 5, 64, 33, 9], [6, 8, 3, 5, 7]
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in lens]
    eng = Engine.from_model_config(cfg, max_batch_size=2, session_len=256, quant_policy=42, max_prefill_token_num=96)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    ref, margin = [], []
    for p, n in zip(prompts, news):
        eng.prefill([p], max_new_tokens=n)
        mg = []
        for k in range(n):
            top2 = np.sort(eng.fetch_logits()[0].astype(np.float32))[-2:]
            mg.append(float(top2[1] - top2[0]))
            if k + 1 < n:
                eng.decode(1)
        ref.append(eng.fetch()[0].copy())
        margin.append(mg)
        eng.release()
    ids = [eng.submit(p, n, -1) for p, n in zip(prompts, news)]
    done, steps = {}, 0
    while len(done) < len(ids):
        na, _ = eng.step()
        assert na <= 2
        steps += 1
        assert steps < 200, 'scheduler does not make progress'
        for i, rid in enumerate(ids):
            if i not in done:
                status, toks = eng.poll(rid)
                if status != 0:
                    done[i] = (status, toks.copy())
    for i, (status, toks) in done.items():
        assert status == 7 and len(toks) == news[i]
        for k in range(news[i]):
            if toks[k] != ref[i][k]:
                assert margin[i][k] < 5e-2, f'request {i} token {k}: {toks} vs {ref[i]} (margin {margin[i][k]})'
                break
    eng.release()
    eng.close()


def test_pipeline_turboquant(cuda):
    pipe = lmdeploy_amd.pipeline('synthetic:tiny', backend_config=lmdeploy_amd.TurbomindEngineConfig(quant_policy=42, session_len=256,
                                                                                                      max_batch_size=2))
    ps = [list(range(5, 40)), list(range(100, 103)), list(range(7, 90))]
    gen = lmdeploy_amd.GenerationConfig(max_new_tokens=5, ignore_eos=True)
    a, b = pipe(ps, gen), pipe(ps, gen)
    assert [r.token_ids for r in a] == [r.token_ids for r in b]
    assert all(r.generate_token_len == 5 and r.finish_reason == 'length' for r in a)
    withl = pipe(ps, lmdeploy_amd.GenerationConfig(max_new_tokens=5, ignore_eos=True, output_logits='generation'))
    for r in withl:
        assert r.logits.shape == (5, 1024) and np.isfinite(r.logits).all()
        assert r.logits.argmax(-1).tolist() == r.token_ids
    ppl = pipe.get_ppl(ps)
    assert len(ppl) == 3 and np.isfinite(np.asarray(ppl, np.float64)).all()
    pipe.close()


@pytest.mark.parametrize('model,reason', [('synthetic:gpt_oss_20b', 'head_dim 64'), ('synthetic:tiny_window', 'sliding window')])
def test_pipeline_refuses_by_name(model, reason):
    """a head_dim-64 or windowed model with quant_policy=42 raises with the reason before anything is allocated"""
    with pytest.raises(NotImplementedError, match=reason):
        lmdeploy_amd.pipeline(model, backend_config=lmdeploy_amd.TurbomindEngineConfig(quant_policy=42, session_len=256, model_format='hf'))
