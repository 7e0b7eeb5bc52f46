"""GPU tests of prompt scoring: tm_engine_score (Engine.score) against the oracle model's lm_head over every prompt row, chunked
prefill and a lm_head chunk boundary inside a sequence, no trace left in the engine, full-size self-consistency with the prefill head,
and Pipeline.get_ppl.

Per-token bound 6e-2: the NLL is 2-Lipschitz in the max-norm of the logits, and the engine's logit gate against the oracle is 3e-2."""
import numpy as np
import pytest

from lmdeploy_amd import TurbomindEngineConfig, _ffi
from lmdeploy_amd.pipeline import Pipeline
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)
EPS = float(np.float32(1e-9))


def nll_rows(logits16, targets):
    """float64 NLL of every row against its target (the reference's formula, max from -FLT_MAX)"""
    x = np.asarray(logits16).astype(np.float64)
    m = np.maximum(x.max(axis=1), -FLT_MAX)
    s = np.exp(x - m[:, None]).sum(axis=1)
    return np.log(s + EPS) + m - x[np.arange(len(x)), np.asarray(targets)]


def oracle_nll(cfg, w, prompts, max_ctx):
    om = o.OracleModel(cfg, w, batch=len(prompts), max_ctx=max_ctx)
    om.forward(prompts)
    lg = o.lm_head(o.rmsnorm(om.last_resid, w['norm'], cfg.rms_eps), w['output'])
    out, off = [], 0
    for p in prompts:
        n = len(p)
        out.append(nll_rows(lg[off:off + n - 1], np.asarray(p[1:])))
        off += n
    return out


def tiny_cfg(kv_bits):
    return o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, kv_bits=kv_bits,
                         rope=o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192))


def check_against_oracle(got, ref, what):
    assert [len(g) for g in got] == [len(r) for r in ref]
    d = max(float(np.max(np.abs(g.astype(np.float64) - r))) for g, r in zip(got, ref))
    print(f'{what}: max per-token NLL diff {d:.4f}')
    assert d <= 6e-2, what


@pytest.mark.parametrize('kv_bits', [8, 4, 16])
def test_engine_score_matches_oracle(cuda, kv_bits):
    """lengths (70, 5, 64, 2) with 96 tokens per prefill forward: chunk boundaries inside sequences, the boundary row's target is the
    first token of the next forward"""
    cfg = tiny_cfg(kv_bits)
    w = o.make_synthetic_weights(cfg, seed=3)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (70, 5, 64, 2)]
    eng = Engine.from_model_config(cfg, max_batch_size=4, session_len=256, quant_policy=0 if kv_bits == 16 else kv_bits,
                                   max_prefill_token_num=96)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    got = eng.score(prompts)
    again = eng.score(prompts)
    eng.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again))
    assert all(g.dtype == np.float32 for g in got)
    check_against_oracle(got, oracle_nll(cfg, w, prompts, 256), f'kv {kv_bits}')


@pytest.mark.parametrize('fmt', ['fp8', 'u4'])
def test_engine_score_moe_matches_oracle(cuda, fmt):
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=256, vocab=512, kv_bits=8,
                        rope=o.RopeParam(128, 1000000.0, 'default', 1.0, 1.0, 4.0, 8192), weight_format=fmt,
                        moe_experts=4, moe_top_k=2, moe_fp8_act=True)
    w = o.make_synthetic_weights(cfg, seed=5)
    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (70, 9, 33)]
    eng = Engine.from_model_config(cfg, weight_type=2 if fmt == 'fp8' else 0, max_batch_size=3, session_len=128, quant_policy=8,
                                   max_prefill_token_num=64)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    got = eng.score(prompts)
    eng.close()
    check_against_oracle(got, oracle_nll(cfg, w, prompts, 128), f'moe {fmt}')


def test_engine_score_crosses_lm_head_chunk(cuda):
    """1500 rows in one forward: two lm_head chunks of at most 1024 rows"""
    cfg = tiny_cfg(8)
    w = o.make_synthetic_weights(cfg, seed=4)
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, cfg.vocab, 1500).astype(np.int32)]
    eng = Engine.from_model_config(cfg, max_batch_size=1, session_len=2048, quant_policy=8, max_prefill_token_num=2048)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    got = eng.score(prompts)
    eng.close()
    check_against_oracle(got, oracle_nll(cfg, w, prompts, 2048), '1500 tokens')


def _generate(eng, prompts):
    eng.prefill(prompts, max_new_tokens=4)
    lg = [eng.fetch_logits().copy()]
    for _ in range(3):
        eng.decode(1)
        lg.append(eng.fetch_logits().copy())
    toks = eng.fetch().copy()
    eng.release()
    return toks, lg


def test_engine_score_leaves_no_trace(cuda):
    cfg = tiny_cfg(8)
    w = o.make_synthetic_weights(cfg, seed=6)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (40, 17)]
    other = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (100, 3, 60)]
    engines = []
    for _ in range(2):
        e = Engine.from_model_config(cfg, max_batch_size=4, session_len=256, quant_policy=8, max_prefill_token_num=96)
        e.load_weights(export_weights(cfg, w))
        e.start()
        engines.append(e)
    fresh, used = engines
    used.score(other)
    ref_toks, ref_lg = _generate(fresh, prompts)
    toks, lg = _generate(used, prompts)
    assert np.array_equal(toks, ref_toks)
    assert all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(lg, ref_lg))
    used.score(other)                                    # after a graph-replayed decode, too
    toks2, lg2 = _generate(used, prompts)
    assert np.array_equal(toks2, ref_toks)
    assert all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(lg2, ref_lg))
    used.prefill(prompts, max_new_tokens=2)
    with pytest.raises(_ffi.TmError):
        used.score(other)
    used.release()
    with pytest.raises(_ffi.TmError) as ei:
        used.score([other[0][:1]])
    assert ei.value.status == 1
    with pytest.raises(_ffi.TmError) as ei:
        used.score([np.zeros(256, np.int32)])
    assert ei.value.status == 6
    with pytest.raises(_ffi.TmError) as ei:
        used.score([np.asarray([1, cfg.vocab], np.int32)])
    assert ei.value.status == 1
    for e in engines:
        e.close()


def test_score_fullsize_matches_prefill_head(cuda):
    """synthetic Llama-3-8B (vocab 128 256): the score of token t behind a 1500-token prompt equals the NLL of t computed from the
    prefill head's logits of that prompt (different GEMM tilings on the two sides)"""
    pipe = Pipeline('synthetic:llama3_8b', backend_config=TurbomindEngineConfig(max_batch_size=1, session_len=2048, quant_policy=8,
                                                                                 max_prefill_token_num=2048))
    try:
        rng = np.random.default_rng(4)
        p = rng.integers(0, 128256, 1500).astype(np.int32)
        t = 4242
        got = pipe.engine.score([np.concatenate([p, [t]]).astype(np.int32)])[0]
        assert got.shape == (1500,)
        pipe.engine.prefill([p], max_new_tokens=1)
        lg = pipe.engine.fetch_logits()
        pipe.engine.release()
        ref = nll_rows(lg, [t])[0]
        print(f'full size: score {got[-1]:.5f} prefill head {ref:.5f}')
        assert abs(float(got[-1]) - ref) <= 1e-2
        assert np.all(np.isfinite(got))
    finally:
        pipe.close()


def test_pipeline_get_ppl(cuda):
    pipe = Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(max_batch_size=4, session_len=512, quant_policy=8,
                                                                            max_prefill_token_num=256))
    try:
        rng = np.random.default_rng(9)
        seqs = [rng.integers(0, 1024, n).tolist() for n in (2, 300, 17, 64, 5, 129, 2, 250, 33)]
        res = pipe.get_ppl(seqs)
        assert len(res) == 9 and all(type(r) is float for r in res)
        singles = [pipe.get_ppl(s)[0] for s in seqs]
        for s, r1 in zip(seqs, singles):
            nll = pipe.engine.score([s])[0]
            assert r1 == float(np.cumsum(nll, dtype=np.float64)[-1] / (len(s) - 1))
        d = np.abs(np.asarray(res) - np.asarray(singles))
        print(f'get_ppl batched vs single: max diff {d.max():.2e}')
        assert d.max() <= 1e-3
    finally:
        pipe.close()
