"""Unquantised (fp16) MoE models through the engine (weight_type 1): every linear -- attention, experts, the shared expert -- is an
fp16 [K][N] `.weight` slot, the experts run on the grouped fp16 GEMM.  Tiny synthetic models (2 layers, H 256, head_dim 128,
expert width 128): Qwen3-MoE style with 8 experts / top-2 (the serial router) and 72 / top-8 (the wide one), and Qwen2-MoE style
with a shared expert of width 128.  Prefill (two iterations under a 96-token budget) plus teacher-forced decode steps against the
oracle models of tests.qwen_moe_reference / tests.qwen2_moe_reference on the same fp16 weights, with the bounds of
tests.test_gpu_qwen_moe_engine: logits within 3e-2, greedy tokens equal wherever the oracle's top-2 margin exceeds 6e-2."""
from dataclasses import replace

import numpy as np
import pytest

from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests.linear_bytes import engine_weight_bytes
from tests.qwen2_moe_reference import QWEN2_MOE_CFG, Qwen2MoeConfig, Qwen2MoeOracleModel
from tests.qwen_moe_reference import QWEN3_MOE_CFG, QwenMoeConfig, QwenMoeOracleModel
from tests.qwen_reference import make_qwen_weights

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
F16 = 1      # TM_WEIGHT_F16


def _qwen3_moe(E, k):
    cfg = QwenMoeConfig(**dict(QWEN3_MOE_CFG, moe_experts=E, moe_top_k=k), kv_bits=8)
    return cfg, make_qwen_weights(cfg, seed=3, quantized=False), QwenMoeOracleModel


def _qwen2_moe():
    """tests.qwen2_moe_reference.make_qwen2_moe_weights without the quantisation: 8 experts / top-2 of a softmax over all experts,
    a shared expert of width 128 drawn like every other linear, its gate [H] ~ 0.2 N(0, 1)"""
    cfg = Qwen2MoeConfig(**dict(QWEN2_MOE_CFG, moe_experts=8, moe_top_k=2, moe_shared_inter=128), kv_bits=8)
    w = make_qwen_weights(cfg, seed=3, quantized=False)
    dense = o.make_synthetic_weights(replace(cfg, moe_experts=0, moe_top_k=0, inter=cfg.moe_shared_inter), 104732, quantized=False)
    rng = np.random.default_rng(15485866)
    for L, Ld in zip(w['layers'], dense['layers']):
        L['w1w3'], L['w2'] = Ld['w1w3'], Ld['w2']
        L['shared_gate'] = (0.2 * rng.standard_normal(cfg.hidden)).astype(f16)
    return cfg, w, Qwen2MoeOracleModel


def _engine_vs_oracle(cfg, w, oracle_cls, use_graph, prompt_lens=(70, 5, 64), steps=3, session_len=256):
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in prompt_lens]
    eng = Engine.from_model_config(cfg, weight_type=F16, max_batch_size=len(prompts), session_len=session_len, quant_policy=8,
                                   max_prefill_token_num=96, use_graph=use_graph)
    slots = export_weights(cfg, w)
    for li in range(cfg.layers):
        for x in (0, cfg.moe_experts - 1):      # fp16 [K][N], no scales / zeros slots
            q = f'layers.{li}.moe_ffn.experts.{x}'
            assert slots[q + '.w1w3.weight'].shape == (cfg.hidden, 2 * cfg.inter) and slots[q + '.w1w3.weight'].dtype == f16
            assert slots[q + '.w2.weight'].shape == (cfg.inter, cfg.hidden)
            assert q + '.w1w3.scales' not in slots and q + '.w2.qweight' not in slots
    eng.load_weights(slots)
    eng.start()
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits().copy()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    weight_bytes = eng.stats()['weight_bytes']
    eng.close()
    om = oracle_cls(cfg, w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    worst = 0.0
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(f32) - lg.astype(f32))
        worst = max(worst, float(d.max()))
        print(f'f16 experts {cfg.moe_experts} graph {use_graph} step {s}: max logit diff {d.max():.4f}')
        assert d.max() <= 3e-2, f'step {s}: max logit diff {d.max()}'
        top2 = np.sort(lg.astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ids[safe]), f'step {s}: greedy tokens differ'
        if s < steps:
            ids, lg = om.forward([[int(t)] for t in toks[:, s]])
    assert weight_bytes == engine_weight_bytes(cfg, 'f16')
    return worst


@pytest.mark.parametrize('use_graph', [0, 1])
def test_f16_moe_engine_matches_oracle(cuda, use_graph):
    """8 experts, top-2, the Qwen3 prologue: prompts of 70 + 5 + 64 tokens, then 3 teacher-forced decode steps, eager and graph"""
    _engine_vs_oracle(*_qwen3_moe(8, 2), use_graph)


def test_f16_moe_engine_72_experts(cuda):
    """72 experts, top-8 (the wide router; most experts see no row of a decode step)"""
    _engine_vs_oracle(*_qwen3_moe(72, 8), 1)


def test_f16_qwen2_moe_engine_shared_expert(cuda):
    """Qwen2-MoE style: q / k / v bias, a dense fp16 shared expert of width 128 behind its sigmoid gate next to the routed experts"""
    _engine_vs_oracle(*_qwen2_moe(), 1)


def test_f16_moe_synthetic_pipeline_generates(cuda):
    """pipeline('synthetic:tiny_moe', model_format='hf'): tm_engine_init_synthetic fills the fp16 expert slots and the pipeline
    generates -- the same greedy tokens for a prompt alone and in a batch"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    pipe = pipeline('synthetic:tiny_moe', backend_config=TurbomindEngineConfig(model_format='hf', max_batch_size=2, session_len=128,
                                                                              quant_policy=8))
    try:
        assert (pipe.model_cfg.moe_experts, pipe.model_cfg.moe_top_k, pipe.model_cfg.weight_format) == (8, 2, 'f16')
        g = GenerationConfig(max_new_tokens=5, ignore_eos=True)
        prompts = [list(range(3, 20)), list(range(40, 44))]
        one = [pipe([p], g)[0].token_ids for p in prompts]
        assert all(len(t) == 5 for t in one)
        assert [r.token_ids for r in pipe(prompts, g)] == one
    finally:
        pipe.close()
