"""The gpt-oss MoE block through the engine and the pipeline: a 2-layer model with fp16 attention linears (weight_type 1), MXFP4 experts
(moe_expert_format 3) with biases, a router bias and the gpt-oss activation, int8 KV.  Prefill (two iterations under a 96-token
budget) plus 3 teacher-forced decode steps, eager and under the captured graph, against tests.mxfp4_reference.GptOssMoeOracleModel
with the bounds of tests/test_gpu_moe_f16_engine.py: logits within 3e-2, greedy tokens equal wherever the oracle's top-2 margin
exceeds 6e-2.  The synthetic pipeline model generates the tokens of an Engine driven directly; tp = 2 is refused."""
import numpy as np
import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind.engine import Engine, make_model_config
from lmdeploy_amd.turbomind.loader import export_weights
from tests.mxfp4_reference import GPTOSS_MOE_CFG, GptOssMoeConfig, GptOssMoeOracleModel, make_gptoss_weights

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
F16 = 1      # TM_WEIGHT_F16: the attention linears and the lm_head


@pytest.mark.parametrize('use_graph', [0, 1])
def test_gptoss_moe_engine_matches_oracle(cuda, use_graph, prompt_lens=(70, 5, 64), steps=3, session_len=256):
    cfg = GptOssMoeConfig(**GPTOSS_MOE_CFG)
    w = make_gptoss_weights(cfg, seed=3)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in prompt_lens]
    eng = Engine.from_model_config(cfg, weight_type=F16, max_batch_size=len(prompts), session_len=session_len, quant_policy=8,
                                   max_prefill_token_num=96, use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits().copy()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    eng.close()
    om = GptOssMoeOracleModel(cfg, w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(f32) - lg.astype(f32))
        print(f'gpt-oss moe graph {use_graph} step {s}: max logit diff {d.max():.4f}, |logit| max {np.abs(lg.astype(f32)).max():.3f}')
        assert d.max() <= 3e-2, f'step {s}: max logit diff {d.max()}'
        top2 = np.sort(lg.astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ids[safe]), f'step {s}: greedy tokens differ'
        if s < steps:
            ids, lg = om.forward([[int(t)] for t in toks[:, s]])


def test_synthetic_pipeline_generates_the_engines_tokens(cuda):
    """pipeline('synthetic:tiny_gptoss_moe', model_format='hf'): tm_engine_init_synthetic fills the MXFP4 expert, bias and router-bias
    slots; the pipeline's greedy tokens are those of an Engine on the same config and seed driven by prefill / decode"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    prompts = [list(range(3, 20)), list(range(40, 44))]
    pipe = pipeline('synthetic:tiny_gptoss_moe', backend_config=TurbomindEngineConfig(model_format='hf', max_batch_size=2,
                                                                                     session_len=128, quant_policy=8))
    try:
        mc = pipe.model_cfg
        assert (mc.moe_experts, mc.moe_top_k, mc.weight_format, mc.moe_expert_format, mc.moe_act, mc.moe_bias) == (8, 2, 'f16', 3, 1, 1)
        got = [r.token_ids for r in pipe(prompts, GenerationConfig(max_new_tokens=5, ignore_eos=True))]
    finally:
        pipe.close()
    assert all(len(t) == 5 for t in got)
    eng = Engine.from_model_config(mc, weight_type=F16, max_batch_size=2, session_len=128, quant_policy=8)
    try:
        eng.init_synthetic(seed=0)
        eng.start()
        eng.prefill([np.asarray(p, np.int32) for p in prompts], max_new_tokens=5)
        eng.decode(4)
        toks = eng.fetch()
    finally:
        eng.close()
    assert [list(map(int, t[:5])) for t in toks] == got
    assert len({tuple(t) for t in got}) == 2, 'two prompts, two continuations'


def test_tune_gemm_covers_the_mxfp4_grouped_gemms(cuda, tmp_path):
    """tm_engine_tune_gemm on an engine with MXFP4 experts: the row tiles of both grouped expert GEMMs are timed (table kind
    kGenGrouped + 3) and the tuned engine generates the tokens of the untuned one (a row's sum does not depend on the tile height)"""
    from lmdeploy_amd.pipeline import SYNTHETIC
    from lmdeploy_amd.turbomind import checkpoint
    mc = checkpoint.ModelConfig(**SYNTHETIC['tiny_gptoss_moe'], quantized=False, weight_format='f16')
    prompts = [np.arange(3, 20, dtype=np.int32), np.arange(40, 44, dtype=np.int32)]
    toks = []
    for tune in (0, 1):
        eng = Engine.from_model_config(mc, weight_type=F16, max_batch_size=16, session_len=128, quant_policy=8)
        try:
            eng.init_synthetic(seed=0)
            eng.start()
            if tune:
                # the export is the PROCESS's table (other tests' engines have tuned into it): what this call adds is the difference
                Engine.export_gemm_table(str(tmp_path / 'before.txt'))
                before = set((tmp_path / 'before.txt').read_text().splitlines())
                eng.tune_gemm(16, str(tmp_path / 'table.txt'))
                final = (tmp_path / 'table.txt').read_text().splitlines()
                added = [ln.split() for ln in final if ln not in before]
                grouped = [x for x in added if x[0] == 'G' and 32 <= int(x[1]) <= 35]
                # a grouped entry is written only where a tile beats the launcher's rule by 7 %: none, or entries of the MXFP4 kind for
                # this model's expert linears (w1w3 256 x 256, w2 128 x 256) at the 16-row bucket with a legal tile
                for x in grouped:
                    assert x[1] == '35' and (x[3], x[4]) in (('256', '256'), ('128', '256')) and x[5] == '16' and x[6] in ('16', '32', '64'), added
                rows = _ffi.C.c_int(-1)
                for K in (256, 128):
                    _ffi.check(_ffi.load().tm_debug_grouped_tile(3, K, 256, 16, _ffi.C.byref(rows)))
                    want = [int(x[6]) for x in map(str.split, final) if x[:6] == ['G', '35', '0', str(K), '256', '16']]
                    assert rows.value == (want[0] if want else 0), (K, rows.value, grouped)
            eng.prefill(prompts, max_new_tokens=4)
            eng.decode(3)
            toks.append(eng.fetch()[:, :4].copy())
        finally:
            eng.close()
    assert np.array_equal(toks[0], toks[1])
    _ffi.check(_ffi.load().tm_gemm_import(str(tmp_path / 'table.txt').encode()))      # every line the tuner wrote is accepted back


def test_tp2_with_mxfp4_experts_is_refused(cuda):
    cfg = GptOssMoeConfig(**GPTOSS_MOE_CFG)
    h = _ffi.C.c_void_p()
    ec = _ffi.EngineConfig(make_model_config(cfg, F16), 2, 0, 0, 2, 128, 8, 64, 0.5, 0, 96, 0, 1)
    rc = _ffi.load().tm_engine_create(_ffi.C.byref(h), _ffi.C.byref(ec))
    assert rc != 0 and not h.value
    assert 'tp > 1 are not built' in _ffi.last_error() and 'MXFP4' in _ffi.last_error()
