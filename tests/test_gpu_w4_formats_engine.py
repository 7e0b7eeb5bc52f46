"""W4A16 dialects through the engine and pipeline().

Group 128: a GPTQ and a compressed-tensors directory hold the same (q, s, z) as the AWQ directory, the loader turns all three into the
same slots, so the engine's logits and greedy tokens are bit-identical -- tiny Llama and tiny Qwen3-MoE, eager and graph-replayed.
Group 32 (compressed-tensors, gemm_u4_g32.hip): a tiny dense Llama with head_dim 128 and one with head_dim 64, prefill + 8 decode steps
against the oracle forward with group = 32, the bound of tests/test_gpu_engine.py::test_engine_matches_oracle (3e-2 on the logits, equal
greedy tokens where the reference's margin exceeds 6e-2), fp16 and int8 KV."""
import numpy as np
import pytest

from tests import w4_formats_reference as r

pytestmark = pytest.mark.gpu
f32 = np.float32
_DIRS, _RUNS = {}, {}
PROMPT_LENS = (70, 5, 33)


def _dir(tmp_path_factory, kind, dialect, group=128, D=128):
    key = (kind, dialect, group, D)
    if key not in _DIRS:
        path = str(tmp_path_factory.mktemp(f'w4_{kind}_{dialect.replace("-", "_")}_{group}_{D}'))
        if ('model', kind, group, D) not in _DIRS:
            _DIRS[('model', kind, group, D)] = r.make_model(kind, group, seed=5, D=D)
        model = _DIRS[('model', kind, group, D)]
        r.write_model(path, model, dialect)
        _DIRS[key] = (path, model)
    return _DIRS[key]


def _engine_run(path, quant_policy, use_graph, steps):
    """read_config / load_hf_weights / export_weights -> Engine: ragged prompts in forwards of <= 96 tokens, then `steps` decode steps"""
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights
    cfg = checkpoint.read_config(path)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in PROMPT_LENS]
    eng = Engine.from_model_config(cfg, max_batch_size=len(prompts), session_len=128, quant_policy=quant_policy, max_prefill_token_num=96,
                                   use_graph=use_graph)
    try:
        eng.load_weights(export_weights(cfg, checkpoint.load_hf_weights(path, cfg)))
        eng.start()
        eng.prefill(prompts, max_new_tokens=steps + 1)
        logits = [eng.fetch_logits().copy()]
        for _ in range(steps):
            eng.decode(1)
            logits.append(eng.fetch_logits().copy())
        toks = eng.fetch().copy()
    finally:
        eng.close()
    return cfg, prompts, logits, toks


@pytest.mark.parametrize('use_graph', [0, 1], ids=['eager', 'graph'])
@pytest.mark.parametrize('kind', ['llama', 'qwen3_moe'])
def test_group_128_dialects_are_bit_identical(cuda, tmp_path_factory, kind, use_graph):
    runs = {}
    for d in r.DIALECTS:
        path, _ = _dir(tmp_path_factory, kind, d)
        cfg, _, logits, toks = _engine_run(path, 8, use_graph, 3)
        assert cfg.w4_dialect == d and cfg.group == 128
        runs[d] = (logits, toks)
    for d in ('gptq', 'compressed-tensors'):
        assert np.array_equal(runs[d][1], runs['awq'][1]), f'{d}: greedy tokens differ from the AWQ directory'
        for s, (a, b) in enumerate(zip(runs['awq'][0], runs[d][0])):
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), f'{d} step {s}: logits differ from the AWQ directory'
    lg = np.stack(runs['awq'][0]).astype(f32)
    assert np.isfinite(lg).all() and lg.std() > 1e-3


def test_pipeline_detects_the_dialect(cuda, tmp_path_factory):
    """pipeline('/path') with model_format=None on the three directories: the same tokens; model_format='compressed-tensors' is accepted
    on its directory and 'awq' on a GPTQ directory is the mismatch error"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    rng = np.random.default_rng(21)
    prompts = [rng.integers(3, 500, n).astype(np.int32).tolist() for n in (19, 5)]
    got = {}
    for d, fmt in (('awq', None), ('gptq', None), ('compressed-tensors', 'compressed-tensors')):
        path, _ = _dir(tmp_path_factory, 'llama', d)
        pipe = pipeline(path, backend_config=TurbomindEngineConfig(model_format=fmt, quant_policy=8, max_batch_size=2, session_len=128))
        try:
            assert pipe.model_cfg.w4_dialect == d
            got[d] = [x.token_ids for x in pipe(prompts, GenerationConfig(max_new_tokens=4, ignore_eos=True))]
        finally:
            pipe.close()
    assert got['gptq'] == got['awq'] and got['compressed-tensors'] == got['awq']
    with pytest.raises(ValueError, match='gptq'):
        pipeline(_dir(tmp_path_factory, 'llama', 'gptq')[0], backend_config=TurbomindEngineConfig(model_format='awq', max_batch_size=2,
                                                                                                  session_len=128))


@pytest.mark.parametrize('quant_policy', [0, 8], ids=['kv16', 'kv8'])
@pytest.mark.parametrize('D', [128, 64])
def test_group_32_engine_matches_oracle(cuda, tmp_path_factory, D, quant_policy):
    from tests.qwen_reference import QwenOracleModel
    steps = 8
    path, model = _dir(tmp_path_factory, 'llama', 'compressed-tensors', 32, D)
    cfg, prompts, logits, toks = _engine_run(path, quant_policy, 1, steps)
    assert cfg.group_size == 32 and cfg.head_dim == D
    oc, w = r.dense_oracle(model, 16 if quant_policy == 0 else quant_policy)
    om = QwenOracleModel(oc, w, batch=len(prompts), max_ctx=128)
    ids, lg = om.forward(prompts)
    ref_logits, ref_toks = [lg], [ids]
    for s in range(steps):
        ids, lg = om.forward([[int(t)] for t in toks[:, s]])      # teacher-forced with the engine's tokens
        ref_logits.append(lg)
        ref_toks.append(ids)
    worst = 0.0
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s].astype(f32))
        worst = max(worst, float(d.max()))
        print(f'g32 head_dim {D} qp {quant_policy} step {s}: max logit diff {d.max():.4g}')
        assert d.max() <= 3e-2, f'step {s}: max logit diff {d.max()}'
        top2 = np.sort(ref_logits[s].astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ref_toks[s][safe]), f'step {s}: greedy tokens differ'
    print(f'g32 head_dim {D} qp {quant_policy}: max logit diff over {steps + 1} steps {worst:.4g} (bound 3e-2)')
