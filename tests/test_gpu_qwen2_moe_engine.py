"""Qwen2-MoE through the engine and pipeline(): 60 experts, top-4 of a softmax over all experts, expert width 128, a shared expert
of width 384 behind its sigmoid gate in every layer, the Qwen2 attention prologue.  Logits within 3e-2 of Qwen2MoeOracleModel and
greedy tokens equal wherever the oracle's top-2 margin exceeds 6e-2 (the bounds of tests.qwen_reference.engine_vs_oracle; at least
two thirds of the (step, sequence) pairs must have that margin); a checkpoint on disk through pipeline(path); the start-up tuner.
The 3e-2 bound checks the wiring of the layer (slots, widths, buffers, capture); it is coarse for the shared term itself -- dropping
the term moves the reference's logits of this model by 8e-3 -- whose arithmetic tests/test_gpu_moe_shared.py pins at operator level."""
import numpy as np
import pytest

from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from tests.qwen2_moe_reference import (engine_vs_oracle_qwen2_moe, hf_qwen2_moe_tensors, parity_inputs, write_qwen2_moe_checkpoint)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('use_graph', [0, 1])
@pytest.mark.parametrize('fmt,kv_bits', [('u4', 8), ('u4', 4), ('fp8', 8)])
def test_qwen2_moe_engine_matches_oracle(cuda, fmt, kv_bits, use_graph):
    """prompts of 70 + 5 + 64 tokens with a 96-token prefill budget (two prefill iterations), then 6 teacher-forced decode steps"""
    worst = engine_vs_oracle_qwen2_moe(fmt, kv_bits, use_graph)
    print(f'{fmt} kv{kv_bits} graph {use_graph}: worst logit diff {worst:.4f}')


def test_qwen2_moe_engine_refusals(cuda):
    """a shared expert needs experts, and a per-rank width that is a multiple of 128"""
    from lmdeploy_amd import _ffi
    cfg, _, _ = parity_inputs('u4', 8)
    for bad in (dict(moe_experts=0, moe_top_k=0), dict(moe_shared_inter=192)):
        c = type(cfg)(**{**cfg.__dict__, **bad})
        with pytest.raises(_ffi.TmError, match='moe_shared_inter'):
            Engine.from_model_config(c, max_batch_size=1, session_len=64)


def test_qwen2_moe_checkpoint_through_pipeline(cuda, tmp_path):
    """tiny AWQ Qwen2-MoE checkpoint -> pipeline(path): batch, one-by-one and stream_infer through the scheduler (5 prompts, 3 slots:
    mixed steps) give the same greedy tokens, and they equal an Engine.from_model_config run on the weights read back"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    from lmdeploy_amd.turbomind import checkpoint
    rng = np.random.default_rng(22)
    H, Hq, Hkv, I, S, E, K, V = 256, 4, 2, 128, 384, 60, 4, 640
    hf = hf_qwen2_moe_tensors(rng, H, Hq, Hkv, I, S, E, V, layers=2)
    write_qwen2_moe_checkpoint(str(tmp_path), hf, H, Hq, Hkv, I, S, E, K, V, layers=2, fmt='awq')
    prompts = [rng.integers(3, V, n).astype(np.int32).tolist() for n in (19, 5, 40, 11, 27)]
    N = 6
    pipe = pipeline(str(tmp_path), backend_config=TurbomindEngineConfig(model_format='awq', quant_policy=8, max_batch_size=3,
                                                                        session_len=128))
    mcf = pipe.model_cfg
    assert (mcf.arch, mcf.moe_experts, mcf.moe_top_k, mcf.moe_shared_inter, mcf.attn_bias, mcf.qk_norm) == ('qwen2', E, K, S, 1, 0)
    g = GenerationConfig(max_new_tokens=N, ignore_eos=True)
    one = [pipe([p], g)[0].token_ids for p in prompts]
    assert all(len(t) == N for t in one)
    batch = [r.token_ids for r in pipe(prompts[:3], g)]
    assert batch == one[:3]
    streamed = sorted(pipe.stream_infer(prompts, g, stream_response=False), key=lambda r: r.index)
    assert [r.token_ids for r in streamed] == one
    pipe.close()

    mc = checkpoint.read_config(str(tmp_path))
    w = checkpoint.load_hf_weights(str(tmp_path), mc)
    eng = Engine.from_model_config(mc, max_batch_size=3, session_len=128, quant_policy=8)
    eng.load_weights(export_weights(mc, w))
    eng.start()
    eng.prefill([np.asarray(p, np.int32) for p in prompts[:3]], max_new_tokens=N)
    eng.decode(N - 1)
    toks = eng.fetch()
    eng.close()
    assert [list(map(int, toks[b, :N])) for b in range(3)] == one[:3]


@pytest.mark.parametrize('fmt', ['u4', 'fp8'])
def test_qwen2_moe_tune_gemm(cuda, tmp_path, fmt):
    """tm_engine_tune_gemm at the decode batch (3 rows) and at a 64-token forward on the parity model: the shared expert's w1w3 / w2
    (roles 3 / 4, width 384) are timed again on a MoE model -- w2 with the combine behind it --, the table is written (the lm_head's
    line is the one every run writes), and an engine that imports it gives identical tokens"""
    cfg, w, _ = parity_inputs(fmt, 8)
    weights = export_weights(cfg, w)
    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (40, 9, 15)]      # one 64-token prefill forward
    path = str(tmp_path / 'table.txt')

    def run(tune):
        eng = Engine.from_model_config(cfg, weight_type=2 if fmt == 'fp8' else 0, max_batch_size=3, session_len=128, quant_policy=8)
        eng.load_weights(weights)
        eng.start()
        if tune:
            eng.tune_gemm(3, path)
            eng.tune_gemm(64, path)
        else:
            eng.import_gemm_table(path)
        eng.prefill(prompts, max_new_tokens=4)
        eng.decode(3)
        toks = eng.fetch()
        eng.close()
        return toks
    tuned = run(True)
    lines = [ln.split() for ln in open(path).read().splitlines()]
    g = [x for x in lines if x and x[0] == 'G']
    assert any(x[1] == '17' and x[3] == '256' and x[4] == str(cfg.vocab) and x[5] == '3' for x in g), g   # the lm_head at the decode batch
    if fmt == 'fp8':      # dense e4m3 linears run the general kernel: the shared expert's roles 3 / 4 at width 384, both sizes
        for role, K, N in ((3, 256, 768), (4, 384, 256)):
            for M in (3, 64):
                assert any(x[1:6] == ['18', str(role), str(K), str(N), str(M)] for x in g), (role, K, N, M, g)
    imported = run(False)
    assert np.array_equal(tuned, imported)
