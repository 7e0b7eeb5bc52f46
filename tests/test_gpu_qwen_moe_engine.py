"""Qwen3-MoE through the engine and pipeline(): 72 experts (above the serial router's 64), top-8, the Qwen3 attention prologue.
Logits within 3e-2 of QwenMoeOracleModel and greedy tokens equal wherever the oracle's top-2 margin exceeds 6e-2 (the bounds of
tests.qwen_reference.engine_vs_oracle); a checkpoint on disk through pipeline(path); the start-up tuner at 128 experts."""
import numpy as np
import pytest

from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests.qwen_moe_reference import (QWEN3_MOE_CFG, QwenMoeConfig, engine_vs_oracle_moe, hf_qwen_moe_tensors, make_qwen_moe_weights,
                                      write_qwen_moe_checkpoint)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('use_graph', [0, 1])
@pytest.mark.parametrize('kv_bits', [8, 4])
@pytest.mark.parametrize('fmt', ['u4', 'fp8'])
def test_qwen3_moe_engine_matches_oracle(cuda, fmt, kv_bits, use_graph):
    """prompts of 70 + 5 + 64 tokens with a 96-token prefill budget (two prefill iterations), then 6 teacher-forced decode steps"""
    worst = engine_vs_oracle_moe(fmt, kv_bits, use_graph)
    print(f'{fmt} kv{kv_bits} graph {use_graph}: worst logit diff {worst:.4f}')


def test_qwen3_moe_checkpoint_through_pipeline(cuda, tmp_path):
    """tiny AWQ Qwen3-MoE checkpoint -> pipeline(path): loads, generates greedily, the same tokens as an Engine.from_model_config
    engine fed the weights read from the same checkpoint; stream_infer through the scheduler (5 prompts, 3 slots) gives the same"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    from lmdeploy_amd.turbomind import checkpoint
    rng = np.random.default_rng(21)
    H, Hq, Hkv, I, E, K, V = 256, 4, 2, 128, 72, 8, 640
    hf = hf_qwen_moe_tensors(rng, H, Hq, Hkv, I, E, V, layers=2)
    write_qwen_moe_checkpoint(str(tmp_path), hf, H, Hq, Hkv, I, E, K, V, layers=2, fmt='awq')
    prompts = [rng.integers(3, V, n).astype(np.int32).tolist() for n in (19, 5, 40, 11, 27)]
    N = 6
    pipe = pipeline(str(tmp_path), backend_config=TurbomindEngineConfig(model_format='awq', quant_policy=8, max_batch_size=3,
                                                                        session_len=128))
    assert (pipe.model_cfg.arch, pipe.model_cfg.moe_experts, pipe.model_cfg.moe_top_k, pipe.model_cfg.qk_norm) == ('qwen3', E, K, 1)
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
def test_qwen3_moe_tune_gemm_128_experts(cuda, tmp_path, fmt):
    """tm_engine_tune_gemm on a 2-layer, 128-expert synthetic model, following test_engine_moe_measured_dispatch.
    (a) It runs at the decode batch and at a 64-token forward and writes its table (G lines); an engine that imports that table gives
    identical tokens.  Of the tuner's own lines only the lm_head's is asserted: it writes an expert line (w1w3 256 x 256,
    w2 128 x 256) only where a measured row tile beats the launcher's rule by 7 %, and the table it exports is the process's, with
    whatever earlier engines measured.
    (b) The expert lines themselves: every row-tile height the grouped kernels have, forced through an imported `G 32 / 34` line for
    each 128-expert shape at both sizes, is live in the table the launchers read (tm_debug_grouped_tile) and reproduces
    QwenMoeOracleModel on the 64-token prefill and two decode steps (3e-2 on the logits)."""
    from lmdeploy_amd import _ffi
    from tests.qwen_moe_reference import QwenMoeOracleModel
    cfg = QwenMoeConfig(**dict(QWEN3_MOE_CFG, moe_experts=128, vocab=512), kv_bits=8, weight_format=fmt, moe_fp8_act=fmt == 'fp8')
    w = make_qwen_moe_weights(cfg, seed=4)
    weights = export_weights(cfg, w)
    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (40, 9, 15)]      # one 64-token prefill forward
    path = str(tmp_path / 'table.txt')

    def run(tune=False, lines=None):
        eng = Engine.from_model_config(cfg, weight_type=2 if fmt == 'fp8' else 0, max_batch_size=3, session_len=128, quant_policy=8)
        eng.load_weights(weights)
        eng.start()
        if tune:
            eng.tune_gemm(3, path)
            eng.tune_gemm(64, path)
        else:
            if lines:
                open(path, 'w').write('\n'.join(lines) + '\n')
            eng.import_gemm_table(path)
        eng.prefill(prompts, max_new_tokens=4)
        lg = [eng.fetch_logits().copy()]
        for _ in range(3):
            eng.decode(1)
            lg.append(eng.fetch_logits().copy())
        toks = eng.fetch()
        eng.close()
        return toks, lg
    tuned, _ = run(tune=True)
    g = [ln.split() for ln in open(path).read().splitlines() if ln.startswith('G')]
    assert any(x[1] == '17' and x[3] == '256' and x[4] == '512' and x[5] == '3' for x in g), g      # the lm_head at the decode batch
    imported, _ = run()
    assert np.array_equal(tuned, imported)

    tm = _ffi.load()
    kind = 34 if fmt == 'fp8' else 32
    for K, N in ((256, 256), (128, 256)):                                                  # experts' w1w3 and w2
        for rows in ((32, 64) if fmt == 'fp8' else (16, 32, 64)):
            toks, lg = run(lines=[f'G {kind} 0 {K} {N} {M} {rows} 0 0 0' for M in (64, 3)])
            for M in (64, 3):
                got = _ffi.C.c_int(0)
                _ffi.check(tm.tm_debug_grouped_tile(kind - 32, K, N, M, _ffi.C.byref(got)))
                assert got.value == rows, (K, N, M, rows, got.value)
            om = QwenMoeOracleModel(cfg, w, batch=3, max_ctx=128)
            _, ref = om.forward(prompts)
            for s_ in range(3):
                d = np.abs(lg[s_].astype(np.float32) - ref.astype(np.float32))
                print(f'{fmt} experts K={K} N={N} forced {rows}-row tiles step {s_}: max logit diff {d.max():.4f}')
                assert d.max() <= 3e-2, f'experts K={K} N={N} forced {rows}-row tiles: step {s_}: max logit diff {d.max()}'
                if s_ < 2:
                    _, ref = om.forward([[int(t)] for t in toks[:, s_]])
