"""Qwen2 (q / k / v bias) and Qwen3 (per-head q / k RMSNorm) models through the whole engine against QwenOracleModel
(tests/qwen_reference.py) with the bounds of test_gpu_engine.test_engine_matches_oracle: 3e-2 on O(1) logits at every step,
greedy tokens equal wherever the oracle's top-2 margin exceeds 6e-2.  Every path that applies the attention prologue is
driven: prefill (kv_rope_store), the fused int8 / int4 decode prologue (slabs and fp16 input, folded norm or not, graph or
eager), fp16-KV decode, TM_FUSE_QKV=0, TM_ATTN_VALU=1, mixed continuous-batching steps, the two-micro-batch / row-half
prefill schedules, and a checkpoint on disk through pipeline(path)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests.qwen_reference import (QWEN2_CFG, QWEN3_CFG, QwenConfig, QwenOracleModel, engine_vs_oracle, hf_qwen_tensors,
                                  make_qwen_weights, tm_weights_from_hf, write_qwen_checkpoint)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('fold', [0, 3])
@pytest.mark.parametrize('kv_bits,use_graph', [(8, 1), (8, 0), (4, 1), (4, 0), (16, 1), (16, 0)])
@pytest.mark.parametrize('kind', ['qwen2', 'qwen3'])
def test_qwen_engine_matches_oracle(cuda, monkeypatch, kind, kv_bits, use_graph, fold):
    monkeypatch.setenv('TM_FOLD_NORM', str(fold))
    worst = engine_vs_oracle(kind, kv_bits, use_graph)
    print(f'[{kind} vs oracle] kv {kv_bits} graph {use_graph} fold {fold}: max logit diff {worst:.5f}')


@pytest.mark.parametrize('kind', ['qwen2', 'qwen3'])
def test_qwen_engine_unfused_qkv(cuda, monkeypatch, kind):
    """TM_FUSE_QKV=0: int8 decode through kv_rope_store + the unfused MFMA kernel"""
    monkeypatch.setenv('TM_FUSE_QKV', '0')
    engine_vs_oracle(kind, 8, 1)


@pytest.mark.parametrize('kind', ['qwen2', 'qwen3'])
def test_qwen_engine_valu_attention(cuda, kind):
    """TM_ATTN_VALU=1 (read once per process by the attention launcher: a child process): the VALU decode kernel behind
    kv_rope_store, which applies the prologue"""
    code = ('import sys; sys.path.insert(0, %r); from tests.qwen_reference import engine_vs_oracle; '
            'print("worst", engine_vs_oracle(%r, 8, 1)); engine_vs_oracle(%r, 4, 0)' % (ROOT, kind, kind))
    env = dict(os.environ, TM_ATTN_VALU='1')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize('kv_bits', [8, 16])
@pytest.mark.parametrize('kind', ['qwen2', 'qwen3'])
def test_qwen_continuous_batching_mixed_steps(cuda, monkeypatch, kind, kv_bits):
    """the scheduler with mixed steps (decode rows of the running requests + an admission's prefill in one forward): every request's
    tokens against the oracle alone, as test_gpu_engine.test_continuous_batching_matches_oracle does"""
    monkeypatch.setenv('TM_MIXED_STEP', '1')
    cfg = QwenConfig(**(QWEN2_CFG if kind == 'qwen2' else QWEN3_CFG), kv_bits=kv_bits)
    w = make_qwen_weights(cfg, seed=13)
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
                st, toks = eng.poll(rid)
                if st != 0:
                    done[i] = (st, toks.copy())
    n_mixed = eng.mixed_steps()
    eng.close()
    assert n_mixed >= 3, f'{n_mixed} mixed steps'
    checked = 0
    for i, (st, toks) in done.items():
        assert st == 7 and len(toks) == news[i], f'request {i}: status {st}, {len(toks)} tokens'
        om = QwenOracleModel(cfg, w, batch=1, max_ctx=256)
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


@pytest.mark.parametrize('min_rows,lens,want_mb', [(256, (300, 77, 190, 33), 1), (256, (600,), 0)])
@pytest.mark.parametrize('kind', ['qwen2', 'qwen3'])
def test_qwen_prefill_two_microbatches_and_row_halves(cuda, monkeypatch, kind, min_rows, lens, want_mb):
    """long prompts on a 1-rank communicator (TM_FORCE_COMM=1): the two-micro-batch forward (forward_layers_two_microbatches) or
    the row-half schedule (forward_tail_two_halves) runs the prefill; logits of the prefill and of 4 decode steps against the oracle"""
    monkeypatch.setenv('TM_PIPE_MIN_ROWS', str(min_rows))
    monkeypatch.setenv('TM_COMM_STREAM', '1')
    monkeypatch.setenv('TM_FORCE_COMM', '1')
    cfg = QwenConfig(**dict(QWEN2_CFG if kind == 'qwen2' else QWEN3_CFG, layers=3), kv_bits=8)
    w = make_qwen_weights(cfg, seed=5)
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in lens]
    eng = Engine.from_model_config(cfg, max_batch_size=4, session_len=1024, quant_policy=8, max_prefill_token_num=1024, use_graph=1)
    eng.comm_init(Engine.comm_unique_id())
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill(prompts, max_new_tokens=6)
    lg = [eng.fetch_logits().copy()]
    for _ in range(4):
        eng.decode(1)
        lg.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    info = eng.comm_info()
    eng.close()
    assert info['overlapped_forwards'] >= 1
    assert (info['microbatch_forwards'] >= 1) == bool(want_mb), info
    om = QwenOracleModel(cfg, w, batch=len(prompts), max_ctx=1024)
    _, ref = om.forward(prompts)
    for s in range(5):
        d = np.abs(lg[s].astype(np.float32) - ref.astype(np.float32)).max()
        assert d <= 3e-2, f'step {s}: max logit diff {d}'
        if s < 4:
            _, ref = om.forward([[int(t)] for t in toks[:, s]])


@pytest.mark.parametrize('kind,awq,kv_bits', [('qwen2', True, 8), ('qwen3', False, 4)])
def test_qwen_checkpoint_through_pipeline(cuda, tmp_path, kind, awq, kv_bits):
    """fabricated AWQ-Qwen2 / fp16-Qwen3 (tied embeddings) checkpoint -> pipeline(path) -> greedy tokens and first-step logits against
    QwenOracleModel on weights assembled here from the HF tensors (not by checkpoint.py)"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    rng = np.random.default_rng(11 + kv_bits)
    H, Hq, Hkv, I, V = 256, (7 if kind == 'qwen2' else 4), (1 if kind == 'qwen2' else 2), 512, 640
    tie = kind == 'qwen3'
    hf = hf_qwen_tensors(rng, kind, H, Hq, Hkv, I, V, layers=2, tie=tie)
    quant = write_qwen_checkpoint(str(tmp_path), kind, hf, H, Hq, Hkv, I, V, layers=2, awq=awq, tie=tie)
    cfg = QwenConfig(hidden=H, layers=2, q_heads=Hq, kv_heads=Hkv, head_dim=128, inter=I, vocab=V, rms_eps=1e-6, kv_bits=kv_bits,
                     rope=o.RopeParam(128, 1e6),
                     attn_bias=int(kind == 'qwen2'), qk_norm=int(kind == 'qwen3'))
    w = tm_weights_from_hf(hf, cfg, quant if awq else None)
    prompts = [rng.integers(3, V, n).astype(np.int32).tolist() for n in (19, 5, 40)]
    N = 6
    pipe = pipeline(str(tmp_path), backend_config=TurbomindEngineConfig(model_format='awq' if awq else 'hf', quant_policy=kv_bits,
                                                                        max_batch_size=3, session_len=128))
    assert pipe.model_cfg.arch == kind
    g = GenerationConfig(max_new_tokens=N, ignore_eos=True)
    got = [r.token_ids for r in pipe(prompts, g)]
    pipe.engine.prefill(prompts, max_new_tokens=2)
    lg0 = pipe.engine.fetch_logits().astype(np.float32)
    pipe.engine.release()
    pipe.close()
    om = QwenOracleModel(cfg, w, batch=3, max_ctx=128)
    _, ref = om.forward([np.asarray(p) for p in prompts])
    ref = ref.astype(np.float32)
    assert np.abs(lg0 - ref).max() <= 3e-2, np.abs(lg0 - ref).max()
    for s in range(N):
        for b in range(3):
            top = np.argsort(ref[b])[::-1][:2]
            margin = ref[b][top[0]] - ref[b][top[1]]
            assert got[b][s] == top[0] or (margin <= 6e-2 and got[b][s] == top[1]), (kind, b, s, got[b][s], top, margin)
        if s + 1 < N:
            _, ref = om.forward([[got[b][s]] for b in range(3)])
            ref = ref.astype(np.float32)
