"""Sliding-window attention and attention sinks through the engine: per-layer windows and sinks at every attention call site (decode
eager and captured, chunked prefill with history beyond the window, the decode rows of a mixed step, the two-micro-batch prefill), the
clamp to full attention, and a Mistral checkpoint with `sliding_window` through pipeline().

Reference: tests/attention_window_reference.py::WindowOracleModel (OracleModel with the per-layer cropped context).  Bounds: the
project's engine bounds (tests/test_gpu_head_dim64.py::_engine_vs_oracle) -- logits within 3e-2 at every step, greedy tokens equal
where the oracle's top-2 gap exceeds 6e-2."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests.attention_window_reference import WindowConfig, WindowOracleModel, make_window_weights
from tests.qwen_reference import hf_qwen_tensors, tm_weights_from_hf

pytestmark = pytest.mark.gpu
f32 = np.float32
ROPE = {64: o.RopeParam(64, 500000.0, 'llama3', 32.0, 1.0, 4.0, 8192), 128: o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192)}
VARIANTS = {'window': dict(window=48), 'alternating+sinks': dict(layer_windows=(48, 0), attn_sinks=1)}


def _cfg(D, kv_bits, **over):
    base = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=D, inter=512, vocab=1024, kv_bits=kv_bits, rope=ROPE[D])
    base.update(over)
    return WindowConfig(**base)


def _engine(cfg, w, use_graph, batch, max_prefill=96, session_len=256):
    eng = Engine.from_model_config(cfg, max_batch_size=batch, session_len=session_len, quant_policy=0 if cfg.kv_bits == 16 else cfg.kv_bits,
                                   max_prefill_token_num=max_prefill, use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    return eng


def _engine_vs_oracle(cfg, w, use_graph, prompt_lens=(70, 5, 64), steps=6, max_prefill=96, session_len=256):
    """prefill + `steps` decode steps against WindowOracleModel, teacher-forced with the engine's tokens; the worst logit difference"""
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in prompt_lens]
    eng = _engine(cfg, w, use_graph, len(prompts), max_prefill, session_len)
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits().copy()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    eng.close()
    om = WindowOracleModel(cfg, w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    ref_logits, ref_toks = [lg], [ids]
    for s in range(steps):
        ids, lg = om.forward([[int(t)] for t in toks[:, s]])
        ref_logits.append(lg)
        ref_toks.append(ids)
    worst = 0.0
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s].astype(f32))
        worst = max(worst, float(d.max()))
        assert d.max() <= 3e-2, f'step {s}: max logit diff {d.max()}'
        top2 = np.sort(ref_logits[s].astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ref_toks[s][safe]), f'step {s}: greedy tokens differ'
    return worst


@pytest.mark.parametrize('use_graph', [0, 1])
@pytest.mark.parametrize('kv_bits', [8, 4, 16])
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('D', [64, 128])
def test_engine_matches_windowed_oracle(cuda, D, variant, kv_bits, use_graph):
    """prompts of 70 / 5 / 64 tokens against a window of 48: the prefill masks, the decode steps skip and mask"""
    cfg = _cfg(D, kv_bits, **VARIANTS[variant])
    worst = _engine_vs_oracle(cfg, make_window_weights(cfg, seed=3), use_graph)
    print(f'[windowed engine vs oracle] D {D} {variant} kv_bits {kv_bits} graph {use_graph}: max logit diff {worst:.5f}')


@pytest.mark.parametrize('kv_bits', [8, 16])
@pytest.mark.parametrize('D', [64, 128])
def test_engine_follows_the_window_not_full_attention(cuda, D, kv_bits):
    """With these small random models the windowed and the full-attention oracle are 1.4e-2 .. 2.2e-2 apart in the logits of the 70- and
    64-token prompts (computed from the two oracles alone) -- inside the 3e-2 engine bound, so the bound above cannot tell a window the
    engine ignored.  This can: the engine must be nearer to the windowed oracle than to the full one, at the prefill and at a decode step."""
    cfg = _cfg(D, kv_bits, window=48)
    w = make_window_weights(cfg, seed=3)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (70, 5, 64)]
    eng = _engine(cfg, w, 1, 3)
    eng.prefill(prompts, max_new_tokens=3)
    got = [eng.fetch_logits().astype(f32)]
    eng.decode(1)
    got.append(eng.fetch_logits().astype(f32))
    toks = eng.fetch()
    eng.close()
    om_w, om_f = WindowOracleModel(cfg, w, batch=3, max_ctx=256), o.OracleModel(cfg, w, batch=3, max_ctx=256)
    feed = prompts
    for s in range(2):
        win, full = om_w.forward(feed)[1].astype(f32), om_f.forward(feed)[1].astype(f32)
        sep = np.abs(win - full).max(-1)
        assert sep[0] > 1e-2 and sep[2] > 1e-2, sep           # 70 and 64 tokens exceed the window
        e_w, e_f = np.abs(got[s] - win).max(-1), np.abs(got[s] - full).max(-1)
        print(f'[window vs full] D {D} kv_bits {kv_bits} step {s}: oracles apart {sep}, engine to windowed {e_w}, to full {e_f}')
        assert e_w[0] < e_f[0] and e_w[2] < e_f[2], (s, e_w, e_f)
        feed = [[int(t)] for t in toks[:, s]]


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('D', [64, 128])
def test_engine_chunked_prefill_history_beyond_the_window(cuda, D, variant):
    """a 150-token prompt in chunks of 64 (the engine's smallest budget): the later chunks' history (64, 128) exceeds the window 48,
    so their key loop starts behind the first stage"""
    cfg = _cfg(D, 8, **VARIANTS[variant])
    _engine_vs_oracle(cfg, make_window_weights(cfg, seed=6), 1, prompt_lens=(150, 9), steps=3, max_prefill=32)


@pytest.mark.parametrize('kv_bits,D', [(8, 128), (16, 64)])
def test_continuous_batching_mixed_steps(cuda, monkeypatch, kv_bits, D):
    """the scheduler with mixed steps (decode rows of the running requests + an admission's prefill in one forward), every request's
    tokens against the windowed oracle alone, as tests/test_gpu_head_dim64.py::test_continuous_batching_mixed_steps does it"""
    monkeypatch.setenv('TM_MIXED_STEP', '1')
    cfg = _cfg(D, kv_bits, layer_windows=(48, 0), attn_sinks=1)
    w = make_window_weights(cfg, seed=13)
    rng = np.random.default_rng(6)
    lens = [70, 5, 64, 33, 150, 9]
    news = [6, 12, 3, 9, 5, 8]
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in lens]
    eng = _engine(cfg, w, 1, 3)
    ids = [eng.submit(p, n, -1, None, None) for p, n in zip(prompts, news)]
    done, steps = {}, 0
    while len(done) < len(ids):
        eng.step()
        steps += 1
        assert steps < 400, 'scheduler does not make progress'
        for i, rid in enumerate(ids):
            if i not in done:
                status, toks = eng.poll(rid)
                if status != 0:
                    done[i] = (status, toks.copy())
    n_mixed = eng.mixed_steps()
    eng.close()
    assert n_mixed >= 3, f'{n_mixed} mixed steps'
    checked = 0
    for i, (status, toks) in done.items():
        assert status == 7 and len(toks) == news[i], f'request {i}: status {status}, {len(toks)} tokens'
        om = WindowOracleModel(cfg, w, batch=1, max_ctx=256)
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


def test_prefill_two_microbatches(cuda, monkeypatch):
    """long prompts on a 1-rank communicator (TM_FORCE_COMM=1) engage forward_layers_two_microbatches, as
    tests/test_gpu_qwen_engine.py::test_qwen_prefill_two_microbatches_and_row_halves does: its prefill attention carries the layer's
    window and sinks too"""
    monkeypatch.setenv('TM_PIPE_MIN_ROWS', '256')
    monkeypatch.setenv('TM_COMM_STREAM', '1')
    monkeypatch.setenv('TM_FORCE_COMM', '1')
    cfg = _cfg(128, 8, layer_windows=(48, 0), attn_sinks=1)
    w = make_window_weights(cfg, seed=5)
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (300, 77, 190, 33)]
    eng = Engine.from_model_config(cfg, max_batch_size=4, session_len=1024, quant_policy=8, max_prefill_token_num=1024, use_graph=1)
    eng.comm_init(Engine.comm_unique_id())
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill(prompts, max_new_tokens=4)
    lg = [eng.fetch_logits().copy()]
    for _ in range(2):
        eng.decode(1)
        lg.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    info = eng.comm_info()
    eng.close()
    assert info['microbatch_forwards'] >= 1, info
    om = WindowOracleModel(cfg, w, batch=4, max_ctx=1024)
    _, ref = om.forward(prompts)
    for s in range(3):
        d = np.abs(lg[s].astype(f32) - ref.astype(f32)).max()
        assert d <= 3e-2, f'step {s}: max logit diff {d}'
        if s < 2:
            _, ref = om.forward([[int(t)] for t in toks[:, s]])


@pytest.mark.parametrize('kv_bits', [8, 16])
def test_window_covering_the_session_is_the_plain_engine(cuda, kv_bits):
    """attn_window = 4096 >= session_len and no sinks: clamped to full attention, the engine keeps its path (fused MFMA decode at
    int8 KV) -- logits bit for bit those of the engine without the field"""
    rng = np.random.default_rng(0)
    runs = []
    for window in (0, 4096):
        cfg = _cfg(128, kv_bits, window=window)
        w = make_window_weights(cfg, seed=3)
        prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in (70, 5, 64)] if not runs else prompts
        eng = _engine(cfg, w, 1, 3)
        eng.prefill(prompts, max_new_tokens=4)
        lg = [eng.fetch_logits().copy()]
        for _ in range(3):
            eng.decode(1)
            lg.append(eng.fetch_logits().copy())
        eng.close()
        runs.append(np.stack(lg))
    assert np.array_equal(runs[0].view(np.uint16), runs[1].view(np.uint16))


def test_layer_windows_are_validated(cuda):
    cfg = _cfg(64, 8)
    eng = Engine.from_model_config(cfg, max_batch_size=1, session_len=128, quant_policy=8)
    with pytest.raises(Exception, match='window'):
        eng.set_layer_windows([48, -1])
    with pytest.raises(Exception, match='layer'):
        eng.set_layer_windows([48])
    eng.close()


# ---- Mistral checkpoint on disk ------------------------------------------------------------------------------------------------------
def _write_mistral_checkpoint(path, hf, H, Hq, Hkv, I, V, layers, D, awq, sliding_window):
    from safetensors.numpy import save_file
    tensors, quant = {}, {}
    for k, v in hf.items():
        if awq and k.endswith('_proj.weight'):
            pre = k[:-len('.weight')]
            q, s, z, _ = o.quantize_groupwise_u4(np.ascontiguousarray(v.T), 128)
            tensors[pre + '.qweight'] = o.pack_awq_gemm(q)
            tensors[pre + '.qzeros'] = o.pack_awq_gemm(z.astype(np.uint8))
            tensors[pre + '.scales'] = s
            quant[pre] = (q, s, z)
        else:
            tensors[k] = v
    save_file(tensors, os.path.join(path, 'model.safetensors'))
    c = {'architectures': ['MistralForCausalLM'], 'hidden_size': H, 'num_hidden_layers': layers, 'num_attention_heads': Hq,
         'num_key_value_heads': Hkv, 'head_dim': D, 'intermediate_size': I, 'vocab_size': V, 'rms_norm_eps': 1e-5, 'rope_theta': 10000.0,
         'max_position_embeddings': 32768, 'sliding_window': sliding_window, 'tie_word_embeddings': False, 'eos_token_id': 2,
         'torch_dtype': 'float16'}
    if awq:
        c['quantization_config'] = {'quant_method': 'awq', 'bits': 4, 'group_size': 128, 'zero_point': True, 'version': 'gemm'}
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)
    return quant


@pytest.mark.parametrize('awq,kv_bits', [(False, 8), (True, 4)])
def test_mistral_checkpoint_through_pipeline(cuda, tmp_path, awq, kv_bits):
    """fabricated fp16 / AWQ Mistral checkpoint with "sliding_window": 48 -> pipeline(path): the window reaches the engine (greedy tokens
    equal to an engine configured with window 48 directly, on weights assembled here) and the windowed oracle agrees"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    rng = np.random.default_rng(31 + kv_bits)
    H, Hq, Hkv, I, V, D = 256, 4, 2, 512, 640, 128
    hf = hf_qwen_tensors(rng, 'qwen2', H, Hq, Hkv, I, V, layers=2, D=D, bias=False)     # Mistral's tensor names are Llama's
    quant = _write_mistral_checkpoint(str(tmp_path), hf, H, Hq, Hkv, I, V, 2, D, awq, 48)
    cfg = WindowConfig(hidden=H, layers=2, q_heads=Hq, kv_heads=Hkv, head_dim=D, inter=I, vocab=V, rms_eps=1e-5, kv_bits=kv_bits,
                       rope=o.RopeParam(D, 10000.0), window=48)
    w = tm_weights_from_hf(hf, cfg, quant if awq else None)
    prompts = [rng.integers(3, V, n).astype(np.int32).tolist() for n in (70, 5, 64)]
    N = 6
    pipe = pipeline(str(tmp_path), backend_config=TurbomindEngineConfig(model_format='awq' if awq else 'hf', quant_policy=kv_bits,
                                                                        max_batch_size=3, session_len=128))
    assert pipe.model_cfg.window == 48 and pipe.model_cfg.quantized == awq
    got = [r.token_ids for r in pipe(prompts, GenerationConfig(max_new_tokens=N, ignore_eos=True))]
    pipe.engine.prefill(prompts, max_new_tokens=2)
    lg0 = pipe.engine.fetch_logits().astype(f32)
    pipe.engine.release()
    pipe.close()
    # the windowed engine, configured directly
    eng = Engine.from_model_config(cfg, weight_type=0 if awq else 1, max_batch_size=3, session_len=128, quant_policy=kv_bits)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    eng.prefill([np.asarray(p, np.int32) for p in prompts], max_new_tokens=N)
    eng.decode(N - 1)
    direct = eng.fetch()
    eng.close()
    assert np.array_equal(np.asarray(got), direct[:, :N]), (got, direct)
    om = WindowOracleModel(cfg, w, batch=3, max_ctx=128)
    _, ref = om.forward([np.asarray(p) for p in prompts])
    ref = ref.astype(f32)
    assert np.abs(lg0 - ref).max() <= 3e-2, np.abs(lg0 - ref).max()
    for s in range(N):
        for b in range(3):
            top = np.argsort(ref[b])[::-1][:2]
            margin = ref[b][top[0]] - ref[b][top[1]]
            assert got[b][s] == top[0] or (margin <= 6e-2 and got[b][s] == top[1]), (b, s, got[b][s], top, margin)
        if s + 1 < N:
            _, ref = om.forward([[got[b][s]] for b in range(3)])
            ref = ref.astype(f32)
