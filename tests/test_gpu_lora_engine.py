"""Multi-LoRA in the engine on a tiny dense fp16 model (hidden 256, 2 layers, 4 q / 2 kv heads, int8 KV): a static batch under adapter a
(rank 8: zero-padded), b (rank 16) and none, against the oracle on each sequence's MERGED weights W + B A (merged in float32, handed over as
fp16, the oracle's weight dtype).  Bound: 3e-2 per logit, that of tests/test_gpu_head_dim64.py::_engine_vs_oracle and smoke() for this
geometry and KV policy.  The scale (B ~ N(0, 0.3^2 / r), A ~ N(0, 1 / K)) makes the adapters matter: on the CPU oracle the three weight
sets give logits more than four bounds apart and different greedy tokens for one prompt -- asserted before any GPU work."""
import copy

import numpy as np
import pytest

from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, _ffi, pipeline
from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o

pytestmark = pytest.mark.gpu
BOUND, STEPS, LENS = 3e-2, 4, (33, 7, 20)
RANKS, SCALE = dict(a=8, b=16), 0.3
_MODELS = {}


def _model(D):
    """cfg, base weights, raw adapters {name: per layer {q, k, v, o, down: (A [r, K], B [N, r])}}, merged weights per name, prompts"""
    if D not in _MODELS:
        cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=D, inter=512, vocab=1024, kv_bits=8,
                            rope=o.RopeParam(D, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192))
        w = o.make_synthetic_weights(cfg, seed=11, quantized=False)
        kq, kkv = cfg.q_heads * D, cfg.kv_heads * D
        shapes = dict(q=(cfg.hidden, kq), k=(cfg.hidden, kkv), v=(cfg.hidden, kkv), o=(kq, cfg.hidden), down=(cfg.inter, cfg.hidden))
        raw, merged = {}, {None: w}
        for name, r in RANKS.items():
            rng = np.random.default_rng(100 + r)
            raw[name] = [{n: (rng.standard_normal((r, K)).astype(np.float32) / np.sqrt(K),
                              rng.standard_normal((N, r)).astype(np.float32) * SCALE / np.sqrt(r)) for n, (K, N) in shapes.items()}
                         for _ in range(cfg.layers)]
            mw = copy.deepcopy(w)
            for L, ad in zip(mw['layers'], raw[name]):
                d = {n: (B @ A).T for n, (A, B) in ad.items()}      # [K, N] like the oracle's weights
                L['w_qkv']['w'] = (L['w_qkv']['w'].astype(np.float32) + np.concatenate([d['q'], d['k'], d['v']], 1)).astype(np.float16)
                L['wo']['w'] = (L['wo']['w'].astype(np.float32) + d['o']).astype(np.float16)
                L['w2']['w'] = (L['w2']['w'].astype(np.float32) + d['down']).astype(np.float16)
            merged[name] = mw
        rng = np.random.default_rng(3)
        prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in LENS]
        # the adapters must matter: one prompt, three weight sets -> logits far apart, different greedy tokens
        first = {k: o.OracleModel(cfg, mw, batch=1, max_ctx=128).forward([prompts[1]]) for k, mw in merged.items()}
        keys = list(first)
        for i, p in enumerate(keys):
            for q in keys[i + 1:]:
                gap = np.abs(first[p][1].astype(np.float32) - first[q][1].astype(np.float32)).max()
                assert gap > 4 * BOUND, (p, q, gap)
                assert int(first[p][0][0]) != int(first[q][0][0]), (p, q)
        _MODELS[D] = (cfg, w, raw, merged, prompts, {k: int(v[0][0]) for k, v in first.items()})
    return _MODELS[D]


def _operands(cfg, ad, zero_b=False):
    kq, kkv = cfg.q_heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    z = (lambda p: (p[0], p[1] * 0)) if zero_b else (lambda p: p)
    return {_ffi.LORA_QKV: checkpoint.lora_operands([z(ad['q']), z(ad['k']), z(ad['v'])], [kq, kkv, kkv], 1.0),
            _ffi.LORA_WO: checkpoint.lora_operands([z(ad['o'])], [cfg.hidden], 1.0),
            _ffi.LORA_W2: checkpoint.lora_operands([z(ad['down'])], [cfg.hidden], 1.0)}


def _engine(D, use_graph, batch=3):
    """an engine with adapters a (slot 0), b (slot 1) and a with B = 0 (slot 2) loaded"""
    cfg, w, raw = _model(D)[:3]
    eng = Engine.from_model_config(cfg, weight_type=1, max_batch_size=batch, session_len=128, quant_policy=8, max_prefill_token_num=64,
                                   decode_splits=2, use_graph=use_graph)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    for slot, (name, zero_b) in enumerate((('a', False), ('b', False), ('a', True))):
        for li, ad in enumerate(raw[name]):
            for kind, (A, B, ranks) in _operands(cfg, ad, zero_b).items():
                eng.load_adapter(slot, li, kind, A, B, ranks)
    return eng


def _generate(eng, prompts, slots):
    """prefill + STEPS decode steps -> (logits [STEPS + 1][batch, vocab], tokens [batch, STEPS + 1])"""
    eng.set_adapters(slots)
    eng.prefill(prompts, max_new_tokens=STEPS + 1)
    logits = [eng.fetch_logits().copy()]
    for _ in range(STEPS):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
    toks = eng.fetch()
    eng.release()
    return logits, toks


@pytest.mark.parametrize('use_graph', [1, 0])
@pytest.mark.parametrize('D', [128, 64])
def test_mixed_batch_against_merged_oracle(D, use_graph):
    cfg, _, _, merged, prompts, first = _model(D)
    eng = _engine(D, use_graph)
    try:
        logits, toks = _generate(eng, prompts, [0, 1, -1])
        alone, _ = _generate(eng, [prompts[2]], [-1])
        same, stoks = _generate(eng, [prompts[1]] * 3, [0, 1, -1])
        zero, _ = _generate(eng, [prompts[0]] * 2, [2, -1])
    finally:
        eng.close()
    for b, name in enumerate(('a', 'b', None)):      # every sequence against the oracle on ITS merged weights, teacher-forced
        om = o.OracleModel(cfg, merged[name], batch=1, max_ctx=128)
        feed = [prompts[b]] + [[int(t)] for t in toks[b, :STEPS]]
        for s, ids in enumerate(feed):
            _, ref = om.forward([ids])
            d = np.abs(logits[s][b].astype(np.float32) - ref[0].astype(np.float32)).max()
            assert d <= BOUND, f'sequence {b} (adapter {name}) step {s}: max logit diff {d}'
    # the adapter-free sequence of the mixed batch: the bits of the same prompt run alone with none selected
    for s in range(STEPS + 1):
        assert np.array_equal(logits[s][2].view(np.uint16), alone[s][0].view(np.uint16)), f'adapter-free sequence differs at step {s}'
    # an adapter with B = 0 changes no bit
    for s in range(STEPS + 1):
        assert np.array_equal(zero[s][0].view(np.uint16), zero[s][1].view(np.uint16)), f'zero adapter differs at step {s}'
    # one prompt under a, b and none: the oracle's (distinct) first tokens
    assert [int(t) for t in stoks[:, 0]] == [first['a'], first['b'], first[None]]


def test_engine_refusals():
    cfg, _, raw = _model(128)[:3]
    eng = _engine(128, 0, batch=2)
    try:
        A, B, ranks = _operands(cfg, raw['a'][0])[_ffi.LORA_WO]
        for args, msg in (((0, 0, _ffi.LORA_W13, A, B, ranks), 'gate_proj / up_proj'), ((8, 0, _ffi.LORA_WO, A, B, ranks), 'at most 8 adapter slots'),
                          ((0, 2, _ffi.LORA_WO, A, B, ranks), 'layer outside the model'),
                          ((0, 0, _ffi.LORA_WO, np.zeros((80, 512), np.float16), np.zeros((256, 80), np.float16), [80]), 'rank over 64 per segment')):
            with pytest.raises(_ffi.TmError, match=msg):
                eng.load_adapter(*args)
        with pytest.raises(_ffi.TmError, match=r'adapter id outside \[-1, 8\)'):
            eng.set_adapters([0, 8])
        with pytest.raises(_ffi.TmError, match='speculative decoding while an adapter is loaded'):
            eng.set_speculative(3)
        eng.set_adapters([0])
        with pytest.raises(_ffi.TmError, match='batch size differs'):
            eng.prefill([[1, 2, 3], [4, 5]], max_new_tokens=2)
    finally:
        eng.close()


def test_pipeline_adapter_name():
    """pipe(prompts, adapter_name=[...]) of a synthetic pipeline: the engine-level tokens, and every refusal of the public surface"""
    pipe = pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(quant_policy=8, max_batch_size=3, session_len=128))
    try:
        for seed, name in enumerate(('a', 'b')):
            pipe.load_synthetic_adapter(name, rank=8 * (seed + 1), seed=seed, scale=0.3)
        rng, g = np.random.default_rng(1), GenerationConfig(max_new_tokens=STEPS + 1, ignore_eos=True)
        prompts = [rng.integers(0, 1024, n).tolist() for n in LENS]
        _, want = _generate(pipe.engine, prompts, [1, 0, -1])
        got = pipe(prompts, g, adapter_name=['b', 'a', None])
        assert [r.token_ids for r in got] == want.tolist()
        assert pipe(prompts[0], g, adapter_name='a').token_ids != pipe(prompts[0], g).token_ids
        for names, msg in ((['a', 'c', None], "unknown adapter 'c'"), (['a'], '1 adapter names for 3 prompts')):
            with pytest.raises(ValueError, match=msg):
                pipe(prompts, g, adapter_name=names)
        mm = dict(input_ids=prompts[1], input_embeddings=[np.zeros((2, 256), np.float16)], input_embedding_ranges=[(0, 2)])
        for call, msg in ((lambda: next(iter(pipe.stream_infer(prompts, g, adapter_name='a'))), 'streaming with an adapter selected'),
                          (lambda: pipe(prompts, [g] * 3, adapter_name='a'), 'continuous batching, which serves the base model only'),
                          (lambda: pipe(prompts * 2, g, adapter_name='a'), 'continuous batching, which serves the base model only'),
                          (lambda: pipe([mm], g, adapter_name='a'), 'multimodal prompts with an adapter selected')):
            with pytest.raises(NotImplementedError, match=msg):
                call()
    finally:
        pipe.close()


@pytest.mark.parametrize('model,policy,msg', [('tiny', 42, 'quant_policy 42'), ('tiny_moe', 8, 'mixture-of-experts')])
def test_engine_refuses_model(model, policy, msg):
    pipe = pipeline('synthetic:' + model, backend_config=TurbomindEngineConfig(quant_policy=policy, max_batch_size=2, session_len=128))
    try:
        with pytest.raises(_ffi.TmError, match=msg):
            pipe.engine.load_adapter(0, 0, _ffi.LORA_WO, np.zeros((16, 512), np.float16), np.zeros((256, 16), np.float16), [16])
    finally:
        pipe.close()
