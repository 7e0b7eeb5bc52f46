"""Qwen2-VL language models in the engine: M-RoPE coordinates, position deltas and image-embedding rows through static prefill
(whole and chunked), decode (fused int8 prologue with the delta array, fp16 KV through the sectioned store; graph and eager), against
the per-sequence oracle of tests/qwen_vl_reference.py; text-only equivalence with an engine without sections; embeddings on a model
without sections; the refusals of tm_engine_set_multimodal; a toy transformers checkpoint through pipeline().

Bounds: logits 3e-2 (tests/test_gpu_engine.py::test_engine_matches_oracle, same geometry), KV blocks as
tests/test_gpu_rope_scaling.py::check_kv_blocks, greedy tokens against transformers by the margin rule of tests/test_gpu_qwen_engine.py.
The weights are the rope-sensitive ones of tests/test_gpu_rope_scaling.py (q / k x 32, v x 8 through the AWQ scales): with the plain
synthetic weights the logits hardly depend on positions and the tests would pass with the coordinates ignored -- the power check in
test_static_batch_matches_oracle asserts that they do not."""
import dataclasses

import numpy as np
import pytest

from lmdeploy_amd import _ffi, vl
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests import qwen_vl_reference as Q
from tests.qwen_reference import make_qwen_weights
from tests.test_gpu_rope_scaling import check_kv_blocks, max_diff

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
LOGIT_BOUND = 3e-2
SESSION = 256
IMG = 1000                        # image placeholder id (inside the vocabulary; never looked up)


def tiny_cfg(kv_bits, sections=Q.SECTIONS):
    return Q.QwenVLConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, kv_bits=kv_bits,
                          rope=o.RopeParam(128, 10000.0), attn_bias=1, mrope_section=sections)


def sensitive_weights(cfg, seed=3):
    w = make_qwen_weights(cfg, seed=seed)
    nqk = (cfg.q_heads + cfg.kv_heads) * cfg.head_dim
    for L in w['layers']:
        s = L['w_qkv']['s']
        s[:, :nqk] = (s[:, :nqk].astype(f32) * f32(32)).astype(f16)
        s[:, nqk:] = (s[:, nqk:].astype(f32) * f32(8)).astype(f16)
    return w


def batch(cfg, seed=0):
    """three prompts and their multimodal input: text only (9 tokens); one 12 x 16 image = 48 image tokens at positions 5 .. 52 of 70;
    two images (4 x 4 and 4 x 6) in 20 tokens.  -> (prompts, mm for the oracle)"""
    rng = np.random.default_rng(seed)

    def text(n):
        return rng.integers(0, 999, n).tolist()
    p0 = text(9)
    p1 = text(5) + [IMG] * 48 + text(17)
    p2 = text(2) + [IMG] * 4 + text(2) + [IMG] * 6 + text(6)
    grids = [None, [[1, 12, 16]], [[1, 4, 4], [1, 4, 6]]]
    prompts, mm = [np.asarray(p, np.int32) for p in (p0, p1, p2)], []
    for p, g in zip(prompts, grids):
        if g is None:
            mm.append(None)
            continue
        coords, delta = vl.mrope_positions(p, g, IMG, 2)
        emb = {int(i): (0.05 * rng.standard_normal(cfg.hidden)).astype(f16) for i in np.flatnonzero(p == IMG)}
        mm.append(dict(coords=coords, delta=delta, emb=emb))
    assert [len(p) for p in prompts] == [9, 70, 20] and mm[1]['delta'] == 8 - 48 and mm[2]['delta'] == (2 + 3) - 4 - 6 + 0
    return prompts, mm


def make_engine(cfg, w, kv_bits, use_graph=1, max_prefill=128, max_batch=3, **kw):
    eng = Engine.from_model_config(cfg, max_batch_size=max_batch, session_len=SESSION, quant_policy=0 if kv_bits == 16 else kv_bits,
                                   max_prefill_token_num=max_prefill, use_graph=use_graph, **kw)
    eng.load_weights(export_weights(cfg, w))
    eng.start()
    return eng


def run_wave(eng, cfg, w, prompts, mm, steps, kv_bits, what, sections=Q.SECTIONS):
    """set_multimodal + prefill + `steps` decode steps against the per-sequence oracle (teacher-forced with the engine's tokens)"""
    lens = [len(p) for p in prompts]
    if any(m is not None for m in mm):
        eng.set_multimodal([Q.engine_mm(m, n, cfg.hidden) for m, n in zip(mm, lens)])
    eng.prefill(prompts, max_new_tokens=steps + 1)
    logits = [eng.fetch_logits()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits())
    toks = eng.fetch()
    oracle = Q.PerSequenceVLOracle(cfg, w, mm, SESSION, sections, SESSION + 1)
    _, lg = oracle.forward(prompts)
    ref = [lg]
    for s in range(steps):
        _, lg = oracle.forward([[int(t)] for t in toks[:, s]])
        ref.append(lg)
    worst = max(float(max_diff(logits[s], ref[s]).max()) for s in range(steps + 1))
    print(f'[qwen-vl] {what}: lens {lens} max logit diff over {steps + 1} steps {worst:.5f}')
    for s in range(steps + 1):
        d = max_diff(logits[s], ref[s])
        assert d.max() <= LOGIT_BOUND, f'{what} step {s}: max logit diff per sequence {d}'
    check_kv_blocks(eng, oracle, lens, steps, kv_bits)
    return logits, ref, toks


@pytest.mark.parametrize('use_graph', [1, 0])
@pytest.mark.parametrize('kv_bits', [8, 16])
def test_static_batch_matches_oracle(cuda, kv_bits, use_graph):
    """(h) prefill + 4 decode steps; then a text-only wave in the same engine (stale deltas or coordinates would show); the same run
    against an oracle given linear coordinates must break the bound"""
    cfg = tiny_cfg(kv_bits)
    w = sensitive_weights(cfg)
    prompts, mm = batch(cfg)
    eng = make_engine(cfg, w, kv_bits, use_graph)
    logits, ref, toks = run_wave(eng, cfg, w, prompts, mm, 4, kv_bits, f'kv {kv_bits} graph {use_graph}')
    eng.release()
    run_wave(eng, cfg, w, prompts[::-1], [None] * 3, 2, kv_bits, f'kv {kv_bits} graph {use_graph} text wave')
    eng.close()
    # sensitivity: linear coordinates (and no delta), same embeddings -- the multimodal sequences must leave the bound, the text one not
    lin = Q.PerSequenceVLOracle(cfg, w, [None if m is None else dict(emb=m['emb']) for m in mm], SESSION, Q.SECTIONS, SESSION + 1)
    _, lg = lin.forward(prompts)
    gaps = [max_diff(logits[0], lg)]
    for s in range(4):
        _, lg = lin.forward([[int(t)] for t in toks[:, s]])
        gaps.append(max_diff(logits[s + 1], lg))
    gaps = np.stack(gaps)
    print(f'[qwen-vl] engine vs an oracle with linear coordinates, per step x sequence (bound {LOGIT_BOUND}):\n{gaps}\n'
          f'ratio to the bound: {gaps.max(axis=0) / LOGIT_BOUND}')
    assert gaps[:, 0].max() <= LOGIT_BOUND and gaps[:, 1].max() > LOGIT_BOUND and gaps[:, 2].max() > LOGIT_BOUND


@pytest.mark.parametrize('kv_bits', [8, 16])
def test_chunked_prefill(cuda, kv_bits):
    """(i) 48 tokens per prefill iteration: 9 + 39 (the image of sequence 1 is cut at row 39), 31 + 17, 3"""
    cfg = tiny_cfg(kv_bits)
    w = sensitive_weights(cfg)
    prompts, mm = batch(cfg)
    eng = make_engine(cfg, w, kv_bits, 1, max_prefill=48)
    run_wave(eng, cfg, w, prompts, mm, 4, kv_bits, f'kv {kv_bits} chunked')
    eng.close()


def _continuous_text(eng, prompts, logprobs):
    """the prompts through the scheduler, the third submitted two steps after the others (its admission meets running requests: a
    mixed step when no request asks for logprobs).  -> what must be the same bits in both engines: the residual stream of the first
    three rows of every step's last forward (all three decode rows of a decode step), every request's tokens and, with logprobs, the
    fp32 logprobs of the kept candidates (top-k 4, seeded draws) and of the drawn token of every generated token"""
    kw = dict(logprobs=logprobs) if logprobs else {}
    sampling = (1.0, logprobs, 1.0, 0.0, 7) if logprobs else None      # top-k = the candidates kept (greedy rows keep one), seeded draw
    rids = [eng.submit(p, 5, -1, sampling, None, **kw) for p in prompts[:2]]
    resid = []
    for step in range(12):
        if step == 2:
            rids.append(eng.submit(prompts[2], 5, -1, sampling, None, **kw))
        eng.step()
        resid.append(eng.fetch_residual(3).view(np.uint16).copy())
    polled = [eng.poll(r) for r in rids]
    assert all(st == 7 and len(t) == 5 for st, t in polled)
    rec = []
    if logprobs:
        for r in rids:
            vals, idx, num, sel = eng.poll_logprobs(r)
            assert vals.shape == (5, logprobs) and np.all(num >= 1) and num.max() > 1 and np.isfinite(sel).all()
            rec += [vals.view(np.uint32).copy(), idx.copy(), num.copy(), sel.view(np.uint32).copy()]
    mixed = eng.mixed_steps()
    eng.release()
    return np.stack(resid), np.stack([t for _, t in polled]), rec, mixed


@pytest.mark.parametrize('kv_bits', [8, 16])
def test_text_only_is_the_engine_without_sections(cuda, kv_bits):
    """(j) the same weights with and without sections, text only, bit for bit: the logits of the static batch (prefill and decode -- the
    delta array of zeros against no array); through the continuous scheduler (which keeps the plain kernels; logits cannot be read back
    there) the residual stream behind the last layer after every scheduler step, mixed steps included, and in a second session the fp32
    logprobs of four kept candidates and of the drawn token of every generated token -- values computed from the logits row"""
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, 1024, n).astype(np.int32) for n in (70, 5, 33)]
    out = []
    for sections in (Q.SECTIONS, None):
        cfg = tiny_cfg(kv_bits, sections)
        eng = make_engine(cfg, sensitive_weights(cfg), kv_bits)
        eng.prefill(prompts, max_new_tokens=4)
        lg = [eng.fetch_logits().copy()]
        for _ in range(3):
            eng.decode(1)
            lg.append(eng.fetch_logits().copy())
        eng.release()
        plain = _continuous_text(eng, prompts, 0)
        with_lp = _continuous_text(eng, prompts, 4)
        eng.close()
        assert plain[3] >= 1, 'no mixed step: the admission of the third prompt must ride on a decode step'
        out.append((np.stack(lg), plain, with_lp))
    assert np.array_equal(out[0][0].view(np.uint16), out[1][0].view(np.uint16)), 'static batch: logits differ'
    for k, what in ((1, 'continuous batching'), (2, 'continuous batching with logprobs')):
        a, b = out[0][k], out[1][k]
        assert np.array_equal(a[0], b[0]), f'{what}: residual streams differ'
        assert np.array_equal(a[1], b[1]), f'{what}: tokens differ'
        assert len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])), f'{what}: logprob records differ'
        assert a[3] == b[3]
    assert len(out[0][2][2]) == 12


@pytest.mark.parametrize('kv_bits', [8, 16])
def test_embeddings_on_a_model_without_sections(cuda, kv_bits):
    """(k) a tiny Llama: rows substituted, positions linear"""
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, kv_bits=kv_bits,
                        rope=o.RopeParam(128, 10000.0))
    w = o.make_synthetic_weights(cfg, seed=5)
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, 1024, n).astype(np.int32) for n in (40, 7)]
    mm = [dict(emb={p: (0.05 * rng.standard_normal(256)).astype(f16) for p in list(range(3, 20)) + [39]}), None]
    eng = make_engine(cfg, w, kv_bits, max_batch=2, max_prefill=32)
    logits, ref, _ = run_wave(eng, cfg, w, prompts, mm, 2, kv_bits, f'llama kv {kv_bits} embeddings', sections=None)
    eng.close()
    plain = Q.PerSequenceVLOracle(cfg, w, [None, None], SESSION, None, SESSION + 1)
    _, lg = plain.forward(prompts)
    gap = max_diff(logits[0], lg)
    print(f'[qwen-vl] llama: engine vs an oracle without the rows {gap}')
    assert gap[0] > LOGIT_BOUND and gap[1] <= LOGIT_BOUND


def test_engine_refusals(cuda):
    """(l) every refusal of tm_engine_set_multimodal, by name; what the engine refuses when it is created"""
    cfg = tiny_cfg(8)
    w = sensitive_weights(cfg)
    eng = make_engine(cfg, w, 8)
    rows = np.zeros((4, 256), f16)
    pos = np.zeros((3, 4), np.int32)

    def refused(e, item, *words):
        with pytest.raises(_ffi.TmError) as ei:
            e.set_multimodal([dict(prompt_len=10, **item)])
        assert all(wd in str(ei.value) for wd in words), str(ei.value)
    refused(eng, dict(input_embeddings=[rows[:2], rows[2:]], input_embedding_ranges=[(5, 7), (2, 4)]), 'unsorted or overlapping')
    refused(eng, dict(input_embeddings=[rows[:2], rows[2:]], input_embedding_ranges=[(2, 4), (3, 5)]), 'unsorted or overlapping')
    refused(eng, dict(input_embeddings=[rows], input_embedding_ranges=[(8, 12)]), 'outside the prompt')
    refused(eng, dict(input_embeddings=[rows], input_embedding_ranges=[(2, 5)]), 'do not add up')
    refused(eng, dict(mrope_position_ids=np.zeros((3, 11), np.int32)), 'n_pos larger')
    refused(eng, dict(mrope_position_ids=pos - 1), 'negative')
    refused(eng, dict(mrope_position_delta=-11), 'position_delta')
    # a prefill whose batch or lengths differ from the armed input is refused, and the input is spent or cleared either way
    eng.set_multimodal([dict(prompt_len=10, mrope_position_ids=pos)])
    with pytest.raises(_ffi.TmError, match='prompt_len differs'):
        eng.prefill([np.arange(9, dtype=np.int32)], max_new_tokens=2)
    eng.release()
    # a prefill that fails before it looks at the input (too long for the session) spends it all the same: the next prefill is plain
    eng.set_multimodal([dict(prompt_len=10, mrope_position_ids=pos)])
    with pytest.raises(_ffi.TmError, match='session_len'):
        eng.prefill([np.arange(10, dtype=np.int32)], max_new_tokens=SESSION)
    eng.prefill([np.arange(9, dtype=np.int32)], max_new_tokens=2)
    eng.release()
    eng.set_multimodal([dict(prompt_len=10, mrope_position_ids=pos)])
    with pytest.raises(_ffi.TmError, match='continuous batching'):
        eng.submit(np.arange(9, dtype=np.int32), 2, -1, None, None)
    with pytest.raises(_ffi.TmError, match='tm_engine_score'):
        eng.score([np.arange(9, dtype=np.int32)])
    eng.set_multimodal(None)
    eng.prefill([np.arange(9, dtype=np.int32)], max_new_tokens=2)
    with pytest.raises(_ffi.TmError, match='before tm_engine_prefill'):
        eng.set_multimodal([dict(prompt_len=10, mrope_position_ids=pos)])
    eng.close()
    # a model without sections takes embeddings, not coordinates or a delta
    plain = tiny_cfg(8, None)
    eng = make_engine(plain, w, 8)
    refused(eng, dict(mrope_position_ids=pos), 'without mrope_section')
    refused(eng, dict(mrope_position_delta=2), 'without mrope_section')
    eng.set_multimodal([dict(prompt_len=10, input_embeddings=[rows], input_embedding_ranges=[(2, 6)])])
    eng.close()
    # TurboQuant KV; tp > 1 (never started: the refusal needs no device state)
    eng = make_engine(cfg, w, 42)
    refused(eng, dict(mrope_position_ids=pos), 'quant_policy 42')
    eng.close()
    eng = Engine.from_model_config(cfg, tp=2, rank=0, max_batch_size=2, session_len=SESSION, quant_policy=8)
    refused(eng, dict(mrope_position_ids=pos), 'tp > 1')
    eng.close()
    # the sections themselves (tm_engine_set_mrope_section)
    for change, word in ((dict(mrope_section=(16, 24, 20)), 'sum to head_dim / 2'), (dict(mrope_section=(-8, 48, 24)), 'non-negative'),
                         (dict(mrope_section=(8, 12, 12), head_dim=64, q_heads=8, kv_heads=2), 'head_dim 128'),
                         (dict(rope=dataclasses.replace(cfg.rope, type='dynamic', factor=2.0)), 'rope_type 4')):
        with pytest.raises(_ffi.TmError) as ei:
            Engine.from_model_config(dataclasses.replace(cfg, **change), max_batch_size=2, session_len=SESSION, quant_policy=8)
        assert word in str(ei.value), str(ei.value)


@pytest.mark.parametrize('quant_policy', [0, 8])
def test_toy_checkpoint_through_pipeline(cuda, quant_policy):
    """(m) the toy transformers Qwen2-VL checkpoint (fp16) through pipeline(path) without model_format; the dict prompt from
    vl.Qwen2VLVision; greedy tokens against transformers fed the same embeddings and coordinates (teacher-forced with the engine's
    tokens): top-1, or top-2 when the margin is at most 6e-2.  A text-only call gives the tokens of the same weights saved as
    Qwen2ForCausalLM."""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    t = Q.toy(0, qk_scale=8.0)
    model = t['model']
    N = 6
    pv = np.random.default_rng(9).standard_normal((24, 3 * 2 * 14 * 14)).astype(f32)
    prompt = vl.Qwen2VLVision(t['nested'], 'cpu').prompt(Q.TOY_PROMPT, pv, Q.TOY_GRID)
    pipe = pipeline(t['nested'], backend_config=TurbomindEngineConfig(quant_policy=quant_policy, max_batch_size=2, session_len=128))
    assert pipe.model_cfg.mrope_section == Q.SECTIONS
    g = GenerationConfig(max_new_tokens=N, ignore_eos=True)
    text = [7, 8, 9, 10, 11, 12, 13]
    got, got_text = [r.token_ids for r in pipe([prompt, text], g)]
    pipe.close()
    n = len(Q.TOY_PROMPT)
    ids = Q.TOY_PROMPT + got
    pos = np.concatenate([prompt['mrope_position_ids'], np.broadcast_to(np.arange(n, n + N) + prompt['mrope_position_delta'], (3, N))], 1)
    emb = {3 + i: prompt['input_embeddings'][0][i] for i in range(6)}
    ref = Q.hf_logits(model, ids, emb, pos)
    ref_text = Q.hf_logits(model, text + got_text, {}, np.broadcast_to(np.arange(len(text) + N), (3, len(text) + N)))
    for name, toks, lg, n0 in (('image', got, ref, n), ('text', got_text, ref_text, len(text))):
        for s in range(N):
            row = lg[n0 - 1 + s]
            top = np.argsort(row)[::-1][:2]
            margin = row[top[0]] - row[top[1]]
            assert toks[s] == top[0] or (margin <= 6e-2 and toks[s] == top[1]), (name, s, toks[s], top, margin)
