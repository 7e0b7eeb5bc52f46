"""The KV block ring of sliding-window engines against the same build with TM_KV_RING=0, bit for bit: a ring engine
runs the same kernels on the same values, only the block table repeats R = ceil((W - 1 + C) / 64) + 1 physical blocks.  The model is
pipeline.SYNTHETIC['tiny']'s geometry with a window of 40 in both layers, max_prefill_token_num = 64 (C = 64, R = 3), session_len 512.
No tolerance anywhere: logits, NLLs, cache bytes and tokens are compared for equality."""
import numpy as np
import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.messages import GenerationConfig, TurbomindEngineConfig
from lmdeploy_amd.pipeline import Pipeline
from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests.attention_window_reference import WindowConfig, make_window_weights

pytestmark = pytest.mark.gpu
W, R, SESSION = 40, 3, 512
OOM, INVALID = 11, 1
_WEIGHTS = {}


def _cfg(kv_bits, **over):
    base = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, kv_bits=kv_bits,
                rope=o.RopeParam(128, 10000.0), window=W)
    base.update(over)
    return WindowConfig(**base)


def _engine(monkeypatch, ring, cfg, batch, use_graph=1, cache_blocks=0):
    """TM_KV_RING is read when the engine is created"""
    monkeypatch.setenv('TM_KV_RING', str(ring))
    key = (cfg.kv_bits, cfg.window, getattr(cfg, 'layer_windows', None))
    if key not in _WEIGHTS:
        _WEIGHTS[key] = export_weights(cfg, make_window_weights(cfg, seed=5))
    eng = Engine.from_model_config(cfg, max_batch_size=batch, session_len=SESSION, quant_policy=0 if cfg.kv_bits == 16 else cfg.kv_bits,
                                   max_prefill_token_num=64, use_graph=use_graph, cache_blocks=cache_blocks)
    eng.load_weights(_WEIGHTS[key])
    eng.start()
    return eng


def _prompts(lens, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1024, n).astype(np.int32) for n in lens]


def _owned(eng):
    return eng.stats()['num_blocks'] - eng.kv_info()['free_blocks']


def _run(eng, prompts, max_new, steps):
    """logits behind the prefill and behind every decode step, the tokens, the blocks the batch owned"""
    eng.prefill(prompts, max_new_tokens=max_new)
    owned = _owned(eng)
    logits = [eng.fetch_logits().copy()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
    return np.stack(logits).view(np.uint16), eng.fetch().copy(), owned


@pytest.mark.parametrize('use_graph', [0, 1])
@pytest.mark.parametrize('kv_bits', [8, 16])
def test_ring_aliasing_in_prefill_and_decode(cuda, monkeypatch, kv_bits, use_graph):
    """250 tokens in four chunks wrap the 192-token ring (logical block 3 lands on block 0); the eight decode steps cross position 256
    into logical block 4 = ring[1].  Whole contexts: 5 + 2 + 1 blocks, rings: 3 + 2 + 1."""
    cfg, prompts = _cfg(kv_bits), _prompts((250, 70, 5))
    out = {}
    for ring in (0, 1):
        eng = _engine(monkeypatch, ring, cfg, 3, use_graph)
        assert eng.kv_info()['ring_blocks'] == (R if ring else 0)
        out[ring] = _run(eng, prompts, 9, 8)
        eng.close()
    assert out[0][2] == 8 and out[1][2] == 6
    assert np.array_equal(out[1][1], out[0][1]), 'generated tokens differ'
    for s in range(9):
        assert np.array_equal(out[1][0][s], out[0][0][s]), f'step {s}: {np.count_nonzero(out[1][0][s] != out[0][0][s])} logits differ'


@pytest.mark.parametrize('kv_bits', [8, 16])
def test_score_and_continuous_batching(cuda, monkeypatch, kv_bits):
    """tm_engine_score of 300 + 70 tokens (5 chunks through a 3-block ring) and the scheduler path: six requests through two slots,
    the long ones wrapping their rings while they decode next to an admission's prefill.  The pool (32 blocks) never limits an
    admission under either setting, so both engines run the same schedule."""
    cfg = _cfg(kv_bits)
    seqs = _prompts((300, 70), seed=3)
    lens, news = (250, 70, 5, 300, 33, 129), (9, 12, 3, 20, 6, 70)
    prompts = _prompts(lens, seed=4)
    got = {}
    for ring in (0, 1):
        eng = _engine(monkeypatch, ring, cfg, 2, cache_blocks=32)
        nll = [x.copy().view(np.uint32) for x in eng.score(seqs)]
        assert _owned(eng) == 0
        ids = [eng.submit(p, n, -1, None, None) for p, n in zip(prompts, news)]
        n_active, _ = eng.step()
        # request 0 runs (a ring of 3 blocks, a whole context of 5), request 1 next to it or not yet (2 blocks either way); one block
        # parks the free slots
        assert n_active in (1, 2) and _owned(eng) == 1 + (3 if ring else 5) + 2 * (n_active - 1)
        done, steps = {}, 1
        while len(done) < len(ids):
            eng.step()
            steps += 1
            assert steps < 400, 'scheduler does not make progress'
            for i, rid in enumerate(ids):
                if i not in done:
                    status, toks = eng.poll(rid)
                    if status != 0:
                        done[i] = (status, toks.copy())
        eng.close()
        got[ring] = (nll, done)
    for a, b in zip(got[1][0], got[0][0]):
        assert np.array_equal(a, b), 'NLLs differ'
    for i, n in enumerate(news):
        assert got[1][1][i][0] == 7 and len(got[1][1][i][1]) == n
        assert np.array_equal(got[1][1][i][1], got[0][1][i][1]), f'request {i}: tokens differ'


def test_capacity_beyond_whole_contexts(cuda, monkeypatch):
    """8 blocks, two prompts of 300 tokens, max_new_tokens 20: 2 x 5 blocks whole-context, 2 x 3 as rings.  The ring engine prefills and
    generates all 20 tokens (the prefill's and 19 decode steps: a session of max_new_tokens 20 has no more); its logits are those of a
    TM_KV_RING=0 engine with 32 blocks.  TM_KV_RING=0 on 8 blocks: TM_OOM, as before."""
    cfg, prompts = _cfg(8), _prompts((300, 300), seed=7)
    eng = _engine(monkeypatch, 0, cfg, 2, cache_blocks=8)
    with pytest.raises(_ffi.TmError) as err:
        eng.prefill(prompts, max_new_tokens=20)
    assert err.value.status == OOM
    eng.close()
    eng = _engine(monkeypatch, 0, cfg, 2, cache_blocks=32)
    ref = _run(eng, prompts, 20, 19)
    eng.close()
    eng = _engine(monkeypatch, 1, cfg, 2, cache_blocks=8)
    got = _run(eng, prompts, 20, 19)
    eng.release()
    assert _owned(eng) == 0
    eng.close()
    assert ref[2] == 10 and got[2] == 6
    assert np.array_equal(got[1], ref[1]) and got[1].shape == (2, 20)
    assert np.array_equal(got[0], ref[0]), 'logits differ'


@pytest.mark.parametrize('over', [dict(window=0), dict(layer_windows=(W, 0))], ids=['no window', 'one full-attention layer'])
def test_engines_without_a_window_in_every_layer_keep_whole_contexts(cuda, monkeypatch, over):
    cfg, prompts = _cfg(8, **over), _prompts((250, 70, 5))
    out = {}
    for ring in (0, 1):
        eng = _engine(monkeypatch, ring, cfg, 3)
        assert eng.kv_info()['ring_blocks'] == 0
        out[ring] = _run(eng, prompts, 9, 8)
        eng.close()
    assert out[0][2] == 8 and out[1][2] == 8
    assert np.array_equal(out[1][1], out[0][1]) and np.array_equal(out[1][0], out[0][0])


def test_a_window_as_long_as_the_session_is_full_attention(cuda, monkeypatch):
    eng = _engine(monkeypatch, 1, _cfg(8, window=SESSION), 1)
    assert eng.kv_info()['ring_blocks'] == 0
    eng.close()


def test_debug_fetch_of_resident_and_overwritten_blocks(cuda, monkeypatch):
    """250 cached tokens: logical blocks 0 .. 3 are written, the ring holds 1 .. 3 (block 0 was overwritten by block 3).  After eight
    decode steps (258 tokens) block 4 has taken block 1's place.  Full blocks are compared: the unwritten tail of a partly filled
    block holds the pool's zeros on one engine and an older block's tokens on the other."""
    cfg, prompts = _cfg(8), _prompts((250, 70))
    engs = {ring: _engine(monkeypatch, ring, cfg, 2) for ring in (0, 1)}
    for e in engs.values():
        e.prefill(prompts, max_new_tokens=9)
    for blk in (1, 2):
        assert np.array_equal(engs[1].fetch_kv_block(0, blk), engs[0].fetch_kv_block(0, blk)), f'block {blk}'
    assert np.array_equal(engs[1].fetch_kv_block(1, 0), engs[0].fetch_kv_block(1, 0))      # 79 tokens: 2 blocks, no wrap
    with pytest.raises(_ffi.TmError) as err:
        engs[1].fetch_kv_block(0, 0)
    assert err.value.status == INVALID
    engs[0].fetch_kv_block(0, 0)                                                          # whole contexts: every block stays
    for e in engs.values():
        e.decode(8)
    for blk in (2, 3):
        assert np.array_equal(engs[1].fetch_kv_block(0, blk), engs[0].fetch_kv_block(0, blk)), f'block {blk}'
    for blk in (0, 1, 5):
        with pytest.raises(_ffi.TmError) as err:
            engs[1].fetch_kv_block(0, blk)
        assert err.value.status == INVALID
    for e in engs.values():
        e.close()


def test_pipeline_generates_beyond_the_pool(cuda, monkeypatch):
    """pipeline('synthetic:tiny_window') on 6 blocks: a 400-token prompt with 20 new tokens is 7 blocks whole-context, 3 as a ring"""
    prompt = _prompts((400,), seed=9)[0].tolist()
    backend = TurbomindEngineConfig(session_len=SESSION, max_batch_size=2, quant_policy=8, max_prefill_token_num=64)
    gen = GenerationConfig(max_new_tokens=20, ignore_eos=True)
    monkeypatch.setenv('TM_KV_RING', '1')
    with Pipeline('synthetic:tiny_window', backend_config=backend, cache_blocks=6) as pipe:
        assert pipe.engine.kv_info()['ring_blocks'] == R and pipe.engine.stats()['num_blocks'] == 6
        res = pipe([prompt], gen)[0]
        model_cfg = pipe.model_cfg
    assert res.finish_reason == 'length' and len(res.token_ids) == 20
    eng = Engine.from_model_config(model_cfg, weight_type=0, max_batch_size=2, session_len=SESSION, quant_policy=8,
                                   max_prefill_token_num=64, cache_blocks=6)
    eng.init_synthetic(seed=0)
    eng.start()
    eng.prefill([np.asarray(prompt, np.int32)], max_new_tokens=20)
    eng.decode(19)
    assert res.token_ids == eng.fetch()[0].tolist()
    eng.close()
    monkeypatch.setenv('TM_KV_RING', '0')
    with Pipeline('synthetic:tiny_window', backend_config=backend, cache_blocks=6) as pipe:
        res = pipe([prompt], gen)[0]
    assert res.finish_reason == 'error' and not res.token_ids
