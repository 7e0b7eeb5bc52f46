"""Qwen2-VL / Qwen2.5-VL on the CPU: the M-RoPE / embedding contract (tests/qwen_vl_reference.py) against the installed transformers,
vl.mrope_positions against transformers' get_rope_index, the reader on both on-disk forms, its refusals, and the dict prompt of
Pipeline through the fake engine of tests/test_pipeline_host.py."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, vl
from lmdeploy_amd.turbomind import checkpoint
from tests import qwen_vl_reference as Q
from tests import test_pipeline_host as TPH

f16, f32 = np.float16, np.float32

# ---- (a) the contract against transformers ----------------------------------------------------------------------------------------------
# The toy's q / k projections are scaled by 8 (sharper attention: with the initialiser's weights the attention is nearly uniform and
# swapping h and w moves the logits by 0.002 .. 0.004).  Measured on the CPU, the 13-token prompt (one 1 x 4 x 6 image), KV unquantised,
# max |logit difference| over all 13 rows (|logits| up to 1.4): seeds 0 / 1 / 2 -> 0.00437 / 0.00275 / 0.00329, the same for both on-disk
# forms (they hold the same numbers).  Bound = twice the largest.
# The mutations, on the same model (seed 0) with a 1 x 8 x 12 image (24 image tokens, 35-token prompt; own difference 0.00382): linear
# coordinates 1.51, h and w swapped 0.64, sections read as (24, 24, 16) 0.34, embedding override dropped 1.45.  (On the 13-token prompt
# the sections mutation reaches only 0.061 < 10 x the bound: the 2 x 3 grid's h and w differ by at most 2.)
QK_SCALE = 8.0
HF_BOUND = 2 * 0.00437
BIG_GRID = [[1, 8, 12]]
BIG_PROMPT = [1, 2, Q.VSTART] + [Q.IMAGE] * 24 + [Q.VEND, 7, 8, 9, 10, 11]
MUTATIONS = ('linear', 'swap_hw', 'sections', 'no_embeddings')


def _case(seed, ids, grid):
    """-> (model dict, transformers' coordinates and delta, {position: fp16 image row}, transformers' logits)"""
    t = Q.toy(seed, qk_scale=QK_SCALE)
    pos, delta = Q.hf_rope_index(t['model'], ids, grid)
    n_img = ids.count(Q.IMAGE)
    pv = np.random.default_rng(seed).standard_normal((n_img * 4, 3 * 2 * 14 * 14)).astype(f32)
    feats = Q.hf_image_features(t['model'], pv, grid).astype(f16)
    first = ids.index(Q.IMAGE)
    emb = {first + i: feats[i] for i in range(n_img)}
    return t, pos, delta, emb, Q.hf_logits(t['model'], ids, emb, pos)


def _contract_logits(path, ids, coords, delta, emb, sections=None):
    mc, slots = Q.load_through_reader(path)
    om = Q.VLSeqModel(Q.oracle_config(mc), Q.weights_from_slots(slots, mc), batch=1, max_ctx=64)
    om.setup(sections or mc.mrope_section, 65, coords=coords, delta=delta, emb=emb).forward([ids])
    return om.all_logits.astype(f32), mc


@pytest.mark.parametrize('form', ['nested', 'published'])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_contract_against_transformers(form, seed):
    """the numpy contract on the slots read_config + load_hf_weights + export_weights make of the checkpoint, against the toy
    Qwen2VLForConditionalGeneration (fp32, eager) fed inputs_embeds + 3-D position_ids"""
    t, pos, delta, emb, ref = _case(seed, Q.TOY_PROMPT, Q.TOY_GRID)
    assert pos.tolist() == [[0, 1, 2, 3, 3, 3, 3, 3, 3, 6, 7, 8, 9], [0, 1, 2, 3, 3, 3, 4, 4, 4, 6, 7, 8, 9],
                            [0, 1, 2, 3, 4, 5, 3, 4, 5, 6, 7, 8, 9]] and delta == -3
    got, mc = _contract_logits(t[form], Q.TOY_PROMPT, pos, delta, emb)
    d = np.abs(got - ref).max()
    print(f'{form} seed {seed}: max |logit diff| {d:.5f} (bound {HF_BOUND:.5f})')
    assert d <= HF_BOUND
    assert mc.mrope_section == Q.SECTIONS and mc.arch == 'qwen2' and mc.attn_bias == 1


@pytest.mark.parametrize('mut', MUTATIONS)
def test_contract_comparison_notices_mutations(mut):
    t, pos, delta, emb, ref = _case(0, BIG_PROMPT, BIG_GRID)
    own = np.abs(_contract_logits(t['nested'], BIG_PROMPT, pos, delta, emb)[0] - ref).max()
    n = len(BIG_PROMPT)
    coords, rows, sections = pos, emb, None
    if mut == 'linear':
        coords = np.broadcast_to(np.arange(n), (3, n))
    elif mut == 'swap_hw':
        coords = pos[[0, 2, 1]]
    elif mut == 'sections':
        sections = (24, 24, 16)
    else:
        rows = {}
    d = np.abs(_contract_logits(t['nested'], BIG_PROMPT, coords, delta, rows, sections)[0] - ref).max()
    print(f'{mut}: max |logit diff| {d:.4f} (unmutated {own:.5f}, bound {HF_BOUND:.5f})')
    assert own <= HF_BOUND and d > 10 * HF_BOUND


# ---- (b) mrope_positions against transformers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ids,grid', [
    (Q.TOY_PROMPT, Q.TOY_GRID),
    ([1, Q.VSTART] + [Q.IMAGE] * 6 + [Q.VEND, 7, 8, Q.VSTART] + [Q.IMAGE] * 8 + [Q.VEND, 9], [[1, 4, 6], [1, 8, 4]]),     # two images
    ([Q.VSTART] + [Q.IMAGE] * 4 + [Q.VEND], [[1, 4, 4]]),                                                                    # image first
    ([1, 2, 3, 7], None)])                                                                                                   # text only
def test_mrope_positions_equal_transformers(ids, grid):
    model = Q.toy(0, qk_scale=QK_SCALE)['model']
    got, delta = vl.mrope_positions(ids, grid, Q.IMAGE, 2)
    if grid is None:
        assert got.tolist() == [list(range(len(ids)))] * 3 and delta == 0
        return
    want, want_delta = Q.hf_rope_index(model, ids, grid)
    assert got.dtype == np.int32 and np.array_equal(got, want) and delta == want_delta


def test_mrope_positions_refusals():
    with pytest.raises(NotImplementedError, match='video'):
        vl.mrope_positions(Q.TOY_PROMPT, Q.TOY_GRID, Q.IMAGE, 2, video_grid_thw=[[2, 4, 4]])
    with pytest.raises(ValueError, match='run of 6 image tokens'):
        vl.mrope_positions(Q.TOY_PROMPT[:6] + [9] * 7, Q.TOY_GRID, Q.IMAGE, 2)
    with pytest.raises(ValueError, match='image grids'):
        vl.mrope_positions(Q.TOY_PROMPT, Q.TOY_GRID + [[1, 2, 2]], Q.IMAGE, 2)


def test_vision_tower_prompt():
    """Qwen2VLVision loads the tower alone, from either prefix, and its prompt() is transformers' features + coordinates"""
    t = Q.toy(0, qk_scale=QK_SCALE)
    pv = np.random.default_rng(5).standard_normal((24, 3 * 2 * 14 * 14)).astype(f32)
    want = Q.hf_image_features(t['model'], pv, Q.TOY_GRID).astype(f16)
    pos, delta = Q.hf_rope_index(t['model'], Q.TOY_PROMPT, Q.TOY_GRID)
    for form in ('nested', 'published'):
        p = vl.Qwen2VLVision(t[form], 'cpu').prompt(Q.TOY_PROMPT, pv, Q.TOY_GRID)
        assert p['input_embedding_ranges'] == [(3, 9)] and p['mrope_position_delta'] == delta
        assert np.array_equal(p['mrope_position_ids'], pos) and p['input_ids'].tolist() == Q.TOY_PROMPT
        assert np.abs(p['input_embeddings'][0].astype(f32) - want.astype(f32)).max() <= 2.0**-9 * np.abs(want.astype(f32)).max()


# ---- (c) reader ------------------------------------------------------------------------------------------------------------------------------
def test_both_forms_give_identical_slots_and_awq_loads(tmp_path):
    t = Q.toy(0, qk_scale=QK_SCALE)
    (mc_a, a), (mc_b, b) = Q.load_through_reader(t['nested']), Q.load_through_reader(t['published'])
    assert mc_a == mc_b and mc_a.mrope_section == Q.SECTIONS and not mc_a.quantized
    assert set(a) == set(b) and not any('visual' in k for k in a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the same weights as Qwen2ForCausalLM (language tensors under model., no sections): the same slots
    from safetensors.numpy import load_file, save_file
    plain = tmp_path / 'plain'
    plain.mkdir()
    tensors = {k: v for k, v in load_file(os.path.join(t['published'], 'model.safetensors')).items() if not k.startswith('visual.')}
    save_file(tensors, str(plain / 'model.safetensors'))
    c = json.load(open(os.path.join(t['published'], 'config.json')))
    c.update(architectures=['Qwen2ForCausalLM'], head_dim=128)
    c.pop('rope_scaling')
    json.dump(c, open(plain / 'config.json', 'w'))
    mc_p, p = Q.load_through_reader(str(plain))
    assert mc_p.mrope_section is None and all(np.array_equal(a[k], p[k]) for k in a)
    # AWQ language model, fp16 vision tower
    for form in ('nested', 'published'):
        path = Q.write_checkpoint(t['model'], str(tmp_path / f'awq_{form}'), form, awq=True)
        mc, slots = Q.load_through_reader(path)
        assert mc.quantized and mc.weight_format == 'u4' and mc.mrope_section == Q.SECTIONS
        assert slots['layers.1.attention.w_qkv.qweight'].dtype == np.int32 and slots['layers.0.attention.w_qkv.bias'].shape == (512,)


def _config(**change):
    c = json.load(open(os.path.join(Q.toy(0, qk_scale=QK_SCALE)['published'], 'config.json')))
    c.update(change)
    return c


@pytest.mark.parametrize('change,needle', [
    (dict(architectures=['Qwen3VLForConditionalGeneration']), 'Qwen3-VL'),
    (dict(architectures=['Qwen3VLMoeForConditionalGeneration']), 'Qwen3-VL'),
    (dict(rope_scaling=dict(type='mrope', mrope_section=[16, 24, 20])), 'mrope_section'),
    (dict(rope_scaling=dict(type='mrope', mrope_section=[16, 48])), 'mrope_section'),
    (dict(rope_scaling=dict(type='mrope', mrope_section=[-8, 48, 24])), 'mrope_section'),
    (dict(rope_scaling=dict(type='mrope')), 'mrope_section'),
    (dict(hidden_size=128, num_attention_heads=2, rope_scaling=dict(type='mrope', mrope_section=[8, 12, 12])), 'head_dim 64'),
    (dict(rope_scaling=dict(type='yarn', factor=4.0, mrope_section=[16, 24, 24])), 'yarn'),
    (dict(rope_scaling=dict(rope_type='dynamic', factor=2.0, mrope_section=[16, 24, 24])), 'dynamic'),
    (dict(use_sliding_window=True), 'use_sliding_window')])
def test_reader_refusals_name_their_reason(tmp_path, change, needle):
    json.dump(_config(**change), open(tmp_path / 'config.json', 'w'))
    with pytest.raises(NotImplementedError, match=needle):
        checkpoint.read_config(str(tmp_path))


def test_qwen2_5_vl_config_reads_like_qwen2_vl(tmp_path):
    json.dump(_config(architectures=['Qwen2_5_VLForConditionalGeneration']), open(tmp_path / 'config.json', 'w'))
    mc = checkpoint.read_config(str(tmp_path))
    assert mc.mrope_section == Q.SECTIONS and mc.arch == 'qwen2' and mc.rope.base == 10000.0 and mc.rope.type == 'default'


# ---- (d) pipeline host plumbing -----------------------------------------------------------------------------------------------------------
class FakeVLEngine(TPH.FakeEngine):
    def __init__(self, *a):
        super().__init__(*a)
        self.mm_calls, self.calls = [], []

    def set_multimodal(self, inputs):
        self.mm_calls.append(inputs)

    def prefill(self, prompts, max_new_tokens):
        self.calls.append('prefill')
        super().prefill(prompts, max_new_tokens)

    def submit(self, *a, **kw):
        self.calls.append('submit')
        return super().submit(*a, **kw)


@pytest.fixture
def vl_pipe(monkeypatch):
    monkeypatch.setattr(TPH.P, 'Engine', FakeVLEngine)
    TPH.FakeEngine.instances.clear()
    p = TPH.P.Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(max_batch_size=2, session_len=64, quant_policy=8))
    p.model_cfg.mrope_section = Q.SECTIONS
    yield p
    p.close()


def _dict_prompt(hidden, **change):
    ids = np.asarray(Q.TOY_PROMPT)
    pos, delta = vl.mrope_positions(ids, Q.TOY_GRID, Q.IMAGE, 2)
    rows = np.arange(6 * hidden, dtype=f32).reshape(6, hidden).astype(f16)
    p = dict(input_ids=ids, input_embeddings=[rows[:2], rows[2:]], input_embedding_ranges=[(3, 5), (5, 9)], mrope_position_ids=pos,
             mrope_position_delta=delta)
    p.update(change)
    return p


def test_dict_prompt_reaches_set_multimodal(vl_pipe):
    hidden = vl_pipe.model_cfg.hidden
    p = _dict_prompt(hidden)
    g = GenerationConfig(max_new_tokens=4, ignore_eos=True)
    out = vl_pipe([p, [5, 6, 7]], g)
    eng = TPH.FakeEngine.instances[-1]
    assert eng.calls == ['prefill'] and len(eng.mm_calls) == 1
    mm, text = eng.mm_calls[0]
    assert mm['prompt_len'] == 13 and mm['input_embedding_ranges'] == [(3, 5), (5, 9)] and mm['mrope_position_delta'] == -3
    assert np.array_equal(mm['mrope_position_ids'], p['mrope_position_ids']) and mm['mrope_position_ids'].dtype == np.int32
    assert [e.dtype for e in mm['input_embeddings']] == [f16, f16]
    assert np.array_equal(np.concatenate(mm['input_embeddings']), np.concatenate(p['input_embeddings']))
    assert text == dict(prompt_len=3)
    assert [r.token_ids for r in out] == [TPH._expect(Q.TOY_PROMPT, 4)[0], TPH._expect([5, 6, 7], 4)[0]]
    # a single dict is one prompt; a dict without multimodal content is a plain prompt (no set_multimodal)
    r = vl_pipe(dict(input_ids=[5, 6, 7]), g)
    assert r.token_ids == TPH._expect([5, 6, 7], 4)[0] and len(eng.mm_calls) == 1


@pytest.mark.parametrize('change,needle', [
    (dict(input_embedding_ranges=[(5, 7), (3, 7)]), 'unsorted or overlaps'),      # (each range as long as its array: the order is at fault)
    (dict(input_embedding_ranges=[(3, 5), (4, 8)]), 'unsorted or overlaps'),
    (dict(input_embedding_ranges=[(3, 5), (9, 14)]), 'inside the prompt'),
    (dict(input_embedding_ranges=[(3, 5)]), '2 input_embeddings for 1'),
    (dict(input_embedding_ranges=[(3, 5), (5, 8)]), 'shape'),
    (dict(mrope_position_ids=np.zeros((3, 14), np.int32)), 'mrope_position_ids'),
    (dict(mrope_position_ids=-np.ones((3, 4), np.int32)), 'mrope_position_ids'),
    (dict(mrope_position_delta=-14), 'mrope_position_delta'),
    (dict(pixel_values=1), 'unknown keys')])
def test_malformed_dict_prompts_raise_before_any_engine_call(vl_pipe, change, needle):
    with pytest.raises(ValueError, match=needle):
        vl_pipe(_dict_prompt(vl_pipe.model_cfg.hidden, **change), GenerationConfig(max_new_tokens=2))
    eng = TPH.FakeEngine.instances[-1]
    assert eng.calls == [] and eng.mm_calls == []


def test_requests_that_cannot_run_as_a_static_batch_refuse_multimodal_input(vl_pipe):
    p = _dict_prompt(vl_pipe.model_cfg.hidden)
    g = GenerationConfig(max_new_tokens=2)
    with pytest.raises(NotImplementedError, match='max_batch_size'):
        vl_pipe([p, p, p], g)
    with pytest.raises(NotImplementedError, match='one GenerationConfig per prompt'):
        vl_pipe([p, [1, 2]], [g, g])
    with pytest.raises(NotImplementedError, match='continuous batching'):
        list(vl_pipe.stream_infer([p], g))
    vl_pipe.backend_config.tp = 2
    with pytest.raises(NotImplementedError, match='tp > 1'):
        vl_pipe(p, g)
    vl_pipe.backend_config.tp = 1
    vl_pipe.backend_config.quant_policy = 42
    with pytest.raises(NotImplementedError, match='quant_policy=42'):
        vl_pipe(p, g)
    vl_pipe.backend_config.quant_policy = 8
    vl_pipe.model_cfg.mrope_section = None
    with pytest.raises(ValueError, match='without M-RoPE sections'):
        vl_pipe(p, g)
    eng = TPH.FakeEngine.instances[-1]
    assert eng.calls == [] and eng.mm_calls == []


def test_a_refused_or_failed_call_leaves_nothing_armed(vl_pipe):
    """the output_logits refusal comes before anything is handed to the engine; set_multimodal is the last call in front of the prefill
    that consumes its input (the engine drops it when that prefill fails), so a later text-only chunk cannot meet it"""
    p = _dict_prompt(vl_pipe.model_cfg.hidden)
    eng = TPH.FakeEngine.instances[-1]
    order = []
    for name in ('set_sampling', 'set_logits_params', 'set_logprobs', 'set_multimodal', 'prefill'):
        def spy(*a, _f=getattr(eng, name), _n=name, **kw):
            order.append(_n)
            return _f(*a, **kw)
        setattr(eng, name, spy)
    with pytest.raises(NotImplementedError, match='output_logits'):
        vl_pipe(p, GenerationConfig(max_new_tokens=2, output_logits='generation', bad_token_ids=[5]))
    assert order == [] and eng.mm_calls == []
    vl_pipe(p, GenerationConfig(max_new_tokens=2))
    assert order[-2:] == ['set_multimodal', 'prefill'] and len(eng.mm_calls) == 1
    order.clear()
    vl_pipe([5, 6, 7], GenerationConfig(max_new_tokens=2))
    assert 'set_multimodal' not in order and order[-1] == 'prefill'


def test_embedding_rows_are_padded_to_the_engine_width():
    """a model served zero-padded (gpt-oss: hidden 2880 run at 2944) takes rows of its own width; the pad columns are +0"""
    from lmdeploy_amd.turbomind.engine import pack_embedding_rows
    a, b = np.ones((2, 2880), f16), np.full((3, 2880), 2, f16)
    rows = pack_embedding_rows([a, b], 2944, 2880)
    assert rows.shape == (5, 2944) and rows.dtype == f16 and np.all(rows[:2, :2880] == 1) and np.all(rows[2:, :2880] == 2)
    assert not rows[:, 2880:].view(np.uint16).any()
    assert pack_embedding_rows([], 256, 256).shape == (0, 256) and np.array_equal(pack_embedding_rows([a[:, :256]], 256, 256), a[:, :256])
    with pytest.raises(ValueError, match='hidden size 2880'):
        pack_embedding_rows([np.ones((2, 2944), f16)], 2944, 2880)
