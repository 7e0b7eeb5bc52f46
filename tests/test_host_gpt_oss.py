"""gpt-oss on the host: the zero-padding functions, YaRN with a fractional correction range against transformers, the
GptOssForCausalLM reader / loader against transformers' own model on a toy checkpoint in both on-disk forms, and the config reader's
fields and refusals.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint, loader
from lmdeploy_amd.turbomind.engine import make_model_config
from tests import gpt_oss_reference as G
from tests import mxfp4_reference as MX

f16, f32 = np.float16, np.float32


@pytest.fixture(scope='module')
def tm():
    return _ffi.load()


# ---- 1. padding -------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if np.asarray(a).dtype == f16 else np.uint8)


def test_pad_mxfp4_linear_dequantises_to_the_zero_padded_original():
    """w1w3 of H 192 -> 256, I 320 -> 384: codes 0x00 and scale bytes 127 in the pad, the interior untouched, and dequant(padded) ==
    zero-padded dequant(original) with +0 (not -0) in every pad element"""
    rng = np.random.default_rng(0)
    lin = MX.random_linear(rng, 192, 640)
    p = loader.pad_mxfp4(lin, 768, 256)
    assert p['blocks'].shape == (768, 128) and p['scales'].shape == (768, 8) and p['blocks'].dtype == p['scales'].dtype == np.uint8
    assert np.array_equal(p['blocks'][:640, :96], lin['blocks']) and np.array_equal(p['scales'][:640, :6], lin['scales'])
    assert not p['blocks'][640:].any() and not p['blocks'][:, 96:].any()
    assert (p['scales'][640:] == 127).all() and (p['scales'][:, 6:] == 127).all()
    want = np.zeros((256, 768), f16)
    want[:192, :640] = MX.dequant(**lin)
    assert np.array_equal(_bits(MX.dequant(**p)), _bits(want))
    same = loader.pad_mxfp4(lin, 640, 192)       # nothing to pad: the same bytes
    assert np.array_equal(same['blocks'], lin['blocks']) and np.array_equal(same['scales'], lin['scales'])


def _unpadded_weights(rng, mx: bool):
    H, I, E, V, nq, nkv = 192, 320, 3, 40, 256, 128

    def r(*s):
        return rng.standard_normal(s).astype(f16)

    def ex():
        if mx:
            return dict(w1w3=MX.random_linear(rng, H, 2 * I), w2=MX.random_linear(rng, I, H), w1w3_bias=r(2 * I), w2_bias=r(H))
        return dict(w1w3=dict(w=r(H, 2 * I)), w2=dict(w=r(I, H)), w1w3_bias=r(2 * I), w2_bias=r(H))
    layer = dict(attn_norm=r(H), ffn_norm=r(H), w_qkv=dict(w=r(H, nq + 2 * nkv)), wo=dict(w=r(nq, H)), wo_bias=r(H),
                 qkv_bias=r(nq + 2 * nkv), sinks=r(4), moe_gate=r(H, E), moe_gate_bias=rng.standard_normal(E).astype(f32),
                 experts=[ex() for _ in range(E)])
    return dict(tok_embeddings=r(V, H), norm=r(H), output=r(H, V), layers=[layer])


@pytest.mark.parametrize('mx', [True, False])
def test_pad_model_weights_shapes_pads_and_interior(mx):
    """every tensor with a hidden or inter axis grows to 256 / 384, every pad element is +0 (MXFP4: code 0x00), the interior keeps its
    bits, tensors without such an axis are the same objects; sizes that are multiples of 128 come back untouched"""
    w = _unpadded_weights(np.random.default_rng(1), mx)
    p = loader.pad_model_weights(w, 192, 320)
    L, P = w['layers'][0], p['layers'][0]

    def check(a, b, shape):
        a, b = np.asarray(a), np.asarray(b)
        assert b.shape == shape and b.dtype == a.dtype
        keep = tuple(slice(0, n) for n in a.shape)
        assert np.array_equal(_bits(b[keep]), _bits(a))
        rest = b.copy()
        rest[keep] = 0
        assert not _bits(rest).any(), 'pad elements must be +0 / code 0x00'
    check(w['tok_embeddings'], p['tok_embeddings'], (40, 256))
    check(w['output'], p['output'], (256, 40))
    check(w['norm'], p['norm'], (256,))
    for k, shape in (('attn_norm', (256,)), ('ffn_norm', (256,)), ('wo_bias', (256,)), ('moe_gate', (256, 3))):
        check(L[k], P[k], shape)
    check(L['w_qkv']['w'], P['w_qkv']['w'], (256, 512))
    check(L['wo']['w'], P['wo']['w'], (256, 256))
    for k in ('qkv_bias', 'sinks', 'moe_gate_bias'):
        assert P[k] is L[k]
    for e, pe in zip(L['experts'], P['experts']):
        check(e['w1w3_bias'], pe['w1w3_bias'], (768,))
        check(e['w2_bias'], pe['w2_bias'], (256,))
        if mx:
            check(e['w1w3']['blocks'], pe['w1w3']['blocks'], (768, 128))
            check(e['w2']['blocks'], pe['w2']['blocks'], (256, 192))
            assert pe['w1w3']['scales'].shape == (768, 8) and pe['w2']['scales'].shape == (256, 12)
            assert (pe['w2']['scales'][192:] == 127).all() and (pe['w2']['scales'][:, 10:] == 127).all()
            assert np.array_equal(pe['w2']['scales'][:192, :10], e['w2']['scales'])
        else:
            check(e['w1w3']['w'], pe['w1w3']['w'], (256, 768))
            check(e['w2']['w'], pe['w2']['w'], (384, 256))
    assert loader.pad_model_weights(w, 256, 384) is w
    with pytest.raises(NotImplementedError, match='fp16 and MXFP4'):
        bad = dict(w, layers=[dict(L, experts=[dict(L['experts'][0], w1w3=dict(q=np.zeros((192, 640), np.uint8)))])])
        loader.pad_model_weights(bad, 192, 320)


def test_padded_gate_up_pair_is_inert():
    """act(0, 0) = 0 * sigmoid(0) * (1 + 0) = 0: the padded (gate, up) columns of w1w3 feed w2's pad rows zeros"""
    assert not MX.gptoss_act(np.zeros((3, 8), f16), np.zeros(8, f16)).any()


def test_make_model_config_hands_over_padded_sizes():
    mc = checkpoint.ModelConfig(hidden=2880, layers=2, q_heads=64, kv_heads=8, head_dim=64, inter=2880, vocab=1024,
                                rope=checkpoint.RopeConfig(64, 150000.0, 'yarn', 32.0, max_position_embeddings=4096, truncate=False),
                                attn_out_bias=1)
    m = make_model_config(mc, 1)
    assert (m.hidden, m.inter, m.hidden_valid, m.attn_out_bias, m.rope_yarn_truncate) == (2944, 2944, 2880, 1, 0)
    assert (mc.hidden, mc.inter) == (2880, 2880)
    m = make_model_config(checkpoint.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024))
    assert (m.hidden, m.inter, m.hidden_valid, m.attn_out_bias, m.rope_yarn_truncate) == (256, 512, 0, 0, 1)
    assert _ffi.ModelConfig(hidden=8).rope_yarn_truncate == 1 and _ffi.RopeParam(dim=64).yarn_truncate == 1


# ---- 2. RoPE ----------------------------------------------------------------------------------------------------------------------
def _inv_freq(tm, **kw):
    p = _ffi.RopeParam(**dict(dict(dim=64, base=150000.0, type=3, factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                   original_max_position=0, max_position_embeddings=4096, yarn_beta_fast=32.0, yarn_beta_slow=1.0,
                                   yarn_attention_factor=1.0), **kw))
    out, af = np.zeros(p.dim // 2, f32), ctypes.c_float()
    _ffi.check(tm.tm_rope_inv_freq(out.ctypes.data, ctypes.byref(af), ctypes.byref(p)))
    return out, af.value


def _hf_yarn(dim, base, factor, original, max_pos, truncate):
    from transformers import GptOssConfig
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    c = GptOssConfig(head_dim=dim, max_position_embeddings=max_pos, num_hidden_layers=2,
                     rope_parameters=dict(rope_type='yarn', rope_theta=base, factor=factor, beta_fast=32.0, beta_slow=1.0,
                                          truncate=truncate, original_max_position_embeddings=original))
    inv, af = ROPE_INIT_FUNCTIONS['yarn'](c, 'cpu')
    return inv.double().numpy(), float(af)


# Both sides compute in fp32 what is a real-valued formula: ours the exponent i * (-log2(base) / dim) (|.| <= log2(base) < 18, one
# rounding of 2^-24 relative -> 18 * 2^-24 * ln 2 = 7.4e-7 relative on freq), transformers base ** (i / dim) (the same size of error
# from the rounded exponent, plus powf's own), then each a handful of fp32 operations on the ramp (<= 2^-24 each).  4e-6 relative covers
# the sum with a factor of two to spare and is 50 times below what separates the truncated from the fractional range.
YARN_REL = 4e-6


@pytest.mark.parametrize('dim,base,factor,original,max_pos', [(64, 150000.0, 32.0, 4096, 131072), (64, 150000.0, 4.0, 32, 128)])
def test_yarn_untruncated_matches_transformers(tm, tmp_path, dim, base, factor, original, max_pos):
    """tm_rope_inv_freq with yarn_truncate = 0 and the correction range over the ORIGINAL length, as the gpt-oss reader passes it,
    against transformers' YaRN inv_freq and attention factor; with yarn_truncate = 1 against transformers' `truncate: true`"""
    c = dict(G.TOY, head_dim=dim, max_position_embeddings=max_pos, torch_dtype='bfloat16',
             rope_parameters=dict(G.TOY['rope_parameters'], rope_theta=base, factor=factor, original_max_position_embeddings=original))
    with open(os.path.join(tmp_path, 'config.json'), 'w') as f:
        json.dump(dict(c, architectures=['GptOssForCausalLM']), f)
    r = checkpoint.read_config(str(tmp_path)).rope
    assert (r.type, r.truncate, r.max_position_embeddings, r.factor) == ('yarn', False, original, factor)
    for trunc in (0, 1):
        got, af = _inv_freq(tm, dim=dim, base=r.base, factor=r.factor, max_position_embeddings=r.max_position_embeddings,
                            yarn_beta_fast=r.beta_fast, yarn_beta_slow=r.beta_slow, yarn_attention_factor=r.attention_factor,
                            yarn_truncate=trunc)
        want, want_af = _hf_yarn(dim, base, factor, original, max_pos, bool(trunc))
        rel = np.abs(got.astype(np.float64) - want) / want
        print(f'dim {dim} original {original} truncate {trunc}: max rel {rel.max():.3e}, attention factor {af} vs {want_af}')
        assert rel.max() <= YARN_REL
        assert abs(af - want_af) <= 2.0**-23 * want_af
    a, b = _hf_yarn(dim, base, factor, original, max_pos, False)[0], _hf_yarn(dim, base, factor, original, max_pos, True)[0]
    assert (np.abs(a - b) / a).max() > 50 * YARN_REL, 'the two correction ranges must differ visibly on these cases'
    assert r.attention_factor == pytest.approx(0.1 * np.log(factor) + 1.0, rel=1e-12)


def test_yarn_truncate_1_is_the_table_as_before(tm):
    """yarn_truncate = 1 (also what a RopeParam built without the field gets) reproduces tests.rope_scaling_reference.yarn_inv_freq, the
    restatement the existing YaRN tests hold the table to, bit for bit; yarn_truncate = 0 differs from it"""
    from tests import rope_scaling_reference as R
    for factor, max_pos, beta in ((4.0, 131072, (32.0, 1.0)), (32.0, 4096, (32.0, 1.0)), (4.0, 32768, (6000.0, 5300.0))):
        kw = dict(dim=128, base=1e6, factor=factor, max_position_embeddings=max_pos, yarn_beta_fast=beta[0], yarn_beta_slow=beta[1])
        want = R.yarn_inv_freq(128, 1e6, factor, max_pos, *beta)
        p = _ffi.RopeParam(type=3, low_freq_factor=1.0, high_freq_factor=4.0, yarn_attention_factor=1.0, **kw)
        assert p.yarn_truncate == 1
        out = np.zeros(64, f32)
        _ffi.check(tm.tm_rope_inv_freq(out.ctypes.data, None, ctypes.byref(p)))
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
        p.yarn_truncate = 0
        _ffi.check(tm.tm_rope_inv_freq(out.ctypes.data, None, ctypes.byref(p)))
        assert not np.array_equal(out.view(np.uint32), want.view(np.uint32))


# ---- 3. reader + loader against transformers ------------------------------------------------------------------------------------------
# Measured on the CPU, 20 random tokens, KV unquantised, max |logit difference| over all 20 rows (|logits| up to 4.2): seeds 0 / 1 / 2
# -> 0.00929 / 0.01454 / 0.00864, the same figures for both on-disk forms (they hold the same numbers).  Bound = twice the largest.
# The mutations land at: gate / up swapped 3.7 .. 4.1, no o_proj bias 1.7 .. 3.2, no q / k / v bias 1.1 .. 1.6, no sinks 4.1 .. 4.3,
# no window 4.2 .. 4.9, no router bias 1.0 .. 3.6.
HF_BOUND = 2 * 0.01454


def _reference_logits(path, ids, mut=None):
    mc, slots = G.load_through_reader(path)
    om = G.GptOssOracleModel(G.oracle_config(mc, 16, 64), G.weights_from_slots(slots, mc), batch=1, max_ctx=64)
    om.forward([ids], mut=mut)
    return om.all_logits.astype(f32), mc, slots


@pytest.mark.parametrize('form', ['save_pretrained', 'published'])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reader_and_loader_against_transformers(form, seed):
    """The toy GptOssForCausalLM (fp32, eager attention) against tests.gpt_oss_reference on the slots that read_config +
    load_hf_weights + export_weights make of the checkpoint -- written by save_pretrained (bf16 experts) and in the published layout
    (MXFP4 blocks / scales, `rope_scaling` + `rope_theta`) -- on 20 tokens with unquantised KV.  The bound is twice the largest
    difference measured over three seeds (HF_BOUND above: 0.00929 / 0.01454 / 0.00864 -> 0.0291); a wrong reader is two orders of
    magnitude away (test_reader_comparison_notices_mutations)."""
    t = G.toy(seed)
    ids = np.random.default_rng(seed).integers(0, G.V, 20)
    got, mc, slots = _reference_logits(t[form], ids)
    d = np.abs(got - G.hf_logits(t['model'], ids)).max()
    print(f'{form} seed {seed}: max |logit diff| {d:.5f} (bound {HF_BOUND:.4f})')
    assert d <= HF_BOUND
    assert mc.moe_expert_format == (3 if form == 'published' else 0)
    assert slots['tok_embeddings.weight'].shape == (G.V, 256) and slots['layers.0.attention.wo.bias'].shape == (256,)
    q = 'layers.1.moe_ffn.experts.3'
    if form == 'published':
        assert slots[q + '.w1w3.blocks'].shape == (768, 128) and slots[q + '.w2.scales'].shape == (256, 12)
    else:
        assert slots[q + '.w1w3.weight'].shape == (256, 768) and slots[q + '.w2.weight'].shape == (384, 256)


@pytest.mark.parametrize('mut', G.MUTATIONS)
def test_reader_comparison_notices_mutations(mut):
    """swapped gate / up, a missing o_proj / qkv / router bias, missing sinks or window: each exceeds the bound by over an order of magnitude"""
    t = G.toy(0)
    ids = np.random.default_rng(0).integers(0, G.V, 20)
    d = np.abs(_reference_logits(t['published'], ids, mut)[0] - G.hf_logits(t['model'], ids)).max()
    print(f'{mut}: max |logit diff| {d:.4f}')
    assert d > 10 * HF_BOUND


def test_both_forms_give_the_same_model():
    """the two checkpoints hold the same numbers: identical non-expert slots, and MXFP4 experts that dequantise to the fp16 experts"""
    t = G.toy(0)
    (mc_a, a), (mc_b, b) = G.load_through_reader(t['save_pretrained']), G.load_through_reader(t['published'])
    assert mc_a.rope == mc_b.rope and mc_a.layer_windows == mc_b.layer_windows == [8, 0]
    for k, v in a.items():
        if 'experts' in k and k.endswith('.weight'):
            stem = k[:-len('.weight')]
            assert np.array_equal(MX.bits(MX.dequant(b[stem + '.blocks'], b[stem + '.scales'])), MX.bits(v)), k
        else:
            assert np.array_equal(v, b[k]), k


# ---- 4. config ------------------------------------------------------------------------------------------------------------------------
PUBLISHED_20B = dict(architectures=['GptOssForCausalLM'], hidden_size=2880, intermediate_size=2880, num_hidden_layers=24,
                     num_attention_heads=64, num_key_value_heads=8, head_dim=64, vocab_size=201088, num_local_experts=32,
                     num_experts_per_tok=4, sliding_window=128, layer_types=['sliding_attention', 'full_attention'] * 12,
                     max_position_embeddings=131072, rms_norm_eps=1e-5, rope_theta=150000, swiglu_limit=7.0, attention_bias=True,
                     rope_scaling=dict(rope_type='yarn', factor=32.0, beta_fast=32.0, beta_slow=1.0, truncate=False,
                                       original_max_position_embeddings=4096),
                     quantization_config=dict(quant_method='mxfp4', modules_to_not_convert=['model.layers.*.self_attn']),
                     eos_token_id=200002)


def _read(tmp_path, c, tp=1):
    with open(os.path.join(tmp_path, 'config.json'), 'w') as f:
        json.dump(c, f)
    return checkpoint.read_config(str(tmp_path), tp)


def test_read_config_of_a_published_gpt_oss(tmp_path):
    m = _read(tmp_path, PUBLISHED_20B)
    assert (m.arch, m.hidden, m.inter, m.layers, m.q_heads, m.kv_heads, m.head_dim, m.vocab) == ('gpt_oss', 2880, 2880, 24, 64, 8, 64, 201088)
    assert (m.attn_bias, m.attn_out_bias, m.attn_sinks, m.qk_norm) == (1, 1, 1, 0)
    assert m.layer_windows == [128, 0] * 12
    assert (m.moe_experts, m.moe_top_k, m.moe_norm_topk, m.moe_act, m.moe_bias, m.moe_expert_format) == (32, 4, True, 1, 1, 3)
    assert (m.weight_format, m.quantized, m.eos_token_id, m.max_position_embeddings) == ('f16', False, 200002, 131072)
    r = m.rope
    assert (r.type, r.dim, r.base, r.factor, r.max_position_embeddings, r.beta_fast, r.beta_slow, r.truncate) \
        == ('yarn', 64, 150000.0, 32.0, 4096, 32.0, 1.0, False)
    assert r.attention_factor == pytest.approx(0.1 * np.log(32.0) + 1.0, rel=1e-12)
    e = make_model_config(m, 1)
    assert (e.hidden, e.inter, e.hidden_valid, e.attn_out_bias, e.attn_sinks, e.attn_bias, e.rope_yarn_truncate) == (2944, 2944, 2880, 1, 1, 1, 0)
    assert (e.moe_expert_format, e.moe_act, e.moe_bias, e.rope_type, e.rope_max_position_embeddings) == (3, 1, 1, 3, 4096)
    # the same settings in the transformers-5 spelling, and the unquantised form
    c = {k: v for k, v in PUBLISHED_20B.items() if k not in ('rope_scaling', 'rope_theta', 'quantization_config')}
    c.update(rope_parameters=dict(PUBLISHED_20B['rope_scaling'], rope_theta=150000.0), dtype='bfloat16')
    u = _read(tmp_path, c)
    assert u.rope == r and u.moe_expert_format == 0 and u.layer_windows == m.layer_windows


@pytest.mark.parametrize('change,exc,words', [
    (dict(swiglu_limit=5.0), NotImplementedError, ('swiglu_limit 5.0', 'clamps at 7')),
    (dict(quantization_config=dict(quant_method='awq', bits=4)), NotImplementedError, ('awq', 'mxfp4')),
    (dict(quantization_config=None, torch_dtype='float32'), NotImplementedError, ('float32', 'float16 / bfloat16')),
    (dict(layer_types=None), NotImplementedError, ('lacks layer_types', 'o_proj bias')),
    (dict(sliding_window=None, rope_scaling=None), NotImplementedError, ('sliding_window', 'rope_scaling + rope_theta', '% 128')),
    (dict(layer_types=['sliding_attention'] * 23 + ['chunked_attention']), NotImplementedError, ('layer_types',)),
    (dict(sliding_window=-4), ValueError, ('sliding_window',)),
    (dict(rope_scaling=dict(rope_type='longrope', factor=2.0)), NotImplementedError, ('rope type longrope',)),
    (dict(head_dim=96), NotImplementedError, ('head_dim 96',)),
])
def test_read_config_refusals_name_their_reason(tmp_path, change, exc, words):
    c = {k: v for k, v in dict(PUBLISHED_20B, **change).items() if v is not None}
    with pytest.raises(exc) as ei:
        _read(tmp_path, c)
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_read_config_refuses_tp(tmp_path):
    with pytest.raises(NotImplementedError, match='tp = 2'):
        _read(tmp_path, PUBLISHED_20B, tp=2)


def test_synthetic_gpt_oss_20b_entry():
    """the timing entry is the published 20b geometry"""
    from lmdeploy_amd.pipeline import SYNTHETIC
    s = SYNTHETIC['gpt_oss_20b']
    m = checkpoint.ModelConfig(**s)
    assert (m.hidden, m.inter, m.layers, m.q_heads, m.kv_heads, m.head_dim, m.vocab) == (2880, 2880, 24, 64, 8, 64, 201088)
    assert (m.moe_experts, m.moe_top_k, m.moe_expert_format, m.moe_act, m.moe_bias) == (32, 4, 3, 1, 1)
    assert m.layer_windows == [128, 0] * 12 and (m.attn_bias, m.attn_out_bias, m.attn_sinks) == (1, 1, 1)
    assert (m.rope.type, m.rope.truncate, m.rope.max_position_embeddings) == ('yarn', False, 4096)
