"""YaRN and dynamic-NTK RoPE on the host: the table builder (tm_rope_table_ex) bit for bit against the numpy restatement, the
per-sequence base (tm_rope_dynamic_base) against the float64 formula, the config reader and the struct plumbing.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.engine import make_model_config
from oracle import tm_oracle as o
from tests import rope_scaling_reference as R

f16, f32 = np.float16, np.float32


@pytest.fixture(scope='module')
def tm():
    return _ffi.load()


def table_ex(tm, max_pos, **kw):
    p = _ffi.RopeParam(dim=128, base=10000.0, type=0, factor=1.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position=8192,
                       max_position_embeddings=0, yarn_beta_fast=32.0, yarn_beta_slow=1.0, yarn_attention_factor=1.0)
    for k, v in kw.items():
        setattr(p, k, v)
    tab = np.zeros((max_pos, p.dim // 2, 2), f16)
    _ffi.check(tm.tm_rope_table_ex(tab.ctypes.data, max_pos, ctypes.byref(p)))
    return tab


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# positions that matter: the first rows, a block boundary, and rows far out where the fp32 angle is large
POS = np.r_[0:130, 4095:4100, 32766:32770]


@pytest.mark.parametrize('factor,max_pos,beta,af', [
    (4.0, 131072, (32.0, 1.0), None),          # Qwen-style: factor 4 over an original 32768, theta 1e6
    (1.0, 32768, (32.0, 1.0), None),           # factor 1: attention_factor 1, inv_freq = freq
    (4.0, 32768, (6000.0, 5300.0), 1.25),      # both correction dimensions clamp to 0: the low == high (+0.001) branch
])
def test_yarn_table_bits(tm, factor, max_pos, beta, af):
    af = R.yarn_attention_factor(dict(factor=factor)) if af is None else af
    n = int(POS.max()) + 1
    got = table_ex(tm, n, type=3, base=1e6, factor=factor, max_position_embeddings=max_pos, yarn_beta_fast=beta[0],
                   yarn_beta_slow=beta[1], yarn_attention_factor=af)[POS]
    inv = R.yarn_inv_freq(128, 1e6, factor, max_pos, *beta)
    c, s = R.table(inv, POS, af)
    assert np.array_equal(bits(got[..., 0]), bits(c)) and np.array_equal(bits(got[..., 1]), bits(s))
    low, high = R.yarn_correction_range(128, 1e6, max_pos, *beta)
    if beta[0] == 6000.0:
        assert low == 0 and high == f32(0.001)
    if factor == 1.0:
        assert af == 1.0
        assert np.array_equal(bits(got), bits(table_ex(tm, n, type=0, base=1e6)[POS])), 'yarn with factor 1 is the default table'
    else:
        assert not np.array_equal(bits(got), bits(table_ex(tm, n, type=0, base=1e6)[POS]))


@pytest.mark.parametrize('base', [1e6, 1527385.25, 10000.0])
def test_dynamic_table_is_the_default_table_of_its_base(tm, base):
    """type 4 ignores factor / max_position_embeddings: the caller passes the sequence's base"""
    n = int(POS.max()) + 1
    dyn = table_ex(tm, n, type=4, base=base, factor=3.0, max_position_embeddings=64)[POS]
    assert np.array_equal(bits(dyn), bits(table_ex(tm, n, type=0, base=base)[POS]))
    c, s = R.table(R.default_freq(128, base), POS)
    assert np.array_equal(bits(dyn[..., 0]), bits(c)) and np.array_equal(bits(dyn[..., 1]), bits(s))
    c0, s0 = o.rope_cos_sin(o.RopeParam(128, float(f32(base))), POS)
    assert np.array_equal(bits(c), bits(c0)) and np.array_equal(bits(s), bits(s0)), 'restatement == oracle on the default recipe'


def test_rope_table_keeps_its_contract(tm):
    """tm_rope_table: types 0..2 as before (same bits as the _ex entry point), 3 / 4 refused"""
    tab = np.zeros((40, 64, 2), f16)
    for t, kw in ((0, {}), (1, dict(factor=2.0)), (2, dict(factor=8.0, original_max_position=8192, base=500000.0))):
        base = kw.get('base', 10000.0)
        _ffi.check(tm.tm_rope_table(tab.ctypes.data, 40, 128, base, t, kw.get('factor', 1.0), 1.0, 4.0, 8192))
        assert np.array_equal(bits(tab), bits(table_ex(tm, 40, type=t, **kw)))
    assert tm.tm_rope_table(tab.ctypes.data, 40, 128, 1e4, 3, 4.0, 1.0, 4.0, 8192) != 0
    assert tm.tm_rope_table(tab.ctypes.data, 40, 128, 1e4, 4, 2.0, 1.0, 4.0, 8192) != 0


@pytest.mark.parametrize('base,factor,dim,max_pos,n', [(1e6, 2.0, 128, 32768, 40000), (1e4, 3.0, 128, 64, 65), (1e4, 3.0, 128, 64, 150),
                                                        (1e4, 3.0, 128, 64, 4096)])
def test_dynamic_base(tm, base, factor, dim, max_pos, n):
    got = f32(tm.tm_rope_dynamic_base(base, factor, dim, max_pos, n))
    ref = R.dynamic_base(base, factor, dim, max_pos, n)
    assert got > base
    assert abs(float(got) - ref) <= 4 * float(np.spacing(f32(ref))), (got, ref)
    for m in (max_pos, max_pos - 1, 1):             # prompt_len <= max_pos: the model's base
        assert f32(tm.tm_rope_dynamic_base(base, factor, dim, max_pos, m)) == f32(base)
    for f in (1.0, 0.5, 0.0):                       # factor <= 1: never
        assert f32(tm.tm_rope_dynamic_base(base, f, dim, max_pos, n)) == f32(base)


# ---- config reader ----------------------------------------------------------------------------------------------------
def write_config(path, arch, **kw):
    c = dict(architectures=[arch], hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=1024,
             num_hidden_layers=2, vocab_size=1000, rms_norm_eps=1e-5, rope_theta=1000000.0, max_position_embeddings=32768)
    c.update(kw)
    with open(os.path.join(str(path), 'config.json'), 'w') as f:
        json.dump(c, f)
    return checkpoint.read_config(str(path))


@pytest.mark.parametrize('key', ['type', 'rope_type'])
def test_read_config_internlm2_dynamic(tmp_path, key):
    mc = write_config(tmp_path, 'InternLM2ForCausalLM', rope_scaling={key: 'dynamic', 'factor': 2.0})
    assert mc.arch == 'internlm2'
    r = mc.rope
    assert (r.type, r.factor, r.max_position_embeddings, r.base, r.dim) == ('dynamic', 2.0, 32768, 1e6, 128)


def test_read_config_llama_yarn(tmp_path):
    # without original_max_position_embeddings: the factor as written
    r = write_config(tmp_path, 'LlamaForCausalLM', rope_scaling=dict(rope_type='yarn', factor=4.0)).rope
    assert (r.type, r.factor, r.max_position_embeddings, r.beta_fast, r.beta_slow) == ('yarn', 4.0, 32768, 32.0, 1.0)
    assert r.attention_factor == pytest.approx(0.1 * np.log(4.0) + 1.0, rel=1e-12)
    # with it: factor = max_position_embeddings / original; attention_factor still from the factor as written; the engine gets the
    # MODEL's max_position_embeddings (the reference's copy_rope_config)
    r = write_config(tmp_path, 'LlamaForCausalLM', max_position_embeddings=131072,
                     rope_scaling=dict(type='yarn', factor=3.0, original_max_position_embeddings=32768, beta_fast=16, beta_slow=2)).rope
    assert (r.factor, r.max_position_embeddings, r.beta_fast, r.beta_slow) == (4.0, 131072, 16.0, 2.0)
    assert r.attention_factor == pytest.approx(0.1 * np.log(3.0) + 1.0, rel=1e-12)
    # mscale / mscale_all_dim
    rs = dict(type='yarn', factor=40.0, mscale=1.0, mscale_all_dim=0.707)
    r = write_config(tmp_path, 'LlamaForCausalLM', rope_scaling=rs).rope
    assert r.attention_factor == pytest.approx((0.1 * np.log(40.0) + 1.0) / (0.1 * 0.707 * np.log(40.0) + 1.0), rel=1e-12)
    assert r.attention_factor == pytest.approx(R.yarn_attention_factor(rs), rel=1e-12)
    # an explicit attention_factor wins
    assert write_config(tmp_path, 'LlamaForCausalLM', rope_scaling=dict(type='yarn', factor=4.0, attention_factor=1.5)).rope.attention_factor == 1.5


def test_read_config_internlm3(tmp_path):
    mc = write_config(tmp_path, 'InternLM3ForCausalLM', head_dim=128, rope_scaling=dict(rope_type='dynamic', factor=6.0), bias=False,
                      qkv_bias=False)
    assert (mc.arch, mc.rope.type, mc.rope.factor, mc.attn_bias) == ('llama', 'dynamic', 6.0, 0)
    for k in ('qkv_bias', 'bias'):
        with pytest.raises(NotImplementedError, match=k):
            write_config(tmp_path, 'InternLM3ForCausalLM', head_dim=128, **{k: True})


def test_read_config_qwen_still_refuses(tmp_path):
    for t in ('yarn', 'dynamic'):
        with pytest.raises(NotImplementedError, match=t):
            write_config(tmp_path, 'Qwen2ForCausalLM', rope_scaling=dict(type=t, factor=4.0))


# ---- struct plumbing ----------------------------------------------------------------------------------------------------
def test_make_model_config_new_fields():
    cfg = o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024,
                        rope=o.RopeParam(128, 500000.0, 'llama3', 8.0, 1.0, 4.0, 8192))
    assert not hasattr(cfg.rope, 'beta_fast')
    m = make_model_config(cfg)                  # an oracle RopeParam without the new attributes still converts
    assert (m.rope_type, m.rope_max_position_embeddings, m.rope_yarn_beta_fast, m.rope_yarn_beta_slow, m.rope_yarn_attention_factor) \
        == (2, 0, 32.0, 1.0, 1.0)
    assert (m.group_size, m.weight_type, m.attn_bias, m.qk_norm) == (128, 0, 0, 0)
    r = checkpoint.RopeConfig(128, 1e6, 'yarn', 4.0, max_position_embeddings=131072, beta_fast=16.0, beta_slow=2.0, attention_factor=1.25)
    m = make_model_config(checkpoint.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, rope=r))
    raw = np.frombuffer(bytes(m), np.int32)
    # directly behind rope_original_max_position (field 13), in front of group_size
    assert _ffi.ModelConfig.rope_original_max_position.offset == 13 * 4
    assert raw[9] == 3 and raw[14] == 131072 and raw[18] == 128
    assert np.array_equal(raw[15:18].view(f32), np.array([16.0, 2.0, 1.25], f32))
    assert [f[0] for f in _ffi.ModelConfig._fields_][14:18] == ['rope_max_position_embeddings', 'rope_yarn_beta_fast',
                                                               'rope_yarn_beta_slow', 'rope_yarn_attention_factor']
    d = checkpoint.RopeConfig(128, 1e6, 'dynamic', 2.0, max_position_embeddings=32768)
    m = make_model_config(checkpoint.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, rope=d))
    assert (m.rope_type, m.rope_factor, m.rope_max_position_embeddings) == (4, 2.0, 32768)


def test_rope_param_struct_matches_header():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tm_mi355x.h')).read()
    body = re.search(r'typedef struct tm_rope_param \{(.*?)\} tm_rope_param;', hdr, re.S).group(1)
    names = [n.strip() for decl in body.split(';') if decl.strip() for n in decl.split(None, 1)[1].split(',')]
    assert [f[0] for f in _ffi.RopeParam._fields_] == names and ctypes.sizeof(_ffi.RopeParam) == 4 * len(names)
