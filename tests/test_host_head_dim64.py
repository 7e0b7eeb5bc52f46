"""head_dim 64 on the host side: the Llama reader accepts Llama-3.2-1B-style configs (head_dim 64 derived from hidden_size /
num_attention_heads) and refuses, by name, what the native side has no kernels for; make_model_config carries head_dim 64 into the
native struct; tm_engine_create refuses other head dims and q/k RMSNorm at head_dim 64 before it touches a device."""
import json
import os

import pytest

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.engine import make_model_config


def _llama32_1b(**over):
    """config.json of Llama-3.2-1B as published (no head_dim key: 2048 / 32 = 64)"""
    c = {'architectures': ['LlamaForCausalLM'], 'hidden_size': 2048, 'num_hidden_layers': 16, 'num_attention_heads': 32,
         'num_key_value_heads': 8, 'intermediate_size': 8192, 'vocab_size': 128256, 'rms_norm_eps': 1e-5, 'rope_theta': 500000.0,
         'max_position_embeddings': 131072, 'tie_word_embeddings': True, 'eos_token_id': 128001, 'torch_dtype': 'bfloat16',
         'rope_scaling': {'rope_type': 'llama3', 'factor': 32.0, 'low_freq_factor': 1.0, 'high_freq_factor': 4.0,
                          'original_max_position_embeddings': 8192}}
    c.update(over)
    return c


def _write(tmp_path, c):
    with open(os.path.join(str(tmp_path), 'config.json'), 'w') as f:
        json.dump(c, f)
    return str(tmp_path)


def test_read_config_llama32_1b(tmp_path):
    mc = checkpoint.read_config(_write(tmp_path, _llama32_1b()))
    assert (mc.head_dim, mc.q_heads, mc.kv_heads, mc.hidden) == (64, 32, 8, 2048)
    assert (mc.rope.dim, mc.rope.type, mc.rope.factor) == (64, 'llama3', 32.0)
    assert mc.tie_word_embeddings and mc.arch == 'llama' and mc.weight_format == 'f16' and not mc.quantized
    c = make_model_config(mc, 1)
    assert (c.head_dim, c.q_heads, c.kv_heads, c.rope_type, c.rope_factor) == (64, 32, 8, 2, 32.0)    # the rope dim is head_dim


def test_read_config_head_dim64_awq_and_explicit_key(tmp_path):
    q = {'quant_method': 'awq', 'bits': 4, 'group_size': 128, 'zero_point': True, 'version': 'gemm'}
    mc = checkpoint.read_config(_write(tmp_path, _llama32_1b(quantization_config=q, head_dim=64)))
    assert mc.head_dim == 64 and mc.weight_format == 'u4' and mc.quantized
    # TinyLlama-1.1B: 32 heads of 64 under 4 kv heads, no rope scaling
    mc = checkpoint.read_config(_write(tmp_path, _llama32_1b(num_key_value_heads=4, num_hidden_layers=22, intermediate_size=5632,
                                                             vocab_size=32000, rope_scaling=None, tie_word_embeddings=False)))
    assert (mc.head_dim, mc.kv_heads, mc.rope.dim, mc.rope.type) == (64, 4, 64, 'default')


@pytest.mark.parametrize('label,over,needles', [
    ('head_dim 96', dict(hidden_size=3072, num_attention_heads=32), ('head_dim 96', '64 and 128')),
    ('head_dim 256', dict(head_dim=256), ('head_dim 256', '64 and 128')),
    ('9 heads x 64', dict(hidden_size=576, num_attention_heads=9, num_key_value_heads=3), ('9 attention heads', 'multiple of 128')),
    ('fp8 + head_dim 64', dict(quantization_config={'quant_method': 'fp8', 'weight_block_size': [128, 128]}), ('fp8', 'head_dim 64')),
])
def test_read_config_head_dim_refusals(tmp_path, label, over, needles):
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(_write(tmp_path, _llama32_1b(**over)))
    for n in needles:
        assert n in str(ei.value), (label, str(ei.value))


def test_read_config_fp8_head_dim128_still_loads(tmp_path):
    mc = checkpoint.read_config(_write(tmp_path, _llama32_1b(
        hidden_size=4096, quantization_config={'quant_method': 'fp8', 'weight_block_size': [128, 128]})))
    assert mc.head_dim == 128 and mc.weight_format == 'fp8'


def _create(head_dim, qk_norm=0, q_heads=4):
    lib = _ffi.load()
    mc = _ffi.ModelConfig(hidden=256, layers=1, q_heads=q_heads, kv_heads=1, head_dim=head_dim, inter=512, vocab=1024, rms_eps=1e-5,
                          group_size=128, weight_type=0, qk_norm=qk_norm)
    cfg = _ffi.EngineConfig(model=mc, tp=1, rank=0, device=-1, max_batch_size=4, session_len=128, quant_policy=8, cache_block_seq_len=64)
    e = _ffi.C.c_void_p()
    rc = lib.tm_engine_create(_ffi.C.byref(e), _ffi.C.byref(cfg))
    assert not e.value
    return rc, _ffi.last_error()


def test_engine_create_refuses_before_touching_a_device():
    rc, msg = _create(96)
    assert rc == 1 and 'head_dim' in msg and '64 or 128' in msg
    rc, msg = _create(64, qk_norm=1)
    assert rc == 1 and 'head_dim' in msg and 'qk_norm' in msg
