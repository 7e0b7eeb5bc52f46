"""What a decode step launches, per profiling category, for every shape of layer the engine's forward builds: the span counts of
Engine.profile_decode(1) after a prefill, against constants.  The counts are host-side integers (one span per TM_PROF site that ran),
so they are compared exactly.  They pin the forward's launch plan: a change to engine_forward.hip that adds, drops or re-labels a
launch in one of these layer forms shows here, whatever the logits do.

Tiny synthetic models (2 layers, H 256, head_dim 128), batch 3, prompts of 40, 5 and 17 tokens.  The constants were recorded at commit
c322eb2, the last one before the forward's layer blocks were factored out of forward(), by running this module's engines there."""
import numpy as np
import pytest

from lmdeploy_amd.turbomind.engine import Engine
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o

pytestmark = pytest.mark.gpu

PROMPT_LENS = (40, 5, 17)


def tiny_cfg(kv_bits):
    return o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024, kv_bits=kv_bits,
                         rope=o.RopeParam(128, 10000.0))


def _dense(kv_bits):
    cfg = tiny_cfg(kv_bits)
    return cfg, export_weights(cfg, o.make_synthetic_weights(cfg, seed=3)), 0


def _moe(tmp_path):
    from tests.qwen_moe_reference import QWEN3_MOE_CFG, QwenMoeConfig, make_qwen_moe_weights
    cfg = QwenMoeConfig(**dict(QWEN3_MOE_CFG, moe_experts=8, moe_top_k=2), kv_bits=8)
    return cfg, export_weights(cfg, make_qwen_moe_weights(cfg, seed=3)), 0


def _moe_shared(tmp_path):
    from tests.qwen2_moe_reference import QWEN2_MOE_CFG, Qwen2MoeConfig, make_qwen2_moe_weights
    cfg = Qwen2MoeConfig(**dict(QWEN2_MOE_CFG, moe_experts=8, moe_top_k=2, moe_shared_inter=128), kv_bits=8)
    return cfg, export_weights(cfg, make_qwen2_moe_weights(cfg, seed=3)), 0


def _fp8_channel(tmp_path):
    from lmdeploy_amd.turbomind import checkpoint
    from tests import fp8_channel_reference as r
    path = str(tmp_path / 'fp8_channel')
    r.write_checkpoint(path, seed=11, q_heads=4, kv_heads=2, vocab=1024, dialect='compressed-tensors', strategy='channel')
    cfg = checkpoint.read_config(path)
    assert cfg.fp8_scale_mode == 1
    return cfg, export_weights(cfg, checkpoint.load_hf_weights(path, cfg)), 2


# name -> (model builder, quant_policy, environment switches)
ENGINES = {
    'fused': (lambda tmp: _dense(8), 8, {}),
    'unfused': (lambda tmp: _dense(8), 8, {'TM_FUSE_QKV': '0'}),
    'fp16_kv': (lambda tmp: _dense(16), 0, {}),
    'fold3': (lambda tmp: _dense(8), 8, {'TM_FOLD_NORM': '3'}),
    'moe': (_moe, 8, {}),
    'moe_shared': (_moe_shared, 8, {}),
    'fp8_channel': (_fp8_channel, 8, {}),
}

# categories with a count of 0 are left out; recorded at commit c322eb2
_DENSE = dict(embed=1, gemm_qkv=2, attention=2, gemm_o=2, residual_norm=5, gemm_gate_up=2, gemm_down=2, lm_head=1, sample=1, allreduce=4)
SPANS = {
    'fused': _DENSE,                                        # no kv_store span: the attention's prologue stores K / V
    'unfused': dict(_DENSE, kv_store=2),
    'fp16_kv': dict(_DENSE, kv_store=2),
    'fold3': dict(_DENSE, residual_norm=2, allreduce=1),   # the first norm and the last layer's w2 -> final norm
    'moe': {k: n for k, n in _DENSE.items() if k != 'gemm_down'},      # router + experts + combine: one gemm_gate_up span a layer
    'moe_shared': dict(_DENSE, gemm_gate_up=4),             # the shared expert's w1w3 / w2 in front of it
    'fp8_channel': _DENSE,
}


def started_engine(name, tmp_path, monkeypatch, max_new_tokens=5):
    """the engine `name` of ENGINES behind its prefill -> (engine, prompts)"""
    build, quant_policy, env = ENGINES[name]
    for k in ('TM_FUSE_QKV', 'TM_FOLD_NORM', 'TM_FOLD_MAX_M', 'TM_ATTN_VALU', 'TM_GEMM_TUNE'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, slots, weight_type = build(tmp_path)
    rng = np.random.default_rng(1)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in PROMPT_LENS]
    eng = Engine.from_model_config(cfg, weight_type=weight_type, max_batch_size=3, session_len=64, quant_policy=quant_policy,
                                   max_prefill_token_num=96)
    eng.load_weights(slots)
    eng.start()
    eng.prefill(prompts, max_new_tokens=max_new_tokens)
    return eng, prompts


def span_counts(eng):
    return {k: n for k, (_, n) in eng.profile_decode(1).items() if n}


@pytest.mark.parametrize('name', list(ENGINES))
def test_decode_step_span_counts(cuda, tmp_path, monkeypatch, name):
    eng, _ = started_engine(name, tmp_path, monkeypatch)
    try:
        got = span_counts(eng)
    finally:
        eng.close()
    print(f'{name}: {got}')
    assert set(got) <= set(Engine.PROF_CATEGORIES)
    assert got == SPANS[name], f'{name}: a decode step launches {got}, the recorded plan is {SPANS[name]}'
