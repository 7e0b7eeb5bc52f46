"""The LoRA reader and operand layout on the CPU: a hand-written PEFT adapter directory (no `peft` here) read back through
checkpoint.read_lora, the folding of lora_alpha / r and rslora, the q | k | v stacking, every reader refusal by name, the new symbols."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.loader import permute_qk_for_interleaved_rope

CFG = checkpoint.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=64, inter=512, vocab=1024, quantized=False, weight_format='f16')
R, ALPHA = 8, 32.0


def _write(path, targets=('q_proj', 'v_proj', 'o_proj', 'down_proj'), **over):
    rng, tensors = np.random.default_rng(0), {}
    shapes = dict(q_proj=('self_attn', 256, 256), k_proj=('self_attn', 256, 128), v_proj=('self_attn', 256, 128), o_proj=('self_attn', 256, 256),
                  down_proj=('mlp', 512, 256), gate_proj=('mlp', 256, 512))
    for i in range(CFG.layers):
        for t in targets:
            mod, K, N = shapes.get(t, ('mlp', 256, 256))
            key = f'base_model.model.model.layers.{i}.{mod}.{t}'
            tensors[key + '.lora_A.weight'] = torch.from_numpy(rng.standard_normal((R, K)).astype(np.float32))
            tensors[key + '.lora_B.weight'] = torch.from_numpy(rng.standard_normal((N, R)).astype(np.float32))
    save_file(tensors, str(path / 'adapter_model.safetensors'))
    cfg = dict(peft_type='LORA', r=R, lora_alpha=ALPHA, target_modules=list(targets), bias='none', use_rslora=False)
    cfg.update(over)
    (path / 'adapter_config.json').write_text(json.dumps(cfg))
    return {k: v.numpy() for k, v in tensors.items()}


@pytest.mark.parametrize('rslora', [False, True])
def test_read_lora_round_trip(tmp_path, rslora):
    raw = _write(tmp_path, use_rslora=rslora)
    layers = checkpoint.read_lora(str(tmp_path), CFG)
    scale = ALPHA / np.sqrt(R) if rslora else ALPHA / R
    assert checkpoint.lora_scale(R, ALPHA, rslora) == pytest.approx(scale)
    for i, L in enumerate(layers):
        assert sorted(L) == ['qkv', 'w2', 'wo']
        p = f'base_model.model.model.layers.{i}.'
        A, B, ranks = L['qkv']
        assert ranks == [16, 0, 16] and A.shape == (32, 256) and B.shape == (512, 16)      # q | (no k) | v, ranks padded to 16
        assert np.array_equal(A[:R], raw[p + 'self_attn.q_proj.lora_A.weight'].astype(np.float16)) and not A[R:16].any()
        assert np.array_equal(A[16:16 + R], raw[p + 'self_attn.v_proj.lora_A.weight'].astype(np.float16))
        bq = permute_qk_for_interleaved_rope(raw[p + 'self_attn.q_proj.lora_B.weight'].T, 4, 64).T * np.float32(scale)
        assert np.array_equal(B[:256, :R], bq.astype(np.float16)) and not B[256:384].any() and not B[:, R:].any()
        assert np.array_equal(B[384:, :R], (raw[p + 'self_attn.v_proj.lora_B.weight'] * np.float32(scale)).astype(np.float16))
        assert L['w2'][2] == [16] and np.array_equal(L['w2'][1][:, :R], (raw[p + 'mlp.down_proj.lora_B.weight'] * np.float32(scale)).astype(np.float16))


def test_read_lora_internlm2_wqkv(tmp_path):
    """the fused wqkv ([q_0, q_1, k, v] per kv group): B's rows split like the base weight's columns, one A for the three segments"""
    rng, t = np.random.default_rng(1), {}
    for i in range(CFG.layers):
        t[f'base_model.model.model.layers.{i}.attention.wqkv.lora_A.weight'] = torch.from_numpy(rng.standard_normal((R, 256)).astype(np.float32))
        t[f'base_model.model.model.layers.{i}.attention.wqkv.lora_B.weight'] = torch.from_numpy(rng.standard_normal((512, R)).astype(np.float32))
    save_file(t, str(tmp_path / 'adapter_model.safetensors'))
    (tmp_path / 'adapter_config.json').write_text(json.dumps(dict(r=R, lora_alpha=R, target_modules=['wqkv'], bias='none')))
    A, B, ranks = checkpoint.read_lora(str(tmp_path), CFG)[1]['qkv']
    a, b = (t[f'base_model.model.model.layers.1.attention.wqkv.lora_{n}.weight'].numpy() for n in 'AB')
    bg = b.reshape(2, 4, 64, R)                                      # [kv group][q, q, k, v][head_dim][r]
    assert ranks == [16, 16, 16] and all(np.array_equal(A[o:o + R], a.astype(np.float16)) for o in (0, 16, 32))
    assert np.array_equal(B[:256, :R], permute_qk_for_interleaved_rope(bg[:, :2].reshape(256, R).T, 4, 64).T.astype(np.float16))
    assert np.array_equal(B[256:384, :R], permute_qk_for_interleaved_rope(bg[:, 2].reshape(128, R).T, 2, 64).T.astype(np.float16))
    assert np.array_equal(B[384:, :R], bg[:, 3].reshape(128, R).astype(np.float16))


@pytest.mark.parametrize('over,targets,msg', [
    (dict(use_dora=True), None, 'use_dora'), (dict(bias='all'), None, "bias != 'none'"), (dict(modules_to_save=['lm_head']), None, 'modules_to_save'),
    (dict(rank_pattern={'q_proj': 4}), None, 'rank_pattern'), (dict(alpha_pattern={'q_proj': 4}), None, 'alpha_pattern'),
    ({}, ('q_proj', 'gate_proj'), 'gate_proj / up_proj'), ({}, ('q_proj', 'embed_tokens'), 'embed_tokens is outside q_proj')])
def test_read_lora_refusals(tmp_path, over, targets, msg):
    _write(tmp_path, **({'targets': targets} if targets else {}), **over)
    with pytest.raises(NotImplementedError, match=msg):
        checkpoint.read_lora(str(tmp_path), CFG)


def test_operand_and_model_refusals():
    with pytest.raises(NotImplementedError, match='rank over 64 per segment'):
        checkpoint.lora_operands([(np.zeros((80, 256)), np.zeros((256, 80)))], [256], 1.0)
    moe = checkpoint.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=64, inter=512, vocab=1024, moe_experts=8, moe_top_k=2)
    for args, msg in (((moe, 8, 1), 'mixture-of-experts'), ((CFG, 8, 2), 'tp > 1'), ((CFG, 42, 1), 'quant_policy=42')):
        with pytest.raises(NotImplementedError, match=msg):
            checkpoint.check_lora(*args)


def test_ffi_declares_the_lora_symbols():
    sig = _ffi._SIGNATURES
    assert sig['tm_lora_plan_workspace'] == (C.c_size_t, [C.c_int]) and len(sig['tm_lora_table_create'][1]) == 7
    assert sig['tm_lora_apply'][1] == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert len(sig['tm_engine_load_adapter'][1]) == 8 and len(sig['tm_engine_set_adapters'][1]) == 3
    assert {'tm_lora_table_set', 'tm_lora_table_destroy', 'tm_lora_plan'} <= set(sig)
