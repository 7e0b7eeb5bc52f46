"""Qwen3-MoE on the host side: config reading and its refusals, reading a fabricated AWQ / block-FP8 checkpoint (router, expert
fusion, q / k norm), the engine slots and the tensor-parallel rule of the expert width."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd.turbomind import checkpoint, loader
from lmdeploy_amd.turbomind.engine import make_model_config
from oracle import tm_oracle as o
from tests.qwen_moe_reference import hf_qwen_moe_tensors, qwen_moe_config_json, write_qwen_moe_checkpoint

f16 = np.float16
AWQ = {'quant_method': 'awq', 'bits': 4, 'group_size': 128}


def _a3b(**extra):
    """config.json of Qwen3-30B-A3B (AWQ)"""
    c = qwen_moe_config_json(2048, 32, 4, 768, 128, 8, 151936, 48, 'awq')
    c.update(extra)
    return c


def _write(path, c):
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)


@pytest.mark.parametrize('norm_topk', [True, False])
@pytest.mark.parametrize('attention_bias', [True, False])
def test_read_config_qwen3_moe(tmp_path, norm_topk, attention_bias):
    _write(tmp_path, _a3b(norm_topk_prob=norm_topk, attention_bias=attention_bias))
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.arch, mc.qk_norm, mc.attn_bias, mc.head_dim) == ('qwen3', 1, int(attention_bias), 128)
    assert (mc.hidden, mc.inter, mc.moe_experts, mc.moe_top_k, mc.moe_norm_topk, mc.moe_routed_scale) == \
        (2048, 768, 128, 8, norm_topk, 1.0)
    assert (mc.quantized, mc.weight_format, mc.q_heads, mc.kv_heads, mc.layers) == (True, 'u4', 32, 4, 48)
    mcfg = make_model_config(mc)
    assert (mcfg.moe_experts, mcfg.moe_top_k, mcfg.moe_norm_topk, mcfg.inter, mcfg.attn_bias, mcfg.qk_norm) == \
        (128, 8, int(norm_topk), 768, int(attention_bias), 1)


def test_read_config_qwen3_moe_fp8(tmp_path):
    c = _a3b(hidden_size=4096, num_attention_heads=64, moe_intermediate_size=1536, num_hidden_layers=94)       # 235B-A22B
    c['quantization_config'] = {'quant_method': 'fp8', 'weight_block_size': [128, 128]}
    _write(tmp_path, c)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.weight_format, mc.hidden, mc.inter, mc.moe_experts, mc.moe_top_k) == ('fp8', 4096, 1536, 128, 8)


def _without(c, *keys):
    return {k: v for k, v in c.items() if k not in keys}


@pytest.mark.parametrize('label,cfg,needle', [
    ('no num_experts', _without(_a3b(), 'num_experts'), 'num_experts'),
    ('no num_experts_per_tok', _without(_a3b(), 'num_experts_per_tok'), 'num_experts_per_tok'),
    ('no moe_intermediate_size', _without(_a3b(), 'moe_intermediate_size'), 'moe_intermediate_size'),
    ('mlp_only_layers', _a3b(mlp_only_layers=[0, 3]), 'mlp_only_layers'),
    ('decoder_sparse_step', _a3b(decoder_sparse_step=2), 'decoder_sparse_step'),
    ('num_experts 512', _a3b(num_experts=512), '256'),
    ('top 10', _a3b(num_experts_per_tok=10), 'top-8'),
    ('head_dim 64', _a3b(head_dim=64), 'head_dim'),
    ('sliding window', _a3b(use_sliding_window=True), 'sliding'),
    ('yarn', _a3b(rope_scaling={'rope_type': 'yarn', 'factor': 4.0, 'original_max_position_embeddings': 32768}), 'yarn'),
    ('dynamic rope', _a3b(rope_scaling={'type': 'dynamic', 'factor': 2.0}), 'dynamic'),
    ('bf16 experts', _without(_a3b(), 'quantization_config'), 'experts'),
    ('Qwen2-MoE', dict(_a3b(), architectures=['Qwen2MoeForCausalLM']), 'Qwen2MoeForCausalLM'),
])
def test_read_config_qwen3_moe_refusals(tmp_path, label, cfg, needle):
    _write(tmp_path, cfg)
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert needle in str(ei.value), f'{label}: the message does not name the reason: {ei.value}'


def test_read_config_missing_keys_are_all_named(tmp_path):
    _write(tmp_path, _without(_a3b(), 'num_experts', 'moe_intermediate_size'))
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert 'num_experts' in str(ei.value) and 'moe_intermediate_size' in str(ei.value) and 'num_experts_per_tok' not in str(ei.value)


H, HQ, HKV, I, E, K, V, LAYERS = 256, 4, 2, 128, 72, 8, 96, 2


@pytest.mark.parametrize('fmt', ['awq', 'fp8'])
def test_load_qwen3_moe_checkpoint(tmp_path, fmt):
    """2 layers, H 256, 72 experts (above the serial router's cap, not a power of two), top-8, expert width 128"""
    rng = np.random.default_rng(2)
    hf = hf_qwen_moe_tensors(rng, H, HQ, HKV, I, E, V, LAYERS)
    quant = write_qwen_moe_checkpoint(str(tmp_path), hf, H, HQ, HKV, I, E, K, V, LAYERS, fmt)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.arch, mc.qk_norm, mc.attn_bias, mc.moe_experts, mc.moe_top_k, mc.inter) == ('qwen3', 1, 0, E, K, I)
    assert mc.weight_format == ('u4' if fmt == 'awq' else 'fp8')
    w = checkpoint.load_hf_weights(str(tmp_path), mc)
    assert len(w['layers']) == LAYERS
    for li, L in enumerate(w['layers']):
        p = f'model.layers.{li}'
        # router: unquantised, transposed to [H][E], fp16
        assert L['moe_gate'].dtype == f16 and L['moe_gate'].shape == (H, E)
        assert np.array_equal(L['moe_gate'], hf[p + '.mlp.gate.weight'].T)
        assert len(L['experts']) == E and 'w1w3' not in L
        for x in (0, 1, E // 2, E - 1):
            g, u, d = (quant[f'{p}.mlp.experts.{x}.{n}'] for n in ('gate_proj', 'up_proj', 'down_proj'))
            exp13 = checkpoint._fuse_w1w3(dict(g), dict(u))
            got13, got2 = L['experts'][x]['w1w3'], L['experts'][x]['w2']
            assert set(got13) == set(exp13)
            for kk in exp13:
                assert np.array_equal(got13[kk], exp13[kk]), (li, x, kk)
            for kk in d:
                assert np.array_equal(got2[kk], d[kk]), (li, x, kk)
            if fmt == 'awq':       # (gate_j, up_j) column interleave of codes, scales and zeros
                assert got13['q'].shape == (H, 2 * I) and got13['s'].shape == (H // 128, 2 * I)
                assert np.array_equal(got13['q'][:, 0::2], g['q']) and np.array_equal(got13['q'][:, 1::2], u['q'])
                assert np.array_equal(got13['s'][:, 1::2], u['s']) and np.array_equal(got13['z'][:, 0::2], g['z'])
            else:                  # codes interleaved; scale row [w1 blocks | w3 blocks]
                assert got13['f8'].shape == (H, 2 * I) and got13['bs'].shape == (H // 128, 2 * (I // 128)) and got13['gated']
                assert np.array_equal(got13['f8'][:, 0::2], g['f8']) and np.array_equal(got13['f8'][:, 1::2], u['f8'])
                assert np.array_equal(got13['bs'], np.concatenate([g['bs'], u['bs']], axis=1))
        a = p + '.self_attn.'
        for n in ('q_norm', 'k_norm'):     # permuted as one head, like the dense Qwen3 reader
            assert np.array_equal(L[n], o.permute_qk_for_interleaved_rope(hf[a + n + '.weight'], 1, 128))
            assert np.array_equal(L[n][0::2], hf[a + n + '.weight'][:64])
        assert 'qkv_bias' not in L
        key = 'q' if fmt == 'awq' else 'f8'
        qp = o.permute_qk_for_interleaved_rope(quant[a + 'q_proj'][key], HQ, 128)
        assert np.array_equal(L['w_qkv'][key][:, :HQ * 128], qp)

    # engine slots.  An expert width of 128 leaves 64 columns per rank at tp = 2, which breaks the 128 rule: that is the refusal;
    # sharded expert slots are checked at the published widths in test_export_expert_width_tp_rule
    wname = 'qweight' if fmt == 'awq' else 'weight'
    with pytest.raises(ValueError, match='multiple of 128'):
        loader.export_weights(mc, w, 2, 0)
    slots = loader.export_weights(mc, w, 1, 0)
    assert slots['layers.1.moe_ffn.gate.weight'].shape == (H, E) and slots['layers.1.moe_ffn.gate.weight'].dtype == f16
    assert 'layers.0.feed_forward.w1w3.' + wname not in slots
    for x in (0, E - 1):
        q = f'layers.0.moe_ffn.experts.{x}'
        if fmt == 'awq':
            assert slots[q + '.w1w3.qweight'].shape == (H, 2 * I // 8) and slots[q + '.w1w3.scales'].shape == (H // 128, 2 * I)
            assert slots[q + '.w2.qweight'].shape == (I, H // 8) and slots[q + '.w2.zeros'].shape == (I // 128, H)
        else:
            assert slots[q + '.w1w3.weight'].shape == (H, 2 * I) and slots[q + '.w1w3.scales'].shape == (H // 128, 2 * I // 128)
            assert slots[q + '.w2.weight'].shape == (I, H) and slots[q + '.w2.scales'].shape == (I // 128, H // 128)
    assert np.array_equal(slots['layers.0.attention.q_norm.weight'], w['layers'][0]['q_norm'])
    n_expert_slots = sum(1 for s in slots if '.moe_ffn.experts.' in s)
    assert n_expert_slots == LAYERS * E * (6 if fmt == 'awq' else 4)

@pytest.mark.parametrize('fmt', ['u4', 'fp8'])
def test_export_expert_width_tp_rule(fmt):
    """moe_intermediate_size / tp must be a multiple of 128: Qwen3-30B-A3B's 768 shards at 2, 3, 6 and not at 4, 8; 1536 at
    2, 3, 4, 6, 12 and not at 8.  (Small H, 4 experts: the rule is about the expert width alone.)"""
    from tests.qwen_moe_reference import QwenMoeConfig
    for inter, good, bad in ((768, (1, 2, 3, 6), (4, 8)), (1536, (2, 3, 4, 6, 12), (8,))):
        cfg = QwenMoeConfig(hidden=128, layers=1, q_heads=24, kv_heads=24, head_dim=128, inter=inter, vocab=48, weight_format=fmt,
                            moe_experts=4, moe_top_k=2)
        rng = np.random.default_rng(0)

        def lin(K, N, gated=False):
            if fmt == 'u4':
                return dict(q=rng.integers(0, 16, (K, N), dtype=np.uint8), s=np.ones((K // 128, N), f16), z=np.ones((K // 128, N), f16))
            d = dict(f8=rng.integers(0, 120, (K, N), dtype=np.uint8), bs=np.ones((K // 128, N // 128), np.float32))
            return dict(d, gated=True) if gated else d
        L = dict(attn_norm=np.ones(128, f16), ffn_norm=np.ones(128, f16), w_qkv=lin(128, 72 * 128), wo=lin(24 * 128, 128),
                 moe_gate=np.zeros((128, 4), f16),
                 experts=[dict(w1w3=lin(128, 2 * inter, True), w2=lin(inter, 128)) for _ in range(4)])
        w = dict(tok_embeddings=np.zeros((48, 128), f16), layers=[L], norm=np.ones(128, f16), output=np.zeros((128, 48), f16))
        for tp in good:
            for r in (0, tp - 1):
                slots = loader.export_weights(cfg, w, tp, r)
                n13 = slots['layers.0.moe_ffn.experts.3.w1w3.' + ('qweight' if fmt == 'u4' else 'weight')].shape[1]
                assert n13 == (2 * inter // tp // 8 if fmt == 'u4' else 2 * inter // tp)
        for tp in bad:
            with pytest.raises(ValueError, match='multiple of 128'):
                loader.export_weights(cfg, w, tp, 0)
