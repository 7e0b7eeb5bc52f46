"""Qwen2-MoE on the host side: config reading at the published geometries and its refusals, reading a fabricated AWQ / block-FP8
checkpoint (router, experts, the shared expert as a dense FFN, its gate vector), the engine slots and their tensor-parallel shards."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd.turbomind import checkpoint, loader
from lmdeploy_amd.turbomind.engine import make_model_config
from oracle import tm_oracle as o
from tests.qwen2_moe_reference import hf_qwen2_moe_tensors, qwen2_moe_config_json, write_qwen2_moe_checkpoint

f16 = np.float16


def _a27b(**extra):
    """config.json of Qwen1.5-MoE-A2.7B (AWQ)"""
    c = qwen2_moe_config_json(2048, 16, 16, 1408, 5632, 60, 4, 151936, 24, 'awq')
    c.update(extra)
    return c


def _57b(**extra):
    """config.json of Qwen2-57B-A14B (AWQ)"""
    c = qwen2_moe_config_json(3584, 28, 4, 2560, 20480, 64, 8, 151936, 28, 'awq')
    c.update(extra)
    return c


def _write(path, c):
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)


@pytest.mark.parametrize('cfg,want', [
    (_a27b(), (2048, 16, 16, 60, 4, 1408, 5632, 24)),
    (_57b(), (3584, 28, 4, 64, 8, 2560, 20480, 28)),
])
def test_read_config_qwen2_moe_published(tmp_path, cfg, want):
    _write(tmp_path, cfg)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.arch, mc.attn_bias, mc.qk_norm, mc.head_dim) == ('qwen2', 1, 0, 128)
    assert (mc.hidden, mc.q_heads, mc.kv_heads, mc.moe_experts, mc.moe_top_k, mc.inter, mc.moe_shared_inter, mc.layers) == want
    assert (mc.moe_norm_topk, mc.moe_routed_scale, mc.quantized, mc.weight_format) == (False, 1.0, True, 'u4')
    mcfg = make_model_config(mc)
    assert (mcfg.moe_experts, mcfg.moe_top_k, mcfg.moe_norm_topk, mcfg.inter, mcfg.moe_shared_inter, mcfg.attn_bias, mcfg.qk_norm) == \
        (want[3], want[4], 0, want[5], want[6], 1, 0)


def test_read_config_qwen2_moe_norm_topk_and_fp8(tmp_path):
    c = _57b(norm_topk_prob=True)
    c['quantization_config'] = {'quant_method': 'fp8', 'weight_block_size': [128, 128]}
    _write(tmp_path, c)
    mc = checkpoint.read_config(str(tmp_path))
    assert (mc.weight_format, mc.moe_norm_topk, mc.moe_shared_inter) == ('fp8', True, 20480)


def test_model_config_without_the_field_has_no_shared_expert():
    cfg = o.ModelConfig(hidden=256, layers=1, q_heads=4, kv_heads=2, head_dim=128, inter=128, vocab=64, moe_experts=4, moe_top_k=2)
    assert make_model_config(cfg).moe_shared_inter == 0


def _without(c, *keys):
    return {k: v for k, v in c.items() if k not in keys}


@pytest.mark.parametrize('label,cfg,needle', [
    ('no num_experts', _without(_a27b(), 'num_experts'), 'num_experts'),
    ('no num_experts_per_tok', _without(_a27b(), 'num_experts_per_tok'), 'num_experts_per_tok'),
    ('no moe_intermediate_size', _without(_a27b(), 'moe_intermediate_size'), 'moe_intermediate_size'),
    ('no shared_expert_intermediate_size', _without(_a27b(), 'shared_expert_intermediate_size'), 'shared_expert_intermediate_size'),
    ('mlp_only_layers', _a27b(mlp_only_layers=[0, 3]), 'mlp_only_layers'),
    ('decoder_sparse_step', _a27b(decoder_sparse_step=2), 'decoder_sparse_step'),
    ('num_experts 512', _a27b(num_experts=512), '256'),
    ('top 10', _a27b(num_experts_per_tok=10), 'top-8'),
    ('head_dim 64', _a27b(head_dim=64), 'head_dim'),
    ('sliding window', _a27b(use_sliding_window=True), 'sliding'),
    ('yarn', _a27b(rope_scaling={'rope_type': 'yarn', 'factor': 4.0, 'original_max_position_embeddings': 32768}), 'yarn'),
    ('dynamic rope', _a27b(rope_scaling={'type': 'dynamic', 'factor': 2.0}), 'dynamic'),
    ('bf16 experts', _without(_a27b(), 'quantization_config'), 'experts'),
    ('shared width 1000', _a27b(shared_expert_intermediate_size=1000), 'multiple of 128'),
])
def test_read_config_qwen2_moe_refusals(tmp_path, label, cfg, needle):
    _write(tmp_path, cfg)
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert needle in str(ei.value), f'{label}: the message does not name the reason: {ei.value}'
    if label.startswith('no '):
        assert 'Qwen2MoeForCausalLM' in str(ei.value)


def test_read_config_missing_keys_are_all_named(tmp_path):
    _write(tmp_path, _without(_a27b(), 'num_experts', 'shared_expert_intermediate_size'))
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    msg = str(ei.value)
    assert 'num_experts' in msg and 'shared_expert_intermediate_size' in msg and 'num_experts_per_tok' not in msg


H, HQ, HKV, I, S, E, K, V, LAYERS = 256, 4, 2, 128, 384, 60, 4, 96, 2


@pytest.fixture(scope='module', params=['awq', 'fp8'])
def ckpt(request, tmp_path_factory):
    """one fabricated checkpoint per format, read once: (fmt, hf tensors, what was written, config, weights)"""
    path = str(tmp_path_factory.mktemp('qwen2moe_' + request.param))
    rng = np.random.default_rng(4)
    hf = hf_qwen2_moe_tensors(rng, H, HQ, HKV, I, S, E, V, LAYERS)
    quant = write_qwen2_moe_checkpoint(path, hf, H, HQ, HKV, I, S, E, K, V, LAYERS, request.param)
    mc = checkpoint.read_config(path)
    return request.param, path, hf, quant, mc, checkpoint.load_hf_weights(path, mc)


def _dequant(lin, gated=False):
    return o._dense_weight(dict(lin, gated=True) if gated and 'f8' in lin else lin, 128)


def test_load_qwen2_moe_checkpoint(ckpt):
    """H 256, 2 layers, 60 experts, top-4, expert width 128, shared width 384"""
    fmt, _, hf, quant, mc, w = ckpt
    assert (mc.arch, mc.attn_bias, mc.qk_norm, mc.moe_experts, mc.moe_top_k, mc.inter, mc.moe_shared_inter, mc.moe_norm_topk) == \
        ('qwen2', 1, 0, E, K, I, S, False)
    assert mc.weight_format == ('u4' if fmt == 'awq' else 'fp8')
    assert len(w['layers']) == LAYERS
    for li, L in enumerate(w['layers']):
        p = f'model.layers.{li}'
        assert L['moe_gate'].dtype == f16 and np.array_equal(L['moe_gate'], hf[p + '.mlp.gate.weight'].T)
        assert len(L['experts']) == E
        for x in (0, E // 2, E - 1):
            g, u, d = (quant[f'{p}.mlp.experts.{x}.{n}'] for n in ('gate_proj', 'up_proj', 'down_proj'))
            exp13 = checkpoint._fuse_w1w3(dict(g), dict(u))
            for kk in exp13:
                assert np.array_equal(L['experts'][x]['w1w3'][kk], exp13[kk]), (li, x, kk)
            for kk in d:
                assert np.array_equal(L['experts'][x]['w2'][kk], d[kk]), (li, x, kk)
        # the shared expert: a dense FFN of width S, fused like one; dequantised, it is what was written
        g, u, d = (quant[f'{p}.mlp.shared_expert.{n}'] for n in ('gate_proj', 'up_proj', 'down_proj'))
        got13 = _dequant(L['w1w3'], gated=True)
        assert got13.shape == (H, 2 * S)
        assert np.array_equal(got13[:, 0::2], _dequant(g)) and np.array_equal(got13[:, 1::2], _dequant(u))
        assert np.array_equal(_dequant(L['w2']), _dequant(d)) and _dequant(L['w2']).shape == (S, H)
        if fmt == 'fp8':
            assert L['w1w3']['gated'] and L['w1w3']['bs'].shape == (H // 128, 2 * S // 128)
        # the gate: [1, H] in the checkpoint -> fp16 [H]
        assert L['shared_gate'].dtype == f16 and L['shared_gate'].shape == (H,)
        assert np.array_equal(L['shared_gate'], hf[p + '.mlp.shared_expert_gate.weight'][0])
        a = p + '.self_attn.'
        assert np.array_equal(L['qkv_bias'][-HKV * 128:], hf[a + 'v_proj.bias']) and 'q_norm' not in L


def test_export_qwen2_moe_slots(ckpt):
    fmt, _, _, _, mc, w = ckpt
    wname = 'qweight' if fmt == 'awq' else 'weight'
    slots = loader.export_weights(mc, w, 1, 0)
    for li in range(LAYERS):
        p = f'layers.{li}'
        assert slots[p + '.moe_ffn.shared_gate.weight'].dtype == f16
        assert np.array_equal(slots[p + '.moe_ffn.shared_gate.weight'], w['layers'][li]['shared_gate'])
        assert slots[p + '.moe_ffn.gate.weight'].shape == (H, E)
        if fmt == 'awq':
            assert slots[p + '.feed_forward.w1w3.qweight'].shape == (H, 2 * S // 8) and slots[p + '.feed_forward.w2.qweight'].shape == (S, H // 8)
            assert slots[p + '.feed_forward.w1w3.scales'].shape == (H // 128, 2 * S)
        else:
            assert slots[p + '.feed_forward.w1w3.weight'].shape == (H, 2 * S) and slots[p + '.feed_forward.w1w3.scales'].shape == (H // 128, 2 * S // 128)
            assert slots[p + '.feed_forward.w2.weight'].shape == (S, H) and slots[p + '.feed_forward.w2.scales'].shape == (S // 128, H // 128)
    assert sum(1 for s in slots if '.moe_ffn.experts.' in s) == LAYERS * E * (6 if fmt == 'awq' else 4)
    assert 'layers.0.moe_ffn.experts.0.w1w3.' + wname in slots
    # the expert width 128 leaves 64 columns per rank at tp = 2: refused as for Qwen3-MoE; so is a shared width that does not shard
    with pytest.raises(ValueError, match='multiple of 128'):
        loader.export_weights(mc, w, 2, 0)


@pytest.mark.parametrize('fmt', ['u4', 'fp8'])
def test_export_shared_expert_tp2(fmt):
    """tp = 2 (expert width 256, shared width 512): the shared w1w3 keeps (gate_j, up_j) pairs together -- rank r owns the inter
    columns [r S / 2, (r + 1) S / 2) of both --, the w2 row halves match, the gate is replicated; shared width 384 is refused at
    tp = 2 (192 per rank)"""
    from tests.qwen2_moe_reference import Qwen2MoeConfig
    Hh, Ii, Ss, Ee = 128, 256, 512, 4
    rng = np.random.default_rng(0)

    def lin(K, N, gated=False):
        if fmt == 'u4':
            return dict(q=rng.integers(0, 16, (K, N), dtype=np.uint8), s=rng.standard_normal((K // 128, N)).astype(f16),
                        z=rng.integers(0, 16, (K // 128, N)).astype(f16))
        d = dict(f8=rng.integers(0, 120, (K, N), dtype=np.uint8), bs=rng.random((K // 128, N // 128)).astype(np.float32))
        return dict(d, gated=True) if gated else d

    def model(shared):
        cfg = Qwen2MoeConfig(hidden=Hh, layers=1, q_heads=2, kv_heads=2, head_dim=128, inter=Ii, vocab=48, weight_format=fmt,
                             moe_experts=Ee, moe_top_k=2, moe_shared_inter=shared)
        L = dict(attn_norm=np.ones(Hh, f16), ffn_norm=np.ones(Hh, f16), w_qkv=lin(Hh, 6 * 128), wo=lin(2 * 128, Hh),
                 qkv_bias=np.zeros(6 * 128, f16), moe_gate=np.zeros((Hh, Ee), f16),
                 experts=[dict(w1w3=lin(Hh, 2 * Ii, True), w2=lin(Ii, Hh)) for _ in range(Ee)],
                 w1w3=lin(Hh, 2 * shared, True), w2=lin(shared, Hh), shared_gate=rng.standard_normal(Hh).astype(f16))
        return cfg, dict(tok_embeddings=np.zeros((48, Hh), f16), layers=[L], norm=np.ones(Hh, f16), output=np.zeros((Hh, 48), f16)), L
    cfg, w, L = model(Ss)
    half = Ss // 2
    for r in range(2):
        slots = loader.export_weights(cfg, w, 2, r)
        assert np.array_equal(slots['layers.0.moe_ffn.shared_gate.weight'], L['shared_gate'])
        if fmt == 'u4':
            q13 = o.unpack_u4_row(slots['layers.0.feed_forward.w1w3.qweight'])
            assert q13.shape == (Hh, 2 * half)
            assert np.array_equal(q13[:, 0::2], L['w1w3']['q'][:, 0::2][:, r * half:(r + 1) * half])       # gate columns of the rank
            assert np.array_equal(q13[:, 1::2], L['w1w3']['q'][:, 1::2][:, r * half:(r + 1) * half])       # their up columns
            assert np.array_equal(slots['layers.0.feed_forward.w1w3.scales'], L['w1w3']['s'][:, 2 * r * half:2 * (r + 1) * half])
            assert np.array_equal(o.unpack_u4_row(slots['layers.0.feed_forward.w2.qweight']), L['w2']['q'][r * half:(r + 1) * half])
            assert np.array_equal(slots['layers.0.feed_forward.w2.zeros'], L['w2']['z'][r * half // 128:(r + 1) * half // 128])
        else:
            c13, b13 = slots['layers.0.feed_forward.w1w3.weight'], slots['layers.0.feed_forward.w1w3.scales']
            assert c13.shape == (Hh, 2 * half) and b13.shape == (1, 2 * half // 128)
            assert np.array_equal(c13[:, 0::2], L['w1w3']['f8'][:, 0::2][:, r * half:(r + 1) * half])
            assert np.array_equal(c13[:, 1::2], L['w1w3']['f8'][:, 1::2][:, r * half:(r + 1) * half])
            nb, hb = Ss // 128, half // 128
            assert np.array_equal(b13, np.concatenate([L['w1w3']['bs'][:, r * hb:(r + 1) * hb], L['w1w3']['bs'][:, nb + r * hb:nb + (r + 1) * hb]], 1))
            assert np.array_equal(slots['layers.0.feed_forward.w2.weight'], L['w2']['f8'][r * half:(r + 1) * half])
            assert np.array_equal(slots['layers.0.feed_forward.w2.scales'], L['w2']['bs'][r * hb:(r + 1) * hb])
    cfg, w, _ = model(384)
    with pytest.raises(ValueError, match='shared expert of width 384'):
        loader.export_weights(cfg, w, 2, 0)


def test_quantised_shared_gate_is_refused(ckpt, tmp_path):
    """a checkpoint whose shared_expert_gate was quantised along with the projections: refused with a message"""
    fmt, path, _, _, mc, _ = ckpt
    import torch
    from safetensors import safe_open
    from safetensors.torch import save_file
    with safe_open(os.path.join(path, 'model.safetensors'), framework='pt') as f:
        tensors = {k: f.get_tensor(k) for k in f.keys()}
    sg = 'model.layers.0.mlp.shared_expert_gate'
    tensors.pop(sg + '.weight')
    if fmt == 'awq':
        tensors[sg + '.qweight'] = torch.zeros((H, 1), dtype=torch.int32)
    else:
        tensors[sg + '.weight'] = torch.zeros((1, H), dtype=torch.uint8).view(torch.float8_e4m3fn)
        tensors[sg + '.weight_scale_inv'] = torch.ones((1, H // 128), dtype=torch.float32)
    save_file(tensors, os.path.join(str(tmp_path), 'model.safetensors'))
    for n in ('config.json', 'generation_config.json'):
        with open(os.path.join(path, n)) as f, open(os.path.join(str(tmp_path), n), 'w') as g:
            g.write(f.read())
    with pytest.raises(NotImplementedError, match='shared_expert_gate'):
        checkpoint.load_hf_weights(str(tmp_path), mc)
