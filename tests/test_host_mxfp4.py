"""MXFP4 experts and the gpt-oss MoE block, host side: the reference arithmetic of tests/mxfp4_reference.py at its edges, the
sharpness of the exact blocks (every fault the path can have changes an output bit), the checkpoint -> slot mapping, and the config
plumbing.  No GPU."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd.turbomind import checkpoint, loader
from lmdeploy_amd.turbomind.engine import make_model_config
from oracle import tm_oracle as o
from tests import mxfp4_reference as r

f16, f32, f64 = np.float16, np.float32, np.float64


def test_dequant_every_code_and_scale_edge():
    """all 16 codes under the scale bytes 0, 112, 113, 127, 141, 142, 143, 255: the flush to +0 (keeping the code's sign), 2^(s - 127)
    in between, the clamp at 2^15, -0, and inf exactly where 6 x 2^15 overflows"""
    codes = np.tile(np.arange(16, dtype=np.uint8), 2)[None, :].repeat(len(r.SCALE_BYTES), 0)      # [8][32]: one group per row
    scales = np.array(r.SCALE_BYTES, np.uint8)[:, None]
    w = r.dequant(r.pack_codes(codes), scales).T                                                  # [8][32]
    mag = np.array([0, .5, 1, 1.5, 2, 3, 4, 6], f64)
    val = np.concatenate([mag, -mag])
    for i, s in enumerate(r.SCALE_BYTES):
        sc = 0.0 if s <= 112 else 2.0**(min(s, 142) - 127)
        want = np.tile(val * sc, 2)
        got = w[i].astype(f64)
        # one fp16 multiply: exact when finite; the product overflows (to inf of its sign) only past fp16's 65504, i.e. from
        # 4 x 2^14 and 2 x 2^15 on -- 6 x 2^15 among them -- and nowhere at the smaller scales
        over = np.abs(want) > 65504
        assert over.any() == (s >= 141) and (not over.any() or over[7])
        assert np.array_equal(got, np.where(over, np.copysign(np.inf, want), want)), s
        assert np.array_equal(np.signbit(w[i]), np.tile(np.arange(16) >= 8, 2)), 'code 8 is -0; a flushed weight keeps its sign'
    assert r.scale_f16(113) == f16(2.0**-14) and r.scale_f16(112) == 0 and r.scale_f16(255) == f16(32768.0)
    # the nibble order of the checkpoint: the low nibble is the even k
    assert np.array_equal(r.unpack_codes(np.array([[0x2B]], np.uint8)), [[0xB, 0x2]])


def test_activation_edges():
    gu = np.array([[8.0, 0.5, 7.0, 9.0, -3.0, -9.0, 0.0, 2.0]], f16)
    a = r.gptoss_act(gu).astype(f64)[0]
    sig = lambda g: g / (1 + np.exp(-1.702 * g))
    want = [sig(7.0) * 1.5, sig(7.0) * 8.0, sig(-3.0) * -6.0, 0.0]
    assert np.allclose(a, want, rtol=2**-10, atol=0)
    b = np.zeros(8, f16)
    b[0], b[1] = -8.0, 0.25
    assert r.gptoss_act(gu, b)[0, 0] == 0 and r.gptoss_act(gu, b)[0, 1] == a[1]


@pytest.fixture(scope='module')
def blk():
    return r.exact_block(256, 128, 8, 2, 17)


def test_exact_block_is_sharp(blk):
    """each fault changes an output bit of the exact block: swapped nibbles, a scale group off by one, swapped gate / up, the
    neighbouring expert's bias, no clamp, no 1.702, no 1 + up, the router bias dropped"""
    base = [r.dense(ex) for ex in blk.experts]
    ref, ids, _ = r.block_forward(blk.x, blk.gate, blk.gate_bias, base, 2, exact=True)
    assert np.array_equal(r.bits(ref), r.bits(blk.out)) and np.array_equal(ids, blk.ids)
    for mut in r.MUTATIONS:
        ex = base
        if mut in ('nibbles', 'scale_group'):
            ex = [dict(d, w13=r.dequant(**e['w1w3'], mut=mut), w2=r.dequant(**e['w2'], mut=mut)) for d, e in zip(base, blk.experts)]
        out, ids2, _ = r.block_forward(blk.x, blk.gate, blk.gate_bias, ex, 2, mut=mut, exact=True)
        changed = int((r.bits(out) != r.bits(ref)).sum())
        print(f'{mut}: {changed} of {ref.size} outputs change')
        assert changed > 0, mut
        assert (mut == 'no_router_bias') == (not np.array_equal(ids2, blk.ids)), mut
    # a single code off by one shows as well (the GPU tests' negative control)
    e0 = int(blk.ids[0, 0])
    c = r.unpack_codes(blk.experts[e0]['w2']['blocks'])
    c[5, 3] ^= 1
    ex = list(base)
    ex[e0] = dict(base[e0], w2=r.dequant(r.pack_codes(c), blk.experts[e0]['w2']['scales']))
    out, _, _ = r.block_forward(blk.x, blk.gate, blk.gate_bias, ex, 2, exact=True)
    assert (r.bits(out) != r.bits(ref)).any()


@pytest.mark.parametrize('E,k,T', [(8, 2, 1), (8, 2, 65), (72, 8, 3), (72, 8, 33)])
def test_exact_blocks_build(E, k, T):
    """the builder's budgets hold at the sizes the GPU tests use (its assertions are the test)"""
    b = r.exact_block(256, 128, E, k, T)
    assert b.out.shape == (T, 256) and max(b.worst) <= r.BUDGET
    print(f'E {E} k {k} T {T}: sum |terms| / lattice w1w3 {b.worst[0]:.0f}, w2 {b.worst[1]:.0f}')


def _published(rng, E, H, I):
    m = 'model.layers.1.mlp'
    return {f'{m}.experts.gate_up_proj_blocks': rng.integers(0, 256, (E, 2 * I, H // 32, 16), dtype=np.uint8),
            f'{m}.experts.gate_up_proj_scales': rng.integers(118, 124, (E, 2 * I, H // 32), dtype=np.uint8),
            f'{m}.experts.gate_up_proj_bias': rng.standard_normal((E, 2 * I)).astype(f32),
            f'{m}.experts.down_proj_blocks': rng.integers(0, 256, (E, H, I // 32, 16), dtype=np.uint8),
            f'{m}.experts.down_proj_scales': rng.integers(118, 124, (E, H, I // 32), dtype=np.uint8),
            f'{m}.experts.down_proj_bias': rng.standard_normal((E, H)).astype(f32),
            f'{m}.router.weight': rng.standard_normal((E, H)).astype(f32),
            f'{m}.router.bias': rng.standard_normal(E).astype(f32)}


def test_gpt_oss_expert_slots_round_trip():
    """the published tensors -> slots: bytes kept, [N, K/32, 16] flattened to [N, K/2]; the dequantised w1w3 [H][2I] has the gate in
    its even and the up projection in its odd columns (o.interleave_w1w3 of the two), as transformers' GptOssExperts reads them
    (gate_up[..., ::2], gate_up[..., 1::2]; low nibble = even k)"""
    E, H, I = 3, 64, 32
    t = _published(np.random.default_rng(5), E, H, I)
    s = checkpoint.gpt_oss_expert_slots(t, 1)
    m, p = 'model.layers.1.mlp', 'layers.1.moe_ffn'
    assert len(s) == 2 + 6 * E
    assert s[p + '.gate.weight'].shape == (H, E) and s[p + '.gate.weight'].dtype == f16 and s[p + '.gate.bias'].dtype == f32
    assert np.array_equal(s[p + '.gate.weight'], t[m + '.router.weight'].astype(f16).T)
    assert np.array_equal(s[p + '.gate.bias'], t[m + '.router.bias'])
    lut = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0.0, -.5, -1, -1.5, -2, -3, -4, -6], f32)
    for x in range(E):
        q = f'{p}.experts.{x}'
        blocks, scales = s[q + '.w1w3.blocks'], s[q + '.w1w3.scales']
        assert blocks.shape == (2 * I, H // 2) and scales.shape == (2 * I, H // 32) and blocks.flags['C_CONTIGUOUS']
        assert s[q + '.w2.blocks'].shape == (H, I // 2) and s[q + '.w2.scales'].shape == (H, I // 32)
        assert blocks.tobytes() == t[m + '.experts.gate_up_proj_blocks'][x].tobytes()
        assert np.array_equal(s[q + '.w1w3.bias'], t[m + '.experts.gate_up_proj_bias'][x].astype(f16))
        assert np.array_equal(s[q + '.w2.bias'], t[m + '.experts.down_proj_bias'][x].astype(f16)) and s[q + '.w2.bias'].dtype == f16
        # the published dequantisation (integrations/mxfp4.py: out[:, 0::2] = lut[blk & 15], out[:, 1::2] = lut[blk >> 4], times 2^(s - 127))
        blk = t[m + '.experts.gate_up_proj_blocks'][x]
        full = np.empty((2 * I, H // 32, 32), f32)
        full[..., 0::2], full[..., 1::2] = lut[blk & 15], lut[blk >> 4]
        full = (full * np.exp2(t[m + '.experts.gate_up_proj_scales'][x].astype(f32) - 127)[..., None]).reshape(2 * I, H)
        w13 = r.dequant(blocks, scales)                                                           # [H][2I]
        assert np.array_equal(w13.astype(f32), full.T)
        assert np.array_equal(w13, o.interleave_w1w3(np.ascontiguousarray(full[0::2].T).astype(f16), np.ascontiguousarray(full[1::2].T).astype(f16)))
    bad = dict(t)
    bad[m + '.experts.down_proj_scales'] = bad[m + '.experts.down_proj_scales'][:, :-1]
    with pytest.raises(ValueError, match='tensor shapes'):
        checkpoint.gpt_oss_expert_slots(bad, 1)


def test_export_weights_emits_the_gptoss_slots():
    cfg = r.GptOssMoeConfig(**r.GPTOSS_MOE_CFG)
    w = r.make_gptoss_weights(cfg, seed=2)
    s = loader.export_weights(cfg, w)
    q = 'layers.1.moe_ffn.experts.7'
    assert s[q + '.w1w3.blocks'].shape == (256, 128) and s[q + '.w1w3.blocks'].dtype == np.uint8
    assert s[q + '.w1w3.scales'].shape == (256, 8) and s[q + '.w2.blocks'].shape == (256, 64) and s[q + '.w2.scales'].shape == (256, 4)
    assert s[q + '.w1w3.bias'].shape == (256,) and s[q + '.w2.bias'].shape == (256,) and s[q + '.w2.bias'].dtype == f16
    assert s['layers.0.moe_ffn.gate.bias'].shape == (8,) and s['layers.0.moe_ffn.gate.bias'].dtype == f32
    assert q + '.w1w3.weight' not in s and s['layers.0.attention.wo.weight'].dtype == f16
    with pytest.raises(ValueError, match='do not shard over tp = 2'):
        loader.export_weights(cfg, w, tp=2, rank=0)
    mc = make_model_config(cfg, weight_type=1)
    assert (mc.moe_expert_format, mc.moe_act, mc.moe_bias, mc.moe_experts, mc.weight_type) == (3, 1, 1, 8, 1)


def test_read_config_names_what_gpt_oss_still_needs(tmp_path):
    c = dict(architectures=['GptOssForCausalLM'], hidden_size=2880, num_attention_heads=64, num_key_value_heads=8, head_dim=64,
             num_hidden_layers=24, intermediate_size=2880, vocab_size=201088, num_local_experts=32, num_experts_per_tok=4,
             quantization_config=dict(quant_method='mxfp4'))
    with open(os.path.join(tmp_path, 'config.json'), 'w') as f:
        json.dump(c, f)
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    msg = str(ei.value)
    assert 'GptOssForCausalLM' in msg and '% 128' in msg and '2880' in msg and 'o_proj bias' in msg
    assert 'the MI355X hot path covers' not in msg, 'the generic architecture message'


def test_tile_table_and_symbols_take_the_mxfp4_kind(tmp_path):
    """the measured-dispatch table accepts row tiles for grouped MXFP4 GEMMs (kind 32 + 3) as for the other formats, the header, the
    ctypes table and the library agree on the new entry points"""
    import re

    from lmdeploy_amd import _ffi
    lib = _ffi.load()
    path = os.path.join(tmp_path, 'table.txt')
    with open(path, 'w') as f:      # (a shape no test runs: the table is process-wide)
        f.write('G 35 0 1152 640 64 32 0 0 0\nG 35 0 1152 768 64 48 0 0 0\nG 35 0 1152 896 128 32 0 0 0\n')
    _ffi.check(lib.tm_gemm_import(path.encode()))
    rows = _ffi.C.c_int(-1)
    for N, want in ((640, 32), (768, 0), (896, 0)):      # 48 rows is no tile; decode buckets only
        _ffi.check(lib.tm_debug_grouped_tile(3, 1152, N, 64 if N != 896 else 128, _ffi.C.byref(rows)))
        assert rows.value == want, N
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tm_mi355x.h')).read()
    assert re.search(r'TM_WEIGHT_MXFP4\s*=\s*3', hdr)
    for name in ('tm_moe_set_activation', 'tm_moe_set_gate_bias', 'tm_moe_set_expert_bias', 'tm_mxfp4_dequant_f16'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _ffi.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_model_config_defaults_are_unchanged():
    mc = checkpoint.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024)
    assert (mc.moe_expert_format, mc.moe_act, mc.moe_bias) == (0, 0, 0)
    f = make_model_config(mc)
    assert (f.moe_expert_format, f.moe_act, f.moe_bias, f.moe_shared_inter, f.attn_window, f.attn_bias, f.qk_norm) == (0,) * 7
    plain = make_model_config(o.ModelConfig(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024))
    assert (plain.moe_expert_format, plain.moe_act, plain.moe_bias) == (0, 0, 0)
    from lmdeploy_amd.pipeline import SYNTHETIC
    g = checkpoint.ModelConfig(**SYNTHETIC['tiny_gptoss_moe'])
    tiny = checkpoint.ModelConfig(**SYNTHETIC['tiny_moe'])
    assert (g.moe_expert_format, g.moe_act, g.moe_bias) == (3, 1, 1) and (tiny.moe_expert_format, tiny.moe_act, tiny.moe_bias) == (0, 0, 0)
    assert (g.hidden, g.inter, g.moe_experts, g.moe_top_k) == (tiny.hidden, tiny.inter, tiny.moe_experts, tiny.moe_top_k) == (256, 128, 8, 2)
