"""Per-tensor and per-channel FP8 checkpoints on the host: the two config dialects and every accepted scale shape through
read_config / load_hf_weights, the column scales following the q / k permutation, the q | k | v concatenation and the w1w3
interleave, every refusal with its needle, the shard arithmetic for tp = 2, static checkpoints (input_scale / k_scale / v_scale read
past), and the reference model (tests/fp8_channel_reference.py) against transformers' LlamaForCausalLM on the dequantised values."""
import json
import os

import numpy as np
import pytest

from lmdeploy_amd.turbomind import checkpoint
from lmdeploy_amd.turbomind.loader import export_weights
from oracle import tm_oracle as o
from tests import fp8_channel_reference as r

f16, f32 = np.float16, np.float32


def _load(path, tp=1, rank=0):
    cfg = checkpoint.read_config(path, tp)
    w = checkpoint.load_hf_weights(path, cfg)
    return cfg, w, export_weights(cfg, w, tp, rank)


def _same_linear(a, b, what):
    assert set(a) == {'f8', 'cs'}, (what, sorted(a))
    assert a['cs'].dtype == np.float32 and a['cs'].shape == (a['f8'].shape[1],), what
    assert np.array_equal(a['f8'], b['f8']), what + ': codes'
    assert np.array_equal(a['cs'].view(np.uint32), b['cs'].view(np.uint32)), what + ': scales'


def _same_weights(w, ref):
    for i, (a, b) in enumerate(zip(w['layers'], ref['layers'])):
        for k in ('w_qkv', 'wo'):
            _same_linear(a[k], b[k], f'layers.{i}.{k}')
        if 'experts' in b:
            assert np.array_equal(a['moe_gate'], b['moe_gate']) and a['moe_gate'].dtype == f16
            for x, (ea, eb) in enumerate(zip(a['experts'], b['experts'])):
                for k in ('w1w3', 'w2'):
                    _same_linear(ea[k], eb[k], f'layers.{i}.experts.{x}.{k}')
        else:
            for k in ('w1w3', 'w2'):
                _same_linear(a[k], b[k], f'layers.{i}.{k}')
    assert np.array_equal(w['output'], ref['output']) and w['output'].dtype == f16       # lm_head stays fp16


@pytest.mark.parametrize('dialect,strategy,scale_shape', [('fp8', 'tensor', '[]'), ('fp8', 'tensor', '[1]'),
                                                          ('compressed-tensors', 'tensor', '[1]'), ('compressed-tensors', 'channel', '[N,1]'),
                                                          ('compressed-tensors', 'channel', '[N]')])
@pytest.mark.parametrize('model', ['dense', 'dense-d64', 'mixtral'])
def test_reader_and_loader(tmp_path, model, dialect, strategy, scale_shape):
    """both dialects, every accepted scale shape, dense (head_dim 128 and 64) and Mixtral: channel mode, the weights the reference
    module assembles from the same tensors, fp32 [N] scale slots"""
    geo = {'dense': {}, 'dense-d64': dict(head_dim=64, q_heads=4, kv_heads=2), 'mixtral': dict(experts=4, top_k=2, inter=256)}[model]
    ck = r.write_checkpoint(str(tmp_path), dialect=dialect, strategy=strategy, scale_shape=scale_shape, seed=3, **geo)
    cfg, w, slots = _load(str(tmp_path))
    assert cfg.weight_format == 'fp8' and cfg.fp8_scale_mode == 1 and cfg.quantized and cfg.head_dim == geo.get('head_dim', 128)
    _same_weights(w, r.tm_weights(ck, r.oracle_config(ck, 16)))
    nq = cfg.q_heads * cfg.head_dim + 2 * cfg.kv_heads * cfg.head_dim
    assert slots['layers.0.attention.w_qkv.weight'].dtype == np.uint8 and slots['layers.0.attention.w_qkv.weight'].shape == (256, nq)
    assert slots['layers.0.attention.w_qkv.scales'].dtype == np.float32 and slots['layers.0.attention.w_qkv.scales'].shape == (nq,)
    pre = 'layers.1.moe_ffn.experts.3' if model == 'mixtral' else 'layers.1.feed_forward'
    assert slots[pre + '.w1w3.scales'].shape == (2 * cfg.inter,) and slots[pre + '.w2.scales'].shape == (256,)
    assert slots['output.weight'].dtype == f16


def _rewrite_scales(path, fn):
    """the checkpoint with every .weight_scale replaced by fn(name, old)"""
    import torch
    from safetensors.torch import load_file, save_file
    f = os.path.join(path, 'model.safetensors')
    t = load_file(f)
    for k in list(t):
        if k.endswith('.weight_scale'):
            t[k] = torch.from_numpy(np.ascontiguousarray(fn(k, t[k].numpy()), dtype=f32))
    save_file(t, f)


def test_scales_follow_their_columns(tmp_path):
    """every column's scale is distinct -- 2^((n mod 7) - 3) times a factor per tensor -- so that a wrong mapping cannot cancel: cs
    follows the q / k RoPE permutation, q | k | v concatenate with three different factors, gate / up interleave"""
    r.write_checkpoint(str(tmp_path), dialect='compressed-tensors', strategy='channel', seed=5)
    factor = {'q_proj': 1.0, 'k_proj': 2.0**10, 'v_proj': 2.0**20, 'o_proj': 1.0, 'gate_proj': 1.0, 'up_proj': 2.0**10, 'down_proj': 1.0}

    def distinct(name, old):
        n = np.arange(old.shape[0])
        return (np.exp2((n % 7) - 3.0) * factor[name.split('.')[-2]]).reshape(old.shape)
    _rewrite_scales(str(tmp_path), distinct)
    cfg, w, _ = _load(str(tmp_path))
    D, Hq, Hkv, I = cfg.head_dim, cfg.q_heads, cfg.kv_heads, cfg.inter

    def col(n, f=1.0):
        return np.exp2((np.asarray(n) % 7) - 3.0).astype(f32) * f32(f)
    # HF channel h * D + (j, j + D / 2) of a head -> engine columns h * D + (2 j, 2 j + 1)
    def permuted(heads):
        src = np.arange(heads * D).reshape(heads, 2, D // 2).swapaxes(1, 2).reshape(-1)
        return src
    want_qkv = np.concatenate([col(permuted(Hq)), col(permuted(Hkv), 2.0**10), col(np.arange(Hkv * D), 2.0**20)])
    for L in w['layers']:
        assert np.array_equal(L['w_qkv']['cs'], want_qkv)
        want13 = np.empty(2 * I, f32)
        want13[0::2], want13[1::2] = col(np.arange(I)), col(np.arange(I), 2.0**10)
        assert np.array_equal(L['w1w3']['cs'], want13)
        assert np.array_equal(L['wo']['cs'], col(np.arange(cfg.hidden))) and np.array_equal(L['w2']['cs'], col(np.arange(cfg.hidden)))
    assert len(np.unique(want_qkv[:D])) == 7 and not np.array_equal(want_qkv[:D], col(np.arange(D)))   # the permutation moves scales


def test_three_per_tensor_scales_concatenate(tmp_path):
    """the per-tensor dialect: q, k and v carry three different scalars, each repeated over its own columns"""
    ck = r.write_checkpoint(str(tmp_path), dialect='fp8', strategy='tensor', seed=6)
    cfg, w, _ = _load(str(tmp_path))
    nq, nkv = cfg.q_heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    s = [float(ck[f'model.layers.0.self_attn.{n}_proj.weight_scale']) for n in 'qkv']
    assert len(set(s)) == 3
    assert np.array_equal(w['layers'][0]['w_qkv']['cs'], np.repeat(np.asarray(s, f32), [nq, nkv, nkv]))


def _edit_config(path, fn):
    f = os.path.join(path, 'config.json')
    with open(f) as fh:
        c = json.load(fh)
    fn(c)
    with open(f, 'w') as fh:
        json.dump(c, fh)


def _group(c):
    return c['quantization_config']['config_groups']['group_0']


REFUSALS = [
    ('block strategy', lambda c: _group(c)['weights'].update(strategy='block'), 'weights.strategy'),
    ('group strategy', lambda c: _group(c)['weights'].update(strategy='group', group_size=128), 'weights.strategy'),
    ('int type', lambda c: _group(c)['weights'].update(type='int'), 'weights.type'),
    ('4 bits', lambda c: _group(c)['weights'].update(num_bits=4), 'weights.num_bits'),
    ('asymmetric', lambda c: _group(c)['weights'].update(symmetric=False), 'weights.symmetric'),
    ('int activations', lambda c: _group(c)['input_activations'].update(type='int'), 'input_activations.type'),
    ('16-bit activations', lambda c: _group(c)['input_activations'].update(num_bits=16), 'input_activations.num_bits'),
    ('group activations', lambda c: _group(c)['input_activations'].update(strategy='group'), 'input_activations.strategy'),
    ('two groups', lambda c: c['quantization_config']['config_groups'].update(group_1=_group(c)), 'config_groups'),
    ('other format', lambda c: c['quantization_config'].update(format='pack-quantized'), 'format'),
    ('decoder linear ignored', lambda c: c['quantization_config']['ignore'].append('model.layers.0.mlp.down_proj'), 'ignore'),
]


@pytest.mark.parametrize('what,edit,needle', REFUSALS, ids=[x[0] for x in REFUSALS])
def test_refusals(tmp_path, what, edit, needle):
    r.write_checkpoint(str(tmp_path), dialect='compressed-tensors', strategy='channel', layers=1)
    checkpoint.read_config(str(tmp_path))
    _edit_config(str(tmp_path), edit)
    with pytest.raises(NotImplementedError) as ei:
        checkpoint.read_config(str(tmp_path))
    assert needle in str(ei.value), str(ei.value)


def test_fp8_dialect_refusals_and_scale_shape(tmp_path):
    """quant_method fp8: other block sizes and an ignored decoder linear are refused; a scale of a foreign shape is refused by name;
    activations absent from a compressed-tensors group are fine"""
    r.write_checkpoint(str(tmp_path), dialect='fp8', layers=1)
    _edit_config(str(tmp_path), lambda c: c['quantization_config'].update(weight_block_size=[64, 64]))
    with pytest.raises(NotImplementedError, match='weight_block_size'):
        checkpoint.read_config(str(tmp_path))
    _edit_config(str(tmp_path), lambda c: c['quantization_config'].update(weight_block_size=None, ignored_layers=['lm_head', 'model.layers.0.mlp.up_proj']))
    with pytest.raises(NotImplementedError, match='ignored_layers'):
        checkpoint.read_config(str(tmp_path))
    _edit_config(str(tmp_path), lambda c: c['quantization_config'].update(ignored_layers=['lm_head']))
    _rewrite_scales(str(tmp_path), lambda k, old: np.ones(3, f32) if k.endswith('o_proj.weight_scale') else old)
    cfg = checkpoint.read_config(str(tmp_path))
    with pytest.raises(ValueError, match='o_proj.weight_scale'):
        checkpoint.load_hf_weights(str(tmp_path), cfg)
    r.write_checkpoint(str(tmp_path), dialect='compressed-tensors', strategy='tensor', layers=1)
    _edit_config(str(tmp_path), lambda c: _group(c).update(input_activations=None))
    assert checkpoint.read_config(str(tmp_path)).fp8_scale_mode == 1


def test_block_128_configs_keep_their_path(tmp_path):
    """a config that names [128, 128] stays block mode (and keeps its head_dim-64 refusal)"""
    r.write_checkpoint(str(tmp_path), dialect='fp8', layers=1)
    _edit_config(str(tmp_path), lambda c: c['quantization_config'].update(weight_block_size=[128, 128]))
    cfg = checkpoint.read_config(str(tmp_path))
    assert cfg.weight_format == 'fp8' and cfg.fp8_scale_mode == 0
    _edit_config(str(tmp_path), lambda c: c.update(head_dim=64, num_attention_heads=4))
    with pytest.raises(NotImplementedError, match='head_dim 64'):
        checkpoint.read_config(str(tmp_path))


@pytest.mark.parametrize('dialect', ['fp8', 'compressed-tensors'])
def test_static_scales_are_read_past(tmp_path, dialect):
    """activation_scheme static / kv_cache_scheme with input_scale, k_scale and v_scale tensors: the same slots as without them"""
    kw = dict(dialect=dialect, strategy='tensor', seed=8)
    r.write_checkpoint(str(tmp_path / 'dyn'), **kw)
    ck = r.write_checkpoint(str(tmp_path / 'static'), static=True, **kw)
    assert 'model.layers.0.self_attn.k_proj.k_scale' in ck and 'model.layers.0.mlp.up_proj.input_scale' in ck
    (_, _, a), (_, _, b) = _load(str(tmp_path / 'dyn')), _load(str(tmp_path / 'static'))
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_shards_tp2(tmp_path):
    """column-parallel shards slice cs with their columns (whole (gate, up) pairs for w1w3), row-parallel shards keep it whole;
    the two ranks' pieces put together are the unsharded linears"""
    r.write_checkpoint(str(tmp_path), dialect='compressed-tensors', strategy='channel', q_heads=4, kv_heads=2, seed=9)
    cfg, w, full = _load(str(tmp_path))
    ranks = [export_weights(cfg, w, 2, rk) for rk in (0, 1)]
    D, I = cfg.head_dim, cfg.inter
    L = w['layers'][1]
    p = 'layers.1.'
    nq, nkv = cfg.q_heads * D, cfg.kv_heads * D
    for rk, s in enumerate(ranks):
        cols = np.r_[rk * nq // 2:(rk + 1) * nq // 2, nq + rk * nkv // 2:nq + (rk + 1) * nkv // 2,
                     nq + nkv + rk * nkv // 2:nq + nkv + (rk + 1) * nkv // 2]
        assert np.array_equal(s[p + 'attention.w_qkv.weight'], L['w_qkv']['f8'][:, cols])
        assert np.array_equal(s[p + 'attention.w_qkv.scales'], L['w_qkv']['cs'][cols])
        assert np.array_equal(s[p + 'attention.wo.weight'], L['wo']['f8'][rk * nq // 2:(rk + 1) * nq // 2])
        assert np.array_equal(s[p + 'attention.wo.scales'], L['wo']['cs'])
        assert np.array_equal(s[p + 'feed_forward.w1w3.weight'], L['w1w3']['f8'][:, rk * I:(rk + 1) * I])
        assert np.array_equal(s[p + 'feed_forward.w1w3.scales'], L['w1w3']['cs'][rk * I:(rk + 1) * I])
        assert np.array_equal(s[p + 'feed_forward.w2.weight'], L['w2']['f8'][rk * I // 2:(rk + 1) * I // 2])
        assert np.array_equal(s[p + 'feed_forward.w2.scales'], L['w2']['cs'])
    # a rank's w1w3 columns are whole (gate_j, up_j) pairs: gate scales on its even columns, up scales on its odd ones
    g = r.tm_weights(r.write_checkpoint(str(tmp_path), dialect='compressed-tensors', strategy='channel', q_heads=4, kv_heads=2, seed=9),
                     r.oracle_config(dict(config=json.load(open(os.path.join(str(tmp_path), 'config.json')))), 16))['layers'][1]['w1w3']['cs']
    assert np.array_equal(ranks[1][p + 'feed_forward.w1w3.scales'][0::2], g[I:][0::2])
    assert np.array_equal(np.concatenate([ranks[0][p + 'feed_forward.w1w3.scales'], ranks[1][p + 'feed_forward.w1w3.scales']]),
                          full[p + 'feed_forward.w1w3.scales'])


# Same kind of comparison as tests/test_host_gpt_oss.py::test_reader_and_loader_against_transformers (a toy model in fp32 with eager
# attention against this repository's fp16 reference model, all rows of 20 tokens, KV unquantised) and its bound, HF_BOUND = 2 * 0.01454.
HF_BOUND = 2 * 0.01454


@pytest.mark.parametrize('dialect,strategy', [('fp8', 'tensor'), ('compressed-tensors', 'channel')])
def test_reference_model_against_transformers(tmp_path, dialect, strategy):
    """ChannelModel with act_quant=False (dequantised weights x fp16 activations) on the weights read_config / load_hf_weights make
    of the checkpoint, against a fp32 LlamaForCausalLM (eager attention) that holds the dequantised values"""
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    ck = r.write_checkpoint(str(tmp_path), dialect=dialect, strategy=strategy, seed=12)
    cfg, w, _ = _load(str(tmp_path))
    c = ck['config']
    hf = LlamaForCausalLM(LlamaConfig(hidden_size=c['hidden_size'], num_hidden_layers=c['num_hidden_layers'],
                                      num_attention_heads=c['num_attention_heads'], num_key_value_heads=c['num_key_value_heads'],
                                      head_dim=c['head_dim'], intermediate_size=c['intermediate_size'], vocab_size=c['vocab_size'],
                                      rms_norm_eps=c['rms_norm_eps'], rope_theta=c['rope_theta'], max_position_embeddings=512,
                                      tie_word_embeddings=False, attention_bias=False, mlp_bias=False, attn_implementation='eager'))
    sd = {}
    for k, v in ck.items():
        if k in ('dequant', 'config') or k.endswith(('.weight_scale', '.input_scale', '.k_scale', '.v_scale')):
            continue
        pre = k[:-len('.weight')]
        sd[k] = torch.from_numpy(np.asarray(ck['dequant'][pre] if pre in ck['dequant'] else v, f32))
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all('rotary' in m for m in missing), (missing, unexpected)
    hf = hf.float().eval()
    ids = np.random.default_rng(12).integers(0, c['vocab_size'], 20)
    with torch.no_grad():
        want = hf(torch.from_numpy(ids)[None]).logits[0].numpy()
    oc = r.oracle_config(ck, 16)
    om = r.ChannelModel(oc, w, batch=1, max_ctx=64, act_quant=False)
    om.forward([ids])
    got = o.lm_head(o.rmsnorm(om.last_resid, w['norm'], oc.rms_eps), w['output']).astype(f32)
    d = np.abs(got - want).max()
    print(f'{dialect} {strategy}: max |logit diff| {d:.5f} over |logits| up to {np.abs(want).max():.3f} (bound {HF_BOUND:.4f})')
    assert d <= HF_BOUND
    # the comparison notices a wrong mapping: the reference with gate and up swapped is far away
    for L in w['layers']:
        f8, cs = L['w1w3']['f8'].copy(), L['w1w3']['cs'].copy()
        L['w1w3'] = dict(f8=np.ascontiguousarray(f8.reshape(f8.shape[0], -1, 2)[:, :, ::-1].reshape(f8.shape)),
                         cs=np.ascontiguousarray(cs.reshape(-1, 2)[:, ::-1].reshape(-1)))
    om = r.ChannelModel(oc, w, batch=1, max_ctx=64, act_quant=False)
    om.forward([ids])
    bad = o.lm_head(o.rmsnorm(om.last_resid, w['norm'], oc.rms_eps), w['output']).astype(f32)
    assert np.abs(bad - want).max() > 4 * d
