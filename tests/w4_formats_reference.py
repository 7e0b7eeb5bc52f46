"""One set of u4 linears (q, s, z) written as an AWQ, a GPTQ and a compressed-tensors `pack-quantized` checkpoint, for the W4A16 dialect
tests.  The packing is numpy written from the layouts (not the loader's unpack functions run backwards):

  AWQ                  .qweight int32 [K][N/8] (nibble AWQ_ORDER[p] of word c = column 8c+p), .scales fp16 [K/g][N], .qzeros [K/g][N/8] alike
  GPTQ                 .qweight int32 [K/8][N] (nibble i of word r = row 8r+i), .scales fp16 [K/g][N], .qzeros int32 [K/g][N/8] (nibble j of
                       word c = column 8c+j) holding zero - 1 (v1) or the zero (gptq_v2), .g_idx int32 [K] = k // g
  compressed-tensors   .weight_packed int32 [N][K/8] (nibble j of word c = input channel 8c+j), .weight_scale fp16 / bf16 [N][K/g],
                       .weight_zero_point int32 [N/8][K/g] (nibble i of word r = output channel 8r+i; asymmetric only), .weight_shape [N, K]

The tensors and config files build on the writers of qwen_reference / qwen_moe_reference; a 'llama' kind is the Qwen tensor set without bias
and q / k norms under LlamaForCausalLM.
"""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import tm_oracle as o
from tests.qwen_moe_reference import hf_qwen_moe_tensors, qwen_moe_config_json
from tests.qwen_reference import hf_qwen_tensors, write_qwen_checkpoint

f16 = np.float16
DIALECTS = ('awq', 'gptq', 'compressed-tensors')


def pack_nibbles_last(q: np.ndarray) -> np.ndarray:
    """uint8 [..., 8C] -> int32 [..., C]: nibble j of word c = element 8c+j"""
    q = np.asarray(q, np.uint8)
    g = q.reshape(*q.shape[:-1], -1, 8).astype(np.uint64)
    w = np.zeros(g.shape[:-1], np.uint64)
    for j in range(8):
        w += g[..., j] * np.uint64(16 ** j)
    return w.astype(np.uint32).view(np.int32)


def pack_nibbles_rows(q: np.ndarray) -> np.ndarray:
    """uint8 [8R, N] -> int32 [R, N]: nibble i of word row r = row 8r+i"""
    q = np.asarray(q, np.uint8)
    g = q.reshape(-1, 8, q.shape[-1]).astype(np.uint64)
    w = np.zeros((g.shape[0], g.shape[2]), np.uint64)
    for i in range(8):
        w += g[:, i, :] * np.uint64(16 ** i)
    return w.astype(np.uint32).view(np.int32)


def quantize(w_kn: np.ndarray, group: int, symmetric: bool = False):
    """fp16 [K, N] -> (q uint8 [K, N], s fp16 [K/g, N], z uint8 [K/g, N]).  Asymmetric: the oracle's group-wise quantiser with the zero
    kept in [1, 15], so that GPTQ's v1 form (zero - 1 in a nibble) can hold it.  Symmetric: zero 8, scale = absmax / 7."""
    K, N = w_kn.shape
    if symmetric:
        x = np.asarray(w_kn, np.float32).reshape(K // group, group, N)
        s = (np.maximum(np.abs(x).max(1), 1e-5) / 7).astype(f16)
        q = np.clip(np.rint(x / s.astype(np.float32)[:, None]) + 8, 0, 15).astype(np.uint8).reshape(K, N)
        return q, s, np.full(s.shape, 8, np.uint8)
    q, s, z, _ = o.quantize_groupwise_u4(w_kn, group)
    return q, s, np.maximum(z.astype(np.uint8), 1)


def linear_tensors(pre: str, q, s, z, dialect: str, *, gptq_v2: bool = False, g_idx: bool = True, symmetric: bool = False,
                   scale_dtype: str = 'float16') -> dict:
    """the torch tensors of one linear in `dialect`"""
    import torch
    K, N = q.shape
    g = K // s.shape[0]
    if dialect == 'awq':
        t = {'.qweight': o.pack_awq_gemm(q), '.qzeros': o.pack_awq_gemm(z), '.scales': s}
    elif dialect == 'gptq':
        t = {'.qweight': pack_nibbles_rows(q), '.qzeros': pack_nibbles_last((z - (0 if gptq_v2 else 1)).astype(np.uint8)), '.scales': s}
        if g_idx:
            t['.g_idx'] = (np.arange(K) // g).astype(np.int32)
    else:
        t = {'.weight_packed': pack_nibbles_last(np.ascontiguousarray(q.T)), '.weight_scale': np.ascontiguousarray(s.T),
             '.weight_shape': np.array([N, K], np.int64)}
        if not symmetric:
            t['.weight_zero_point'] = pack_nibbles_rows(np.ascontiguousarray(z.T))
    out = {pre + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in t.items()}
    if dialect == 'compressed-tensors' and scale_dtype == 'bfloat16':
        out[pre + '.weight_scale'] = out[pre + '.weight_scale'].to(torch.bfloat16)
    return out


def quant_config(dialect: str, group: int = 128, *, gptq_v2: bool = False, symmetric: bool = False) -> dict:
    if dialect == 'awq':
        return {'quant_method': 'awq', 'bits': 4, 'group_size': group, 'zero_point': True, 'version': 'gemm'}
    if dialect == 'gptq':
        c = {'quant_method': 'gptq', 'bits': 4, 'group_size': group, 'sym': True, 'desc_act': False, 'damp_percent': 0.01,
             'true_sequential': True}
        if gptq_v2:
            c['checkpoint_format'] = 'gptq_v2'
        return c
    return {'quant_method': 'compressed-tensors', 'format': 'pack-quantized', 'quantization_status': 'compressed',
            'config_groups': {'group_0': {'targets': ['Linear'], 'input_activations': None, 'output_activations': None,
                                          'weights': {'num_bits': 4, 'type': 'int', 'symmetric': symmetric, 'strategy': 'group',
                                                      'group_size': group, 'dynamic': False, 'actorder': None,
                                                      'block_structure': None, 'observer': 'minmax'}}},
            'ignore': ['lm_head'], 'kv_cache_scheme': None}


GEOMETRY = dict(H=256, Hq=4, Hkv=2, I=512, V=512, layers=2)       # dense kinds; tp = 2 shards every axis into multiples of 128
MOE_GEOMETRY = dict(H=256, Hq=4, Hkv=2, I=256, E=4, k=2, V=512, layers=1)


def make_model(kind: str, group: int = 128, seed: int = 0, symmetric: bool = False, D: int = 128) -> dict:
    """kind 'llama' | 'qwen2' | 'qwen3' | 'qwen3_moe' -> {'kind', 'hf': fp16 HF tensors, 'quant': {linear prefix: (q, s, z)}, 'group'}:
    every *_proj quantised once, to be written in any dialect"""
    rng = np.random.default_rng(seed)
    if kind == 'qwen3_moe':
        hf = hf_qwen_moe_tensors(rng, **{k: v for k, v in MOE_GEOMETRY.items() if k != 'k'})
    else:
        hf = hf_qwen_tensors(rng, kind, **GEOMETRY, D=D, bias=(kind == 'qwen2'))
        if kind == 'llama':
            hf = {k: v for k, v in hf.items() if not k.endswith(('q_norm.weight', 'k_norm.weight'))}
    quant = {k[:-len('.weight')]: quantize(np.ascontiguousarray(v.T), group, symmetric) for k, v in hf.items() if k.endswith('_proj.weight')}
    return dict(kind=kind, hf=hf, quant=quant, group=group, symmetric=symmetric, D=D)


def write_model(path: str, model: dict, dialect: str, **opts) -> None:
    """the model of make_model as a checkpoint directory in `dialect` (opts: gptq_v2, g_idx, scale_dtype)"""
    import torch
    from safetensors.torch import save_file
    kind, hf, quant, group = model['kind'], model['hf'], model['quant'], model['group']
    cfg_opts = dict(gptq_v2=opts.get('gptq_v2', False), symmetric=model['symmetric'])
    if kind == 'qwen3_moe':
        c = qwen_moe_config_json(**MOE_GEOMETRY, fmt='hf')
    else:
        g = GEOMETRY
        write_qwen_checkpoint(path, 'qwen3' if kind == 'qwen3' else 'qwen2', {}, g['H'], g['Hq'], g['Hkv'], g['I'], g['V'], g['layers'])
        with open(os.path.join(path, 'config.json')) as f:
            c = json.load(f)
        c['head_dim'] = model['D']
        if kind == 'llama':
            c['architectures'] = ['LlamaForCausalLM']
    c['quantization_config'] = quant_config(dialect, group, **cfg_opts)
    tensors = {}
    for name, v in hf.items():
        pre = name[:-len('.weight')]
        if pre in quant:
            tensors.update(linear_tensors(pre, *quant[pre], dialect, symmetric=model['symmetric'],
                                          **{k: v_ for k, v_ in opts.items() if k in ('gptq_v2', 'g_idx', 'scale_dtype')}))
        else:
            tensors[name] = torch.from_numpy(v)
    save_file(tensors, os.path.join(path, 'model.safetensors'))
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)


def tm_linear(model: dict, pre: str) -> dict:
    q, s, z = model['quant'][pre]
    return dict(q=q, s=s, z=z.astype(f16))


def dense_oracle(model: dict, kv_bits: int = 8):
    """(oracle config, engine-layout weights) of a dense make_model (any kind), assembled from (q, s, z) directly -- not by checkpoint.py"""
    from tests.qwen_reference import QwenConfig, tm_weights_from_hf
    g = GEOMETRY
    cfg = QwenConfig(hidden=g['H'], layers=g['layers'], q_heads=g['Hq'], kv_heads=g['Hkv'], head_dim=model['D'], inter=g['I'], vocab=g['V'],
                     rms_eps=1e-6, rope=o.RopeParam(model['D'], 1e6), group=model['group'], kv_bits=kv_bits,
                     attn_bias=int(model['kind'] == 'qwen2'), qk_norm=int(model['kind'] == 'qwen3'))
    return cfg, tm_weights_from_hf(model['hf'], cfg, dict(model['quant']))
