"""Multi-head Latent Attention (DeepSeek-V2 / V3 / R1, Kimi-K2, MiniCPM3) glue, kept thin: the two absorbed projections are torch
einsums, the cache store and the attention run on the library's kernels (csrc/attention_mla.hip: tm_mla_kv_store, tm_mla_attention).
This is the operator-level entry; an engine that serves these models replaces the einsums with its own GEMMs.

Absorbed form: with kv_b_proj = [W_UK | W_UV] per head, q_nope . k_nope = (q_nope W_UK) . c and sum_t p_t v_t = (sum_t p_t c_t) W_UV,
so attention runs on the cached latent c (512) | k_pe (64) alone: one 1152-byte row per token, shared by every head.
"""
from __future__ import annotations

RANK, ROPE = 512, 64          # kv_lora_rank, qk_rope_head_dim: the one geometry the kernels are built for
ROW = RANK + ROPE
TARGET_WORKGROUPS = 512       # two workgroups per CU on 256 CUs (the attention kernel's LDS budget)


def absorb(kv_b_proj_weight, H: int, nope: int, v_dim: int):
    """kv_b_proj.weight [H * (nope + v_dim), 512] (numpy or torch) -> (W_UK [H, nope, 512], W_UV [H, 512, v_dim]):
    q_lat[h] = q_nope[h] @ W_UK[h] and out[h] = o_lat[h] @ W_UV[h]."""
    w = kv_b_proj_weight
    if tuple(w.shape) != (H * (nope + v_dim), RANK):
        raise ValueError(f'kv_b_proj.weight has shape {tuple(w.shape)}, expected {(H * (nope + v_dim), RANK)} '
                         f'(kv_lora_rank {RANK} only)')
    w = w.reshape(H, nope + v_dim, RANK)
    w_uk, w_uv = w[:, :nope, :], w[:, nope:, :].swapaxes(1, 2)
    if hasattr(w_uk, 'contiguous'):
        return w_uk.contiguous(), w_uv.contiguous()
    import numpy as np
    return np.ascontiguousarray(w_uk), np.ascontiguousarray(w_uv)


def default_splits(batch: int, max_q_len: int, H: int, max_k_len: int) -> int:
    """Split-K count that brings batch x chunks x splits to two workgroups per CU, with at least two 64-token tiles per split."""
    chunks = -(-max_q_len * H // 16)
    tiles = -(-max_k_len // 64)
    want = -(-TARGET_WORKGROUPS // max(1, batch * chunks))
    return max(1, min(want, tiles // 2, 128))


def mla_forward(q_nope, q_pe, kv_a, norm_w, W_UK, W_UV, cache, cu_q_len, k_len, softmax_scale: float, cos_sin=None,
                eps: float = 1e-6, splits: int | None = None):
    """One MLA attention forward on the GPU: einsum -> store -> attention -> einsum.

    q_nope fp16 [T, H, nope], q_pe fp16 [T, H, 64] (unrotated), kv_a fp16 [T, 576] (kv_a_proj_with_mqa's output), norm_w fp16 [512]
    (kv_a_layernorm), W_UK / W_UV from absorb(), cache: _ffi.KvCache view of the latent cache (kv_heads 1, head_dim 576, bits 16),
    cu_q_len int32 [B + 1] and k_len int32 [B] device tensors (k_len counts every row of this forward), cos_sin fp16 [max_pos, 32, 2]
    device table or None.  Returns fp16 [T, H, v_dim].  The rows' latent is written to the cache."""
    import torch

    from . import _ffi
    tm = _ffi.load()
    T, H, _ = q_nope.shape
    B = k_len.numel()
    q = torch.empty((T, H, ROW), dtype=torch.float16, device=q_nope.device)
    q[:, :, :RANK].copy_(torch.einsum('thd,hdr->thr', q_nope, W_UK))
    q[:, :, RANK:].copy_(q_pe)
    kv_a = kv_a.contiguous()
    st = torch.cuda.current_stream().cuda_stream
    _ffi.check(tm.tm_mla_kv_store(kv_a.data_ptr(), kv_a.shape[1], norm_w.data_ptr(), eps, q.data_ptr(), H * ROW, H, cu_q_len.data_ptr(),
                                  k_len.data_ptr(), B, T, None if cos_sin is None else cos_sin.data_ptr(),
                                  0 if cos_sin is None else cos_sin.shape[0], cache, st))
    if splits is None:
        ql = (cu_q_len[1:] - cu_q_len[:-1]).max().item()
        splits = default_splits(B, int(ql), H, int(k_len.max().item()))
    ws = torch.empty(max(1, tm.tm_mla_attention_workspace(T, H, splits)), dtype=torch.uint8, device=q.device)
    o_lat = torch.empty((T, H, RANK), dtype=torch.float16, device=q.device)
    _ffi.check(tm.tm_mla_attention(o_lat.data_ptr(), q.data_ptr(), H * ROW, cu_q_len.data_ptr(), k_len.data_ptr(), B, H, softmax_scale,
                                   splits, ws.data_ptr(), cache, st))
    return torch.einsum('thr,hrv->thv', o_lat, W_UV)
