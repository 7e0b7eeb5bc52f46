"""Multi-head Latent Attention (DeepSeek-V2 / V3 / R1, Kimi-K2, MiniCPM3) glue, kept thin: the projections are torch einsums, the
cache store and the attention run on the library's kernels (csrc/attention_mla.hip: tm_mla_kv_store, tm_mla_attention;
csrc/attention_mla_prefill.hip: tm_mla_flatten, tm_mla_prefill_attention).
This is the operator-level entry; an engine that serves these models replaces the einsums with its own GEMMs.

Absorbed form: with kv_b_proj = [W_UK | W_UV] per head, q_nope . k_nope = (q_nope W_UK) . c and sum_t p_t v_t = (sum_t p_t c_t) W_UV,
so attention runs on the cached latent c (512) | k_pe (64) alone: one 1152-byte row per token, shared by every head.

Expanded form (prefill): the context's latent rows are gathered from the cache, k_nope = W_UK c and v = c W_UV are expanded per head
once per forward, and attention runs at qk width 192 / v width 128: 640 flop per (row, head, key) where the absorbed form spends 2176.
The cache rows are written by the same tm_mla_kv_store call in both forms.  Chunked prefill re-expands the history once per chunk.

FP8 latent cache: a view with bits = _ffi.KV_BITS_FP8 and k_scale = the layer's latent scale holds 640-byte rows, 512 e4m3fn codes of
c / k_scale then k_pe as fp16 (row_bytes(); the layer size is tm_mla_layer_size_fp8).  The same calls serve it -- the store quantises,
csrc/attention_mla_fp8.hip attends on the codes and flattens them to fp16 for the expanded form -- so mla_forward takes no new argument.
"""
from __future__ import annotations

RANK, ROPE = 512, 64          # kv_lora_rank, qk_rope_head_dim: the one geometry the kernels are built for
ROW = RANK + ROPE
TARGET_WORKGROUPS = 512       # two workgroups per CU on 256 CUs (the attention kernel's LDS budget)
NOPE, V_DIM = 128, 128        # qk_nope_head_dim, v_head_dim of the expanded form (tm_mla_prefill_attention)
FORMS = ('absorbed', 'expanded', 'auto')
# form='auto' takes the expanded form from this q_len on.  Measured (crossover tables): the summed expanded path first
# beats the absorbed call at q_len 256 (H 128) and 768 (H 16) behind 1024 cached tokens, and at 512 (H 128) and 1536 (H 16) with no
# history; the constant is the largest of the four, so 'auto' takes the expanded form in no measured row where it was the slower one
# (below the constant it stays absorbed, also where expanded would already win).  It is H = 16's 70 us of torch expansion einsums that
# sets it: an engine that expands with its own GEMM should measure again.
AUTO_EXPANDED_MIN_Q_LEN = 1536


def row_bytes(bits: int) -> int:
    """Bytes of one cached token for a latent view's `bits`: 16 -> 1152 (576 fp16), _ffi.KV_BITS_FP8 -> 640 (512 codes + 64 fp16)."""
    from . import _ffi
    if bits not in (16, _ffi.KV_BITS_FP8):
        raise ValueError(f'the MLA latent cache is bits 16 or KV_BITS_FP8 ({_ffi.KV_BITS_FP8}), got {bits}')
    return ROW * 2 if bits == 16 else RANK + ROPE * 2


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


def pick_form(form: str, max_q_len: int) -> str:
    """'absorbed' or 'expanded' for a forward whose longest sequence has max_q_len rows; any other `form` is refused by name."""
    if form not in FORMS:
        raise ValueError(f"mla_forward: form must be one of {FORMS}, got {form!r}")
    if form != 'auto':
        return form
    return 'expanded' if max_q_len >= AUTO_EXPANDED_MIN_Q_LEN else 'absorbed'


def _forward_expanded(tm, q_nope, q, W_UK, W_UV, cache, cu_q_len, k_len, max_q_len: int, softmax_scale: float, st):
    """flatten -> two einsums -> tm_mla_prefill_attention; q [T, H, 576] carries the ROTATED q_pe in its last 64 columns."""
    import torch

    from . import _ffi
    T, H, nope = q_nope.shape
    v_dim = W_UV.shape[2]
    if (nope, v_dim) != (NOPE, V_DIM):
        raise ValueError(f'mla_forward: the expanded form is built for qk_nope_head_dim {NOPE} and v_head_dim {V_DIM}, got {nope} / {v_dim}')
    B = k_len.numel()
    tokens, max_k = int(k_len.sum().item()), int(k_len.max().item())
    cu_k_off = (torch.cumsum(k_len, 0) - k_len).to(torch.int32)
    qx = torch.cat([q_nope, q[:, :, RANK:]], 2)                                   # q_nope | rotated q_pe: [T, H, 192]
    lat = torch.empty((max(1, tokens), ROW), dtype=torch.float16, device=q.device)
    _ffi.check(tm.tm_mla_flatten(lat.data_ptr(), cu_k_off.data_ptr(), k_len.data_ptr(), B, max_k, cache, st))
    kv = torch.empty((max(1, tokens), H, NOPE + V_DIM), dtype=torch.float16, device=q.device)
    c = lat[:tokens, :RANK]
    kv[:tokens, :, :NOPE].copy_(torch.einsum('tr,hdr->thd', c, W_UK))            # k_nope[t, h] = W_UK[h] c_t
    kv[:tokens, :, NOPE:].copy_(torch.einsum('tr,hrv->thv', c, W_UV))            # v[t, h] = c_t W_UV[h]
    out = torch.empty((T, H, V_DIM), dtype=torch.float16, device=q.device)
    _ffi.check(tm.tm_mla_prefill_attention(out.data_ptr(), qx.data_ptr(), H * (NOPE + ROPE), kv.data_ptr(), H * (NOPE + V_DIM),
                                           lat.data_ptr() + RANK * 2, ROW, cu_q_len.data_ptr(), cu_k_off.data_ptr(), k_len.data_ptr(), B,
                                           max_q_len, H, softmax_scale, st))
    return out


def mla_forward(q_nope, q_pe, kv_a, norm_w, W_UK, W_UV, cache, cu_q_len, k_len, softmax_scale: float, cos_sin=None,
                eps: float = 1e-6, splits: int | None = None, form: str = 'absorbed'):
    """One MLA attention forward on the GPU.  form 'absorbed' (the default): einsum -> store -> attention -> einsum.  form 'expanded':
    store -> flatten -> expansion einsums -> prefill attention at 192 / 128, for prompts (qk_nope 128, v 128 only; `splits` is unused).
    form 'auto': 'expanded' when the longest sequence of the forward has at least AUTO_EXPANDED_MIN_Q_LEN rows.  The cache rows written
    are the same bytes in every form.

    q_nope fp16 [T, H, nope], q_pe fp16 [T, H, 64] (unrotated), kv_a fp16 [T, 576] (kv_a_proj_with_mqa's output), norm_w fp16 [512]
    (kv_a_layernorm), W_UK / W_UV from absorb(), cache: _ffi.KvCache view of the latent cache (kv_heads 1, head_dim 576, bits 16 or KV_BITS_FP8 with k_scale),
    cu_q_len int32 [B + 1] and k_len int32 [B] device tensors (k_len counts every row of this forward), cos_sin fp16 [max_pos, 32, 2]
    device table or None.  Returns fp16 [T, H, v_dim].  The rows' latent is written to the cache."""
    pick_form(form, 0)  # an unknown form is refused before anything else happens
    import torch

    from . import _ffi
    tm = _ffi.load()
    T, H, _ = q_nope.shape
    B = k_len.numel()
    max_q_len = 0
    if form != 'absorbed':
        max_q_len = int((cu_q_len[1:] - cu_q_len[:-1]).max().item())
        form = pick_form(form, max_q_len)
    q = torch.empty((T, H, ROW), dtype=torch.float16, device=q_nope.device)
    if form == 'absorbed':  # the expanded form needs the q_pe columns only: the store touches nothing else of q
        q[:, :, :RANK].copy_(torch.einsum('thd,hdr->thr', q_nope, W_UK))
    q[:, :, RANK:].copy_(q_pe)
    kv_a = kv_a.contiguous()
    st = torch.cuda.current_stream().cuda_stream
    _ffi.check(tm.tm_mla_kv_store(kv_a.data_ptr(), kv_a.shape[1], norm_w.data_ptr(), eps, q.data_ptr(), H * ROW, H, cu_q_len.data_ptr(),
                                  k_len.data_ptr(), B, T, None if cos_sin is None else cos_sin.data_ptr(),
                                  0 if cos_sin is None else cos_sin.shape[0], cache, st))
    if form == 'expanded':
        return _forward_expanded(tm, q_nope, q, W_UK, W_UV, cache, cu_q_len, k_len, max_q_len, softmax_scale, st)
    if splits is None:
        ql = (cu_q_len[1:] - cu_q_len[:-1]).max().item()
        splits = default_splits(B, int(ql), H, int(k_len.max().item()))
    ws = torch.empty(max(1, tm.tm_mla_attention_workspace(T, H, splits)), dtype=torch.uint8, device=q.device)
    o_lat = torch.empty((T, H, RANK), dtype=torch.float16, device=q.device)
    _ffi.check(tm.tm_mla_attention(o_lat.data_ptr(), q.data_ptr(), H * ROW, cu_q_len.data_ptr(), k_len.data_ptr(), B, H, softmax_scale,
                                   splits, ws.data_ptr(), cache, st))
    return torch.einsum('thr,hrv->thv', o_lat, W_UV)
