"""Vision-language glue for Qwen2-VL / Qwen2.5-VL, kept thin: the vision tower stays with PyTorch (as in the reference's
lmdeploy/vl), the engine runs the language model and takes what this module prepares -- the dict prompt of Pipeline
(input_ids, input_embeddings, input_embedding_ranges, mrope_position_ids, mrope_position_delta; the reference's names,
lmdeploy/turbomind/turbomind.py:632-674).  Images only: image preprocessing, chat templates and video are out of scope.
With attention='hip' the tower's one non-GEMM operation, its bidirectional varlen attention with the 2-D rotary embedding, runs on
the library's MFMA kernel (vision_attention below; csrc/attention_vision.hip); linears, norms and activations stay torch modules.
"""
from __future__ import annotations

import numpy as np


def mrope_positions(input_ids, image_grid_thw, image_token_id: int, spatial_merge_size: int = 2, video_grid_thw=None):
    """M-RoPE coordinates of a prompt with images -> (ids int32 [3, n] = (t, h, w) per token, delta).

    A text run counts up on all three axes from the running maximum + 1.  Image k is a run of T * (H / m) * (W / m) image tokens for
    its grid (T, H, W) in patches and merge size m; with `start` = the running maximum + 1 its token (ti, row, column) sits at
    t = start + ti, h = start + row, w = start + column (ti = 0 for a still image), and the next start is the largest of them + 1.
    delta = largest coordinate + 1 - n: what a token behind the prompt adds to its linear position."""
    if video_grid_thw is not None and len(video_grid_thw):
        raise NotImplementedError('video_grid_thw: video inputs are not built (images only)')
    ids = np.asarray(input_ids).reshape(-1)
    grids = [tuple(int(v) for v in g) for g in (np.asarray(image_grid_thw).reshape(-1, 3) if image_grid_thw is not None else [])]
    n, m = len(ids), int(spatial_merge_size)
    out = np.zeros((3, n), np.int32)
    nxt, p, k = 0, 0, 0
    while p < n:
        if ids[p] != image_token_id:
            out[:, p] = nxt
            nxt += 1
            p += 1
            continue
        if k >= len(grids):
            raise ValueError(f'image token at position {p} but only {len(grids)} image grids')
        T, H, W = grids[k]
        if H % m or W % m:
            raise ValueError(f'image grid {grids[k]} is no multiple of the spatial merge size {m}')
        h, w = H // m, W // m
        cnt = T * h * w
        if p + cnt > n or np.any(ids[p:p + cnt] != image_token_id):
            raise ValueError(f'image {k} with grid {grids[k]} needs a run of {cnt} image tokens at position {p}')
        ti, row, col = np.meshgrid(np.arange(T), np.arange(h), np.arange(w), indexing='ij')
        out[0, p:p + cnt] = nxt + ti.reshape(-1)
        out[1, p:p + cnt] = nxt + row.reshape(-1)
        out[2, p:p + cnt] = nxt + col.reshape(-1)
        nxt += max(T, h, w)
        p += cnt
        k += 1
    if k != len(grids):
        raise ValueError(f'{len(grids)} image grids but {k} runs of image tokens')
    return out, int(nxt - n)


class VisionAttentionPlan:
    """What tm_vision_attention needs besides the activations, made once per cu_seqlens and shared by every block that runs on it:
    the int32 device cu_seqlens, its host copy and the device work list of (segment, 64-row query block), longest segments first.
    Building it reads cu_seqlens back when it is a device tensor (one synchronisation per forward and boundary list: segment lengths
    are host knowledge in the tower, they come from image_grid_thw)."""

    def __init__(self, cu_seqlens, device=None):
        import ctypes as C

        import torch

        from . import _ffi
        dev_in = cu_seqlens if isinstance(cu_seqlens, torch.Tensor) and cu_seqlens.is_cuda else None
        host = cu_seqlens.cpu().numpy() if isinstance(cu_seqlens, torch.Tensor) else np.asarray(cu_seqlens)
        host = np.ascontiguousarray(host.reshape(-1).astype(np.int32))
        if len(host) < 1:
            raise ValueError('cu_seqlens needs at least one entry')
        self.host, self.nseg = host, len(host) - 1
        device = dev_in.device if dev_in is not None else torch.device(device or 'cuda')
        keep = dev_in is not None and dev_in.dtype == torch.int32 and dev_in.is_contiguous()
        self.cu = dev_in if keep else torch.from_numpy(host).to(device)
        tm, hp = _ffi.load(), host.ctypes.data_as(C.POINTER(C.c_int))
        n = C.c_int(0)
        _ffi.check(tm.tm_vision_attention_plan(hp, self.nseg, None, 0, C.byref(n)))
        work = np.zeros((max(n.value, 1), 2), np.int32)
        _ffi.check(tm.tm_vision_attention_plan(hp, self.nseg, work.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
        self.n_work = n.value
        self.work = torch.from_numpy(work).to(device)


def vision_attention(qkv, cu_seqlens, cos, sin, heads: int, softmax_scale: float = 0.0, plan: VisionAttentionPlan = None):
    """tm_vision_attention on torch's current stream, no copies: qkv fp16 cuda [tokens, 3 * heads * D] (the fused qkv linear's output,
    rows may be strided), cos / sin fp16 or fp32 cuda [tokens, >= D / 2] (transformers' [tokens, D] = two copies side by side is
    read through its row stride) -> fp16 [tokens, heads * D].  Token i attends token j iff both lie in one segment of cu_seqlens."""
    import ctypes as C

    import torch

    from . import _ffi
    tokens, width = qkv.shape
    if qkv.dtype != torch.float16 or not qkv.is_cuda or qkv.stride(1) != 1:
        raise ValueError('vision_attention: qkv must be an fp16 cuda tensor with contiguous rows')
    if width % (3 * heads):
        raise ValueError(f'vision_attention: qkv rows of {width} are not 3 x {heads} heads')
    if cos.dtype != sin.dtype or cos.dtype not in (torch.float16, torch.float32):
        cos, sin = cos.float(), sin.float()
    if cos.stride(-1) != 1 or sin.stride() != cos.stride():
        cos, sin = cos.contiguous(), sin.contiguous()
    plan = plan or VisionAttentionPlan(cu_seqlens, qkv.device)
    out = torch.empty((tokens, width // 3), dtype=torch.float16, device=qkv.device)
    _ffi.check(_ffi.load().tm_vision_attention(
        out.data_ptr(), qkv.data_ptr(), qkv.stride(0), plan.cu.data_ptr(), plan.host.ctypes.data_as(C.POINTER(C.c_int)), plan.nseg,
        plan.work.data_ptr(), plan.n_work, tokens, heads, width // (3 * heads), cos.data_ptr(), sin.data_ptr(), cos.stride(0),
        int(cos.dtype == torch.float32), float(softmax_scale), _ffi.stream_ptr()))
    return out


class Qwen2VLVision:
    """The vision tower of a Qwen2-VL / Qwen2.5-VL checkpoint, loaded alone through the installed transformers (the language
    weights are never materialised here: the engine holds them).  attention='torch' (the default) leaves the tower as transformers
    built it; attention='hip' (device 'cuda', fp16 tower) sends every block's attention to tm_vision_attention: the block's own
    qkv linear, one kernel (RoPE on q and k, segment softmax, P V), the block's own proj.  The forward of the blocks' attention
    modules is replaced rather than registered as an attention interface: transformers' hook is called behind
    apply_rotary_pos_emb_vision with q / k / v already rotated, split and transposed -- a kernel fed from there would need the repack
    copies and the separate fp32 rotary passes this one exists to remove."""

    def __init__(self, model_path: str, device: str = 'cpu', dtype=None, attention: str = 'torch'):
        import json
        import os
        from glob import glob

        import torch
        from safetensors import safe_open
        from transformers import AutoConfig

        from .turbomind.checkpoint import QWEN_VL
        with open(os.path.join(model_path, 'config.json')) as f:
            arch = (json.load(f).get('architectures') or [''])[0]
        if arch not in QWEN_VL['archs']:
            raise NotImplementedError(f'architecture {arch}: the vision tower is loaded for Qwen2-VL and Qwen2.5-VL')
        cfg = AutoConfig.from_pretrained(model_path)
        if arch == 'Qwen2VLForConditionalGeneration':
            from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VisionTransformerPretrainedModel as Tower
        else:
            from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VisionTransformerPretrainedModel as Tower
        self.image_token_id = int(cfg.image_token_id)
        self.spatial_merge_size = int(cfg.vision_config.spatial_merge_size)
        tower = Tower(cfg.vision_config)
        state = {}
        for fn in sorted(glob(os.path.join(model_path, '*.safetensors'))):
            with safe_open(fn, framework='pt') as f:
                for k in f.keys():
                    for pfx in QWEN_VL['vision_prefixes']:
                        if k.startswith(pfx):
                            state[k[len(pfx):]] = f.get_tensor(k)
                            break
        tower.load_state_dict(state, strict=True)
        self.device = torch.device(device)
        self.tower = tower.to(self.device, dtype or next(iter(state.values())).dtype).eval()
        if attention not in ('torch', 'hip'):
            raise ValueError(f"attention={attention!r}: 'torch' or 'hip'")
        self.attention = attention
        self._plans = {}
        if attention == 'hip':
            if self.device.type != 'cuda' or next(self.tower.parameters()).dtype != torch.float16:
                raise ValueError("attention='hip' runs an fp16 tower on device='cuda' (there is no CPU form of the kernel)")
            for blk in self.tower.blocks:
                blk.attn.forward = self._hip_attention(blk.attn)

    def _hip_attention(self, attn):
        """forward of one block's attention module on the HIP kernel; cu_seqlens is whichever boundary list the block was handed
        (Qwen2.5-VL: cu_window_seqlens or cu_seqlens), its plan made once per features() call and list"""
        heads, scale = int(attn.num_heads), float(attn.scaling)

        def forward(hidden_states, cu_seqlens, position_embeddings=None, **kwargs):
            if position_embeddings is None:
                raise NotImplementedError("attention='hip' needs the (cos, sin) position_embeddings the tower passes to its blocks")
            key = (cu_seqlens.data_ptr(), cu_seqlens.numel())
            if key not in self._plans:      # the tensor is kept beside its plan: its address stays taken while the key lives
                self._plans[key] = (VisionAttentionPlan(cu_seqlens, hidden_states.device), cu_seqlens)
            cos, sin = position_embeddings
            return attn.proj(vision_attention(attn.qkv(hidden_states), cu_seqlens, cos, sin, heads, scale, self._plans[key][0]))
        return forward

    def features(self, pixel_values, image_grid_thw):
        """merged image features, one row per image token: float16 numpy [sum of T * (H / m) * (W / m), hidden]"""
        import torch
        grid = torch.as_tensor(np.asarray(image_grid_thw)).reshape(-1, 3).to(self.device)
        pv = torch.as_tensor(pixel_values).to(self.device, next(self.tower.parameters()).dtype)
        with torch.no_grad():
            out = self.tower(pv, grid_thw=grid)
        self._plans.clear()
        out = getattr(out, 'pooler_output', out)     # newer transformers return (last_hidden_state, pooler_output = merged rows)
        if isinstance(out, (list, tuple)):
            out = torch.cat(list(out))
        return out.float().cpu().numpy().astype(np.float16)

    def prompt(self, input_ids, pixel_values, image_grid_thw) -> dict:
        """the dict prompt Pipeline takes: every run of image tokens becomes an embedding range over its image's feature rows"""
        ids = np.asarray(input_ids, np.int32).reshape(-1)
        feats = self.features(pixel_values, image_grid_thw)
        pos, delta = mrope_positions(ids, image_grid_thw, self.image_token_id, self.spatial_merge_size)
        is_img = np.concatenate([[False], ids == self.image_token_id, [False]])
        edges = np.flatnonzero(is_img[1:] != is_img[:-1])
        ranges = [(int(b), int(e)) for b, e in zip(edges[0::2], edges[1::2])]
        if sum(e - b for b, e in ranges) != len(feats):
            raise ValueError(f'{len(feats)} image feature rows for {sum(e - b for b, e in ranges)} image tokens')
        embs, row = [], 0
        for b, e in ranges:
            embs.append(feats[row:row + e - b])
            row += e - b
        return dict(input_ids=ids, input_embeddings=embs, input_embedding_ranges=ranges, mrope_position_ids=pos,
                    mrope_position_delta=delta)
