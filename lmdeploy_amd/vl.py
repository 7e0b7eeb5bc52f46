"""Vision-language glue for Qwen2-VL / Qwen2.5-VL, kept thin: the vision tower stays with PyTorch (as in the reference's
lmdeploy/vl), the engine runs the language model and takes what this module prepares -- the dict prompt of Pipeline
(input_ids, input_embeddings, input_embedding_ranges, mrope_position_ids, mrope_position_delta; the reference's names,
lmdeploy/turbomind/turbomind.py:632-674).  Images only: image preprocessing, chat templates and video are out of scope.
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


class Qwen2VLVision:
    """The vision tower of a Qwen2-VL / Qwen2.5-VL checkpoint, loaded alone through the installed transformers (the language
    weights are never materialised here: the engine holds them)."""

    def __init__(self, model_path: str, device: str = 'cpu', dtype=None):
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

    def features(self, pixel_values, image_grid_thw):
        """merged image features, one row per image token: float16 numpy [sum of T * (H / m) * (W / m), hidden]"""
        import torch
        grid = torch.as_tensor(np.asarray(image_grid_thw)).reshape(-1, 3).to(self.device)
        pv = torch.as_tensor(pixel_values).to(self.device, next(self.tower.parameters()).dtype)
        with torch.no_grad():
            out = self.tower(pv, grid_thw=grid)
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
