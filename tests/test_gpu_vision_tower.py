"""Qwen2VLVision(device='cuda', attention='hip') against the torch tower on tiny random Qwen2-VL / Qwen2.5-VL vision configs
(depth 2, embed 160 = 2 heads of 80; 2.5-VL: block 0 full attention, block 1 windows of 8 x 8 patches): two images of different
grids and one whose grid is not a whole number of windows.  The bound is measured, not fixed: d_torch = max |torch fp16 - fp32| on
these inputs is the reference path's own distance, and the HIP path must stay within 2 d_torch (a different but equally valid summation
order) + one fp16 ulp of the largest feature."""
import json
import os

import numpy as np
import pytest
import torch

from lmdeploy_amd import vl

pytestmark = pytest.mark.gpu
IMAGE, GRIDS = 5, [[1, 16, 16], [1, 8, 24], [1, 12, 20]]
VISION = dict(depth=2, num_heads=2, patch_size=14, spatial_merge_size=2, temporal_patch_size=2, in_channels=3)


def _checkpoint(path, arch):
    """config.json + the tower's fp16 weights under visual.; q / k projections scaled by 8 so that the attention is not uniform"""
    from safetensors.torch import save_file
    text = dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1, intermediate_size=64, vocab_size=32,
                bos_token_id=None, eos_token_id=None)
    if arch == 'Qwen2VLForConditionalGeneration':
        from transformers import Qwen2VLConfig as Config
        from transformers.models.qwen2_vl.modeling_qwen2_vl import Qwen2VisionTransformerPretrainedModel as Tower
        vision = dict(VISION, embed_dim=160, hidden_size=64, mlp_ratio=2)
    else:
        from transformers import Qwen2_5_VLConfig as Config
        from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VisionTransformerPretrainedModel as Tower
        vision = dict(VISION, hidden_size=160, out_hidden_size=64, intermediate_size=320, fullatt_block_indexes=[0], window_size=112)
    cfg = Config(text_config=text, vision_config=vision, image_token_id=IMAGE)
    torch.manual_seed(0)
    tower = Tower(cfg.vision_config)
    with torch.no_grad():
        for name, p in tower.named_parameters():
            if name.endswith('.bias'):
                p.normal_(0.0, 0.1)
            if '.attn.qkv.' in name:
                p[:320] *= 8.0
    save_file({'visual.' + k: v.half().contiguous() for k, v in tower.state_dict().items()}, os.path.join(path, 'model.safetensors'))
    c = json.loads(cfg.to_json_string())
    c['architectures'] = [arch]
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)
    return str(path)


@pytest.mark.parametrize('arch', ['Qwen2VLForConditionalGeneration', 'Qwen2_5_VLForConditionalGeneration'])
def test_hip_tower_matches_torch_tower(tmp_path, arch):
    pytest.importorskip('transformers.models.' + ('qwen2_vl' if arch.startswith('Qwen2VL') else 'qwen2_5_vl'))
    path = _checkpoint(tmp_path, arch)
    pv = np.random.default_rng(3).standard_normal((sum(t * h * w for t, h, w in GRIDS), 3 * 2 * 14 * 14)).astype(np.float32)
    hip = vl.Qwen2VLVision(path, 'cuda', attention='hip')
    ref16 = vl.Qwen2VLVision(path, 'cuda', attention='torch')
    ref32 = vl.Qwen2VLVision(path, 'cuda', dtype=torch.float32)
    f_hip, f_16, f_32 = (t.features(pv, GRIDS).astype(np.float64) for t in (hip, ref16, ref32))
    d_torch, d_hip = np.abs(f_16 - f_32).max(), np.abs(f_hip - f_32).max()
    ulp = float(np.spacing(np.float16(np.abs(f_32).max())))
    print(f'{arch}: max |feature| {np.abs(f_32).max():.3f}, |torch fp16 - fp32| {d_torch:.3e}, |hip - fp32| {d_hip:.3e}, ulp {ulp:.3e}')
    assert f_hip.shape == f_32.shape == (sum(t * h * w for t, h, w in GRIDS) // 4, 64) and np.isfinite(f_hip).all()
    assert d_hip <= 2 * d_torch + ulp
    ids = [1, 2]
    for t, h, w in GRIDS:
        ids += [3] + [IMAGE] * (t * h * w // 4) + [4, 7]
    a, b = hip.prompt(ids, pv, GRIDS), ref16.prompt(ids, pv, GRIDS)
    assert a['input_embedding_ranges'] == b['input_embedding_ranges'] and a['mrope_position_delta'] == b['mrope_position_delta']
    assert np.array_equal(a['mrope_position_ids'], b['mrope_position_ids']) and np.array_equal(a['input_ids'], b['input_ids'])
    assert [e.shape for e in a['input_embeddings']] == [e.shape for e in b['input_embeddings']]
