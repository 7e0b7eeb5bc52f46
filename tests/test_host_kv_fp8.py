"""quant_policy 16 (FP8 KV cache): the reader returns a written checkpoint's k_scale / v_scale, 1.0 where a layer carries none."""
import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from lmdeploy_amd import TurbomindEngineConfig
from lmdeploy_amd.turbomind import checkpoint


def test_reader_returns_kv_scales(tmp_path):
    save_file({checkpoint.KV_SCALES['k'].format(i=0): torch.tensor(0.37), checkpoint.KV_SCALES['v'].format(i=0): torch.tensor([2.9]),
               checkpoint.KV_SCALES['k'].format(i=2): torch.tensor(0.5, dtype=torch.bfloat16)}, str(tmp_path / 'model.safetensors'))
    k, v = checkpoint.read_kv_scales(str(tmp_path), 3)
    assert k.dtype == np.float32 and k.tolist() == [np.float32(0.37), 1.0, 0.5] and v.tolist() == [np.float32(2.9), 1.0, 1.0]


def test_config_refuses_e5m2():
    with pytest.raises(AssertionError, match='FP8'):
        TurbomindEngineConfig(quant_policy=17)
