"""Plain reference of the FP8 KV cache (quant_policy 16; include/tm_mi355x.h, TM_KV_BITS_FP8), torch on the CPU: store
e4m3fn(clamp(f32(x) / scale, -448, 448)), flatten f16(f32(code) * scale), decode over f64(code) * scale.  Block layout: per kv head
K rows [block_len][head_dim] bytes, then V rows; no per-token parameters."""
from dataclasses import dataclass

import numpy as np
import torch

from lmdeploy_amd import _ffi


@dataclass
class Fp8Layout:   # what tests.gpu_helpers.DevCache reads of a layout, for the FP8 tag
    layers: int
    kv_heads: int
    head_dim: int = 128
    block_len: int = 64
    bits: int = _ffi.KV_BITS_FP8

    @property
    def layer_size(self):
        return self.kv_heads * 2 * self.block_len * self.head_dim

    @property
    def block_size(self):
        return self.layers * self.layer_size

    def k_data(self, layer, head, ti):
        return layer * self.layer_size + (head * 2 * self.block_len + ti) * self.head_dim

    def v_data(self, layer, head, ti):
        return self.k_data(layer, head, ti) + self.block_len * self.head_dim


def quantise(x: np.ndarray, scale: float) -> np.ndarray:   # fp16 [...] -> e4m3fn codes uint8 [...]
    y = torch.clamp(torch.from_numpy(np.asarray(x, np.float16)).float() / torch.tensor(scale, dtype=torch.float32), -448.0, 448.0)
    return y.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def dequantise(codes: np.ndarray, scale: float, dtype=np.float64) -> np.ndarray:
    """float64: exact f64(code) * f64(f32(scale)); float16: the flatten form f16(f32(code) * scale)"""
    c = torch.from_numpy(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn).float()
    if dtype == np.float16:
        return (c * torch.tensor(scale, dtype=torch.float32)).half().numpy()
    return c.double().numpy() * np.float64(np.float32(scale))


def store(pool: np.ndarray, L: Fp8Layout, table, layer: int, t0: int, k: np.ndarray, v: np.ndarray, k_scale: float, v_scale: float):
    # k (roped) / v fp16 [T, kv_heads, D] at positions t0 .. into pool [blocks, block_size] uint8 -> K, V codes [kv_heads, T, D]
    kc, vc = quantise(k, k_scale), quantise(v, v_scale)
    for i in range(k.shape[0]):
        blk, ti = int(table[(t0 + i) // 64]), (t0 + i) % 64
        for hd in range(L.kv_heads):
            a, b = L.k_data(layer, hd, ti), L.v_data(layer, hd, ti)
            pool[blk, a:a + L.head_dim] = kc[i, hd]
            pool[blk, b:b + L.head_dim] = vc[i, hd]
    return kc.transpose(1, 0, 2), vc.transpose(1, 0, 2)


def view(dc, layer: int, k_scale: float, v_scale: float) -> _ffi.KvCache:   # DevCache.view leaves the scales 0 = 1.0
    c = dc.view(layer)
    c.k_scale, c.v_scale = k_scale, v_scale
    return c
