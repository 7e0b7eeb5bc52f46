"""Host side of Multi-head Latent Attention: the absorbed projections of lmdeploy_amd.mla and the sizes the C-ABI reports."""
import numpy as np
import pytest

from lmdeploy_amd import _ffi, mla


def test_absorb_reproduces_the_expanded_scores_and_values():
    """q_nope . k_nope = (q_nope W_UK) . c and p v = (p c) W_UV for k_nope | v = kv_b_proj(c), head by head"""
    rng = np.random.default_rng(0)
    H, nope, vd = 3, 8, 5
    w = rng.standard_normal((H * (nope + vd), 512))
    c, q = rng.standard_normal(512), rng.standard_normal((H, nope))
    kv = (w @ c).reshape(H, nope + vd)
    W_UK, W_UV = mla.absorb(w, H, nope, vd)
    assert W_UK.shape == (H, nope, 512) and W_UV.shape == (H, 512, vd) and W_UV.flags['C_CONTIGUOUS']
    assert np.allclose(np.einsum('hd,hdr->hr', q, W_UK) @ c, (q * kv[:, :nope]).sum(-1), rtol=1e-12)
    assert np.allclose(np.einsum('r,hrv->hv', c, W_UV), kv[:, nope:], rtol=1e-12)
    with pytest.raises(ValueError, match='kv_lora_rank 512'):
        mla.absorb(w[:, :256], H, nope, vd)


def test_sizes_and_split_rule():
    tm = _ffi.load()
    assert tm.tm_mla_layer_size(64, 512, 64) == 64 * 576 * 2 and tm.tm_mla_layer_size(64, 512, 128) == -1
    assert tm.tm_mla_attention_workspace(7, 16, 1) == 0 and tm.tm_mla_attention_workspace(7, 16, 4) == 7 * 16 * 4 * 514 * 4
    assert mla.default_splits(64, 1, 16, 4096) == 8 and mla.default_splits(64, 1, 128, 4096) == 1
    assert mla.default_splits(1, 1, 16, 64) == 1 and mla.default_splits(1, 1, 16, 1 << 20) == 128
