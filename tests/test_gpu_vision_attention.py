"""tm_vision_attention (attention_vision.hip) against a float64 reference on the fp16-rounded inputs: rotate-half RoPE in float64,
softmax over the row's own segment, no mask tricks.  Bound 1e-2 |ref| + 2e-3, the project's bound for attention on random operands
(DESIGN 7.13, 7.14).  Segment lists: one key / one row; a ragged last 16-row tile; a ragged last 64-key stage and a two-stage double
buffer; segment boundaries inside what would be a shared tile; 600 segments of 4 (more workgroups than CUs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi, vl

pytestmark = pytest.mark.gpu
f16 = np.float16
SEGMENTS = [(1,), (15, 16, 17), (63, 64, 65), (129, 4, 200), (4,) * 600]


def _inputs(segs, heads, D, cs_f32, seed=0):
    """qkv fp16 [tokens, 3 heads D]; cos / sin as the tower makes them (fp32 [tokens, D], two copies side by side) or fp16 [tokens, D/2]"""
    rng = np.random.default_rng(seed)
    n = sum(segs)
    qkv = rng.standard_normal((n, 3 * heads * D)).astype(f16)
    ang = rng.uniform(0, 2 * np.pi, (n, D // 2))
    cos, sin = (np.cos(ang), np.sin(ang))
    if cs_f32:
        cos, sin = (np.concatenate([a, a], 1).astype(np.float32) for a in (cos, sin))
    else:
        cos, sin = cos.astype(f16), sin.astype(f16)
    return qkv, cos, sin, np.concatenate([[0], np.cumsum(segs)]).astype(np.int32)


def _reference(qkv, cos, sin, cu, heads, D):
    n = len(qkv)
    q, k, v = qkv.astype(np.float64).reshape(n, 3, heads, D).transpose(1, 2, 0, 3)       # [heads, n, D] each
    c, s = (np.concatenate([a[:, :D // 2]] * 2, 1).astype(np.float64) for a in (cos, sin))
    rot = lambda x: np.concatenate([-x[..., D // 2:], x[..., :D // 2]], -1)              # noqa: E731
    q, k = q * c + rot(q) * s, k * c + rot(k) * s
    out = np.zeros((n, heads, D))
    for b, e in zip(cu[:-1], cu[1:]):
        sc = q[:, b:e] @ k[:, b:e].transpose(0, 2, 1) / np.sqrt(D)
        p = np.exp(sc - sc.max(-1, keepdims=True))
        out[b:e] = ((p / p.sum(-1, keepdims=True)) @ v[:, b:e]).transpose(1, 0, 2)
    return out.reshape(n, heads * D)


def _run(qkv, cos, sin, cu, heads):
    out = vl.vision_attention(torch.from_numpy(qkv).cuda(), cu, torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda(), heads)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('segs', SEGMENTS, ids=lambda s: f'{len(s)}x{s[0]}' if len(s) > 3 else '-'.join(map(str, s)))
@pytest.mark.parametrize('heads', [1, 3])
@pytest.mark.parametrize('D', [64, 80, 128])
def test_against_float64(D, heads, segs):
    qkv, cos, sin, cu = _inputs(segs, heads, D, cs_f32=heads == 1)
    ref = _reference(qkv, cos, sin, cu, heads, D)
    got = _run(qkv, cos, sin, cu, heads).astype(np.float64)
    excess = np.abs(got - ref) - (1e-2 * np.abs(ref) + 2e-3)
    print(f'D {D} heads {heads} segments {segs[:3]}: max |err| {np.abs(got - ref).max():.2e}, worst err - bound {excess.max():.2e}')
    assert np.isfinite(got).all() and excess.max() <= 0


@pytest.mark.parametrize('D', [64, 80, 128])
def test_poisoned_segment_does_not_leak(D):
    """NaN in every token of the middle segment (qkv, cos and sin): its neighbours, whose ragged last stage and last rows border on
    it, must give the bits of a batch that never held it"""
    segs, heads = (70, 33, 130), 2
    qkv, cos, sin, cu = _inputs(segs, heads, D, cs_f32=True, seed=1)
    keep = np.r_[0:70, 103:233]
    want = _run(qkv[keep], cos[keep], sin[keep], np.array([0, 70, 200], np.int32), heads)
    for a in (qkv, cos, sin):
        a[70:103] = np.nan
    got = _run(qkv, cos, sin, cu, heads)
    assert np.isnan(got[70:103]).all() and np.isfinite(want).all()
    assert np.array_equal(got[keep].view(np.uint16), want.view(np.uint16))


def test_refusals_name_their_reason():
    tm = _ffi.load()
    z = torch.zeros((8, 3 * 128), dtype=torch.float16, device='cuda')
    cs = torch.zeros((8, 64), dtype=torch.float32, device='cuda')
    cu_dev, work = torch.tensor([0, 8], dtype=torch.int32, device='cuda'), torch.zeros((1, 2), dtype=torch.int32, device='cuda')

    def call(cu_host, heads, D, stride):
        host = np.asarray(cu_host, np.int32)
        return tm.tm_vision_attention(z.data_ptr(), z.data_ptr(), stride, cu_dev.data_ptr(), host.ctypes.data_as(C.POINTER(C.c_int)),
                                      len(host) - 1, work.data_ptr(), 1, 8, heads, D, cs.data_ptr(), cs.data_ptr(), 64, 1, 0.0, None)
    for args, needle in [(([0, 8], 1, 96, 384), 'head_dim'), (([0, 6, 4, 8], 1, 128, 384), 'never decrease'),
                         (([0, 8], 2, 128, 384), 'qkv row stride')]:
        assert call(*args) == 1 and needle in _ffi.last_error(), (args, _ffi.last_error())
    with pytest.raises(_ffi.TmError, match='head_dim must be 64, 80 or 128'):
        vl.vision_attention(torch.zeros((8, 3 * 96), dtype=torch.float16, device='cuda'), [0, 8], cs, cs, 1)
