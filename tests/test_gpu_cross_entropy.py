"""GPU parity of the per-row cross-entropy operator (tm_cross_entropy, cross_entropy.hip) against a float64 numpy restatement of the
reference's formula (kernels/cross_entropy_kernels.cu:31-73):  nll = log(sum exp(x - max) + 1e-9f) + max - x[target], max starting
at -FLT_MAX, from the fp16 logits.  Shapes: the reference's test_cross_entropy.cu cases plus the vocabularies served here (Llama-3
128 256, Qwen 151 936 on a padded 152 064 stride), an unaligned vocabulary / stride and a misaligned base.

Bound: |got - ref| <= 5e-5 + 1e-5 |ref| -- fp32 exponentials and sums against float64 (a first estimate; the worst case is printed)."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16 = np.float16
FLT_MAX = float(np.finfo(np.float32).max)
EPS = float(np.float32(1e-9))


def ref_nll(x16, tgt, V):
    """float64 restatement; target < 0 -> 0, target >= V -> NaN"""
    out = np.zeros(len(tgt), np.float64)
    with np.errstate(all='ignore'):
        for r, t in enumerate(tgt):
            if t < 0:
                continue
            if t >= V:
                out[r] = np.nan
                continue
            x = x16[r, :V].astype(np.float64)
            m = max(-FLT_MAX, float(np.max(x)))
            s = float(np.sum(np.exp(x - m)))
            out[r] = np.log(s + EPS) + m - x[t]
    return out


def run(tm, logits, tgt, rows, V, ld, offset=0, nll=None):
    """logits: fp16 [rows][ld] (flat buffer, `offset` halves in front of row 0)"""
    buf = dev(logits.reshape(-1))
    t = dev(np.asarray(tgt, np.int32))
    out = nll if nll is not None else torch.full((max(rows, 1),), -7.0, dtype=torch.float32, device='cuda')
    _ffi.check(tm.tm_cross_entropy(out.data_ptr(), buf.data_ptr() + 2 * offset, t.data_ptr(), rows, V, ld, st()))
    torch.cuda.synchronize()
    return host(out)[:rows]


def check(got, ref, what):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), what
    d = np.abs(got[fin].astype(np.float64) - ref[fin])
    bound = 5e-5 + 1e-5 * np.abs(ref[fin])
    worst = float(np.max(d / bound)) if d.size else 0.0
    print(f'{what}: max |d| {d.max() if d.size else 0:.3e}, worst d / bound {worst:.3f}')
    assert np.all(d <= bound), what


@pytest.mark.parametrize('rows,V,ld', [(1, 4, 4), (7, 1001, 1001), (3, 1001, 1008), (300, 32000, 32000), (64, 151936, 152064),
                                       (2048, 32000, 32000), (16, 128256, 128256)])
def test_cross_entropy_matches_reference(tm, cuda, rows, V, ld):
    rng = np.random.default_rng(rows * 7 + V)
    x = (rng.standard_normal((rows, ld)) * 3).astype(f16)
    x[:, V:] = f16(60000.0)                              # padding columns are never read
    tgt = rng.integers(0, V, rows).astype(np.int32)
    got = run(tm, x, tgt, rows, V, ld)
    check(got, ref_nll(x, tgt, V), f'rows {rows} V {V} ld {ld}')
    again = run(tm, x, tgt, rows, V, ld)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))     # fixed reduction order: bitwise reproducible


def test_cross_entropy_misaligned_base(tm, cuda):
    """a row base that is not 16-byte aligned takes the scalar path"""
    rng = np.random.default_rng(5)
    rows, V = 5, 4096
    flat = (rng.standard_normal(rows * V + 8) * 2).astype(f16)
    tgt = rng.integers(0, V, rows).astype(np.int32)
    got = run(tm, flat, tgt, rows, V, V, offset=1)
    check(got, ref_nll(flat[1:1 + rows * V].reshape(rows, V), tgt, V), 'misaligned base')


def test_cross_entropy_rows_zero_is_noop(tm, cuda):
    out = torch.full((4,), 3.5, dtype=torch.float32, device='cuda')
    x = np.zeros((1, 64), f16)
    run(tm, x, [0], 0, 64, 64, nll=out)
    assert np.all(host(out) == 3.5)


def test_cross_entropy_special_rows(tm, cuda):
    V = 32000
    rng = np.random.default_rng(11)
    x = rng.standard_normal((12, V)).astype(f16)
    tgt = rng.integers(0, V, 12).astype(np.int32)
    x[0] = f16(1.5)                                      # all equal -> log V
    x[1, tgt[1]] = f16(60.0)                             # target spike -> ~0
    x[2, (tgt[2] + 1) % V] = f16(60.0)                   # non-target spike -> ~60
    x[3, ::3] = -np.inf                                  # -inf entries (target on a finite one)
    tgt[3] = 1
    x[4] = -np.inf                                       # all -inf -> +inf
    x[5, 7] = -np.inf                                    # target on a -inf entry -> +inf
    tgt[5] = 7
    tgt[6] = 0
    tgt[7] = V - 1
    x[8] = np.nan                                        # target -1 on a NaN row: 0, the row is not read
    tgt[8] = -1
    tgt[9] = V                                           # target out of range -> NaN
    x[10, 123] = np.nan                                  # a NaN logit poisons the row
    x[11, :V // 2] = f16(-65504.0)                       # the most negative finite fp16 half the row
    got = run(tm, x, tgt, 12, V, V)
    ref = ref_nll(x, tgt, V)
    ref[10] = np.nan
    assert abs(got[0] - np.log(V)) <= 5e-5 + 1e-5 * np.log(V)
    assert abs(got[1]) <= 1e-4 and abs(got[2] - ref[2]) <= 1e-3 and got[2] > 50
    assert got[4] == np.inf and got[5] == np.inf
    assert got[8] == 0.0 and np.isnan(got[9]) and np.isnan(got[10])
    check(got, ref, 'special rows')
