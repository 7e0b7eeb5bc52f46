"""tm_decode_attention_window and tm_prefill_attention_window against operands whose softmax weights are exact powers of two and
whose weighted sums are exact in fp32 (tests/attention_exact_reference.py with a window and sinks; proved on the CPU by
tests/test_host_attention_window_exact.py): every correct order of computation returns the same bits, and the kernels are held to
those bits.  A mismatch is a window edge off by one, a skipped tile or step that held a visible token, a split that lost or doubled
its tiles, a sink left out, added twice, taken from another head or weighted against the wrong maximum -- never an
accumulation-order effect.

The window's first token and the newest token are live for every head, the token in front of the window looks live (in tier B with
the top weight).  q carries an offset channel that puts the live maximum at exponent 0 (tier A) or at a small integer (tier B: 3 for
the top weight), so a sink logit of +0 / -0 is a whole weight among the live ones; -inf and -65504 are weight 0.  Heads take
+0, -inf, -0, -65504 in turn: a sink from the neighbouring head is a unit of weight gained or lost.

All comparisons are equalities of uint16 views with -0 mapped to +0, but for the outputs the builder could not move away from an fp16
rounding boundary (at most 1 in 1000 per case, compared at 1 ulp; their worst distance is printed).  Outputs are pre-filled with
fp16 NaN; the cache pool outside the sequences' own rows, every block that lies wholly before a window included, and the split-KV
workspace with 0xFF; the workspace is allocated once per case and never cleared.  Block tables are shuffled.  In prefill the K rows
past a context and before the first row's window hold NaN.

Decode: one launch covers the contexts (1, 31, 33, 64, 65, 97, 129, 200, 330, 1089) under one window.  First token of the window /
number of 32-token tiles the kernel walks (fewer than the splits at 2, 3 or 16 splits wherever the count says so):

      n    W 1        W 32       W 33       W 64       W 100      W 4096
      1      0 /  1      0 /  1      0 /  1      0 /  1      0 /  1      0 /  1      W = n, W > n
     31     30 /  1      0 /  1      0 /  1      0 /  1      0 /  1      0 /  1
     33     32 /  1      1 /  2      0 /  2      0 /  2      0 /  2      0 /  2      first token 1; W = n
     64     63 /  1     32 /  1     31 /  2      0 /  2      0 /  2      0 /  2      31 mod 32; 0 mod 32; W = n
     65     64 /  1     33 /  2     32 /  2      1 /  3      0 /  3      0 /  3      block boundary; 1 mod 32; first token 1
     97     96 /  1     65 /  2     64 /  2     33 /  3      0 /  4      0 /  4      window inside the newest partial block
    129    128 /  1     97 /  2     96 /  2     65 /  3     29 /  5      0 /  5
    200    199 /  1    168 /  2    167 /  2    136 /  3    100 /  4      0 /  7
    330    329 /  1    298 /  2    297 /  2    266 /  3    230 /  4      0 / 11
   1089   1088 /  1   1057 /  2   1056 /  2   1025 /  3    989 /  5      0 / 35

Comparisons (case x kernel launch): decode 288 (6 (head_dim, KV width) x 6 windows x 2 tiers x 4 split counts; the six GQA groups
and sinks off / on rotate so that every (head_dim, KV width) meets each of them), prefill 54 (2 head_dims x 9 windows x 3 batches;
tiers, the five GQA groups and sinks rotate), negative controls 4 launches.

Configurations this module caught: none."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import attention_exact_reference as r
from tests.gpu_helpers import DevCache, dev, host, st

pytestmark = pytest.mark.gpu
f16 = np.float16
LAYER = 1
SPLITS = (1, 2, 3, 16)
DECODE = list(r.decode_window_cases())
PREFILL = list(r.prefill_window_cases())


def test_thinning_covers_every_axis():
    for D in (128, 64):
        for bits in (8, 4, 16):
            mine = [a for a in DECODE if (a[1], a[0]) == (D, bits)]
            assert {a[2] for a in mine} == set(r.GROUPS_WINDOW) == {1, 2, 3, 4, 7, 8}
            assert {(a[4], a[3]) for a in mine} == {(W, t) for W in (1, 32, 33, 64, 100, 4096) for t in 'AB'}
            assert {(a[4], a[5]) for a in mine} == {(W, k) for W in r.WINDOWS_DECODE for k in (0, 1)}
            assert {(a[3], a[5]) for a in mine} == {(t, k) for t in 'AB' for k in (0, 1)}
        mine = [a for a in PREFILL if a[0] == D]
        assert {a[1] for a in mine} == set(r.GROUPS_PREFILL)
        assert {(a[4], a[3]) for a in mine} == {(W, s) for W in (1, 16, 17, 32, 33, 64, 65, 100, 4096) for s in r.PREFILL_SHAPES}
        for W in r.WINDOWS_PREFILL:
            assert {a[2] for a in mine if a[4] == W} == {'A', 'B'} and {a[5] for a in mine if a[4] == W} == {0, 1}
    assert len(DECODE) * len(SPLITS) == 288 and len(PREFILL) == 54


def _tables(rng, klen, spare=2):
    nblk = [(k + 63) // 64 for k in klen]
    perm = rng.permutation(sum(nblk) + spare)                # shuffled block tables
    tables, off = [], 0
    for nb in nblk:
        tables.append(perm[off:off + nb])
        off += nb
    return tables, len(perm)


def _pool(case, L, tables, total, window):
    """0xFF everywhere (fp16 / (scale, zero) NaN: the other layer, the spare blocks, the blocks wholly before `window`), the
    sequences' rows and the look-alive rows behind them in LAYER"""
    pool = np.full((total, L.block_size), 0xFF, np.uint8)
    for s, tab in zip(case.seqs, tables):
        r.fill_cache(pool, L, tab, LAYER, s.K, s.V)
        pool[tab[:max(s.n - window, 0) // 64]] = 0xFF
    return pool


class _Decode:
    """one case on the device: the pool, the queries, and a workspace that is filled with 0xFF once"""

    def __init__(self, tm, case, pool_window):
        self.tm, self.case = tm, case
        klen, self.B, self.Hq = case.klen, len(case.seqs), case.Hq
        L = o.BlockLayout(2, case.Hkv, case.D, 64, case.bits)
        tables, total = _tables(np.random.default_rng(case.bits + case.D + case.Hq + case.window), klen)
        self.dc = DevCache(L, total, tables)
        self.dc.pool.copy_(torch.from_numpy(_pool(case, L, tables, total, pool_window)).cuda())
        self.q = dev(np.stack([s.q[0].reshape(-1) for s in case.seqs]))
        self.klen = dev(np.asarray(klen, np.int32))
        self.ws = torch.full((max(1, tm.tm_decode_attention_workspace(self.B, self.Hq, max(SPLITS))),), 0xFF, dtype=torch.uint8, device='cuda')
        self.sinks = None if case.sinks is None else dev(case.sinks)

    def run(self, splits, window, sinks=True):
        case = self.case
        out = torch.full((self.B, self.Hq * case.D), 0x7e00, dtype=torch.int16, device='cuda')
        sp = self.sinks.data_ptr() if sinks and self.sinks is not None else None
        _ffi.check(self.tm.tm_decode_attention_window(out.data_ptr(), self.q.data_ptr(), self.Hq * case.D, self.klen.data_ptr(), self.B,
                                                      self.Hq, r.softmax_scale(case.tier, case.D), splits, self.ws.data_ptr(),
                                                      self.dc.view(LAYER), window, sp, st()))
        got = host(out).view(np.uint16).reshape(self.B, self.Hq, case.D).copy()
        got[got == 0x8000] = 0
        return got


def _assert_bits(got, case, what):
    """-> worst ulp over the loose outputs"""
    worst = 0
    for b, s in enumerate(case.seqs):
        g, e = got[b], s.bits[0]
        bad = (g != e) & ~s.loose[0]
        assert not bad.any(), (f'{what}, sequence {b} (k_len {s.n}): {int(bad.sum())} outputs differ, first (head, channel) '
                               f'{tuple(np.argwhere(bad)[0])}: got {g[bad][0]:#06x}, expected {e[bad][0]:#06x}')
        worst = max(worst, int(r.ulp16(g, e)[s.loose[0]].max(initial=0)))
    assert worst <= 1, what
    return worst


# ---- decode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,bits', [(128, 8), (128, 4), (128, 16), (64, 8), (64, 4), (64, 16)])
def test_decode_window_exact(tm, cuda, D, bits):
    """every (head_dim, bits) runs the VALU kernel's window variant: six windows in both tiers, GQA groups 1, 2, 3, 4, 7, 8 (heads per
    workgroup 1, 2, 3, 4, seven chunks of 1, two chunks of 4), sinks off and on, 1 .. 16 splits"""
    n_cmp = n_loose = worst = 0
    for a in DECODE:
        if (a[1], a[0]) != (D, bits):
            continue
        case = r.decode_window_case(*a)
        dv = _Decode(tm, case, case.window)
        n_loose += sum(int(s.loose.sum()) for s in case.seqs)
        for splits in SPLITS:
            what = (f'bits {bits} head_dim {D} group {a[2]} tier {case.tier} window {case.window} '
                    f'sinks {"on" if case.sinks is not None else "off"} splits {splits}')
            worst = max(worst, _assert_bits(dv.run(splits, case.window), case, what))
            n_cmp += 1
    print(f'[attention window exact] decode bits {bits} head_dim {D}: {n_cmp} launches, all bits equal; {n_loose} loose outputs, worst {worst} ulp')


def _differs(got, case):
    """[B, Hq]: a strict output of that (sequence, head) is not the expected one"""
    return np.array([((got[b] != s.bits[0]) & ~s.loose[0]).any(-1) for b, s in enumerate(case.seqs)])


def test_decode_window_off_by_one_is_seen(tm, cuda):
    """negative control: the control case launched with W + 1 (the token in front of the window looks live) and with W - 1 (the
    window's first token is live) differs from the expectation in every sequence, at one split and at three"""
    case = r.control_case()
    W = case.window
    assert all(s.n > W + 1 for s in case.seqs)
    dv = _Decode(tm, case, W + 1)
    for splits in (1, 3):
        _assert_bits(dv.run(splits, W), case, f'control, splits {splits}')
        for w in (W + 1, W - 1):
            diff = _differs(dv.run(splits, w), case)
            print(f'[attention window exact] control window {w} for {W}, splits {splits}: {int(diff.sum())} of {diff.size} (sequence, head) differ')
            assert diff.any(1).all(), f'window {w} in place of {W} went unseen in sequences {np.flatnonzero(~diff.any(1))}'


def test_decode_missing_sinks_are_seen(tm, cuda):
    """negative control: the control case launched without its sinks differs in every head whose sink is +0 or -0 and equals the
    expectation in every head whose sink is -inf or -65504, in the kernel's epilogue (1 split) and behind the merge (2 splits)"""
    case = r.control_case()
    unit = case.sinks.astype(np.float64) == 0
    assert unit.any() and (~unit).any() and {0xfc00, 0xfbff} <= set(case.sinks.view(np.uint16).tolist())
    dv = _Decode(tm, case, case.window)
    for splits in (1, 2):
        diff = _differs(dv.run(splits, case.window, sinks=False), case)
        assert diff[:, unit].all(), f'splits {splits}: a missing sink of weight one went unseen'
        assert not diff[:, ~unit].any(), f'splits {splits}: a sink of weight zero changed an output'


# ---- prefill --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', r.WINDOWS_PREFILL)
@pytest.mark.parametrize('D', [128, 64])
def test_prefill_window_exact(tm, cuda, D, W):
    """W 1: the diagonal alone; 16, 17: edges inside a wave's 16 rows; 32, 33 and 64, 65: edges on a 32-key step and a 64-key stage;
    100; 4096: wider than everything.  History 0, inside the window, and (300 at W <= 100) wholly outside it"""
    n_cmp = n_loose = worst = 0
    for a in PREFILL:
        if (a[0], a[4]) != (D, W):
            continue
        case = r.prefill_window_case(*a)
        (qlens, hists), Hq, Hkv = a[3], case.Hq, case.Hkv
        klen, B = case.klen, len(case.seqs)
        koff = np.concatenate([[0], np.cumsum([((k + 63) // 64) * 64 for k in klen])]).astype(np.int32)
        stride = int(koff[-1])
        cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
        T = int(cu[-1])
        q = np.concatenate([s.q.reshape(len(s.q), -1) for s in case.seqs])
        K = np.full((Hkv, stride, D), np.nan, f16)        # garbage past the context must be masked, not multiplied
        Vt = np.zeros((Hkv, D, stride), f16)
        for b, s in enumerate(case.seqs):
            K[:, koff[b]:koff[b] + s.n] = s.K
            K[:, koff[b]:koff[b] + max(s.hist - W + 1, 0)] = np.nan                                    # ... and so in front of every window
            Vt[:, :, koff[b]:koff[b] + s.n] = s.V.transpose(0, 2, 1)
        out = torch.full((T, Hq * D), 0x7e00, dtype=torch.int16, device='cuda')
        sp = None if case.sinks is None else dev(case.sinks).data_ptr()
        _ffi.check(tm.tm_prefill_attention_window(out.data_ptr(), dev(q).data_ptr(), Hq * D, dev(K).data_ptr(), dev(Vt).data_ptr(), stride,
                                                  dev(cu).data_ptr(), dev(koff).data_ptr(), dev(np.asarray(klen, np.int32)).data_ptr(), B,
                                                  max(qlens), Hq, Hkv, D, r.softmax_scale(case.tier, D), W, sp, st()))
        got = host(out).view(np.uint16).copy()
        got[got == 0x8000] = 0
        for b, s in enumerate(case.seqs):
            g = got[cu[b]:cu[b + 1]].reshape(s.bits.shape)
            bad = (g != s.bits) & ~s.loose
            what = (f'prefill head_dim {D} group {a[1]} tier {case.tier} window {W} sinks {"on" if sp else "off"} '
                    f'q_lens {qlens} on {hists} sequence {b}')
            assert not bad.any(), (f'{what}: {int(bad.sum())} outputs differ, first (row, head, channel) {tuple(np.argwhere(bad)[0])}: '
                                   f'got {g[bad][0]:#06x}, expected {s.bits[bad][0]:#06x}')
            worst = max(worst, int(r.ulp16(g, s.bits)[s.loose].max(initial=0)))
            n_loose += int(s.loose.sum())
        assert worst <= 1
        n_cmp += 1
    print(f'[attention window exact] prefill head_dim {D} window {W}: {n_cmp} launches, all bits equal; {n_loose} loose outputs, worst {worst} ulp')
