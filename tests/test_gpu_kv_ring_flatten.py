"""tm_flatten_kv_window (flatten_kv_kernel<.., WIN = true>, kv_cache.hip) against tm_flatten_kv, bit for bit: over a scratch poisoned
with an fp16 NaN pattern every 64-token tile with t0 + 64 <= max(k_len - q_len - window + 1, 0) still holds the pattern after the call
(it is neither read nor written), every other byte of the scratch equals what tm_flatten_kv leaves there, and
tm_prefill_attention_window over the partly flattened scratch returns the bytes it returns over the fully flattened one -- the
windowed prefill kernel never stages a skipped tile.  window = 0 is the old call.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests.gpu_helpers import DevCache, dev, host, st

pytestmark = pytest.mark.gpu
f16 = np.float16
NAN = 0x7e00
CASES = [(0, 70), (63, 1), (64, 70), (200, 70)]      # (hist, q_len) of sequence 0
SECOND = (130, 5)                                    # sequence 1 of every batch: another length, another number of skipped tiles
WINDOWS = [1, 40, 64, 65]
HQ, HKV, LAYER = 4, 2, 1


def _poisoned(shape):
    return torch.full(shape, NAN, dtype=torch.int16, device='cuda').view(torch.float16)


def _flatten(tm, case, window):
    """(K, V^T) scratch as uint16 after one flatten call over the poisoned scratch; window None: tm_flatten_kv"""
    kf, vf = _poisoned((HKV, case['stride'], case['D'])), _poisoned((HKV, case['D'], case['stride']))
    head = (kf.data_ptr(), vf.data_ptr(), 1, case['koff_d'].data_ptr(), case['klen_d'].data_ptr(), 2, max(case['klen']), case['stride'],
            case['dc'].view(LAYER))
    if window is None:
        _ffi.check(tm.tm_flatten_kv(*head, st()))
    else:
        _ffi.check(tm.tm_flatten_kv_window(*head, case['cu_d'].data_ptr(), window, st()))
    return kf, vf


def _attention(tm, case, kf, vf, window):
    out = torch.zeros((int(case['cu'][-1]), HQ * case['D']), dtype=torch.float16, device='cuda')
    _ffi.check(tm.tm_prefill_attention_window(out.data_ptr(), case['q_d'].data_ptr(), HQ * case['D'], kf.data_ptr(), vf.data_ptr(), case['stride'],
                                              case['cu_d'].data_ptr(), case['koff_d'].data_ptr(), case['klen_d'].data_ptr(), 2,
                                              max(case['qlen']), HQ, HKV, case['D'], 0.0, window, None, st()))
    return host(out).view(np.uint16)


_CASES = {}


def _case(tm, D, bits, hist, qlen):
    """the filled cache, the queries and the fully flattened scratch of one (head_dim, KV width, lengths): built once, left unchanged"""
    key = (D, bits, hist, qlen)
    if key not in _CASES:
        rng = np.random.default_rng(D + bits + 7 * hist + qlen)
        hists, qlens = (hist, SECOND[0]), (qlen, SECOND[1])
        klen = [h + n for h, n in zip(hists, qlens)]
        L = o.BlockLayout(2, HKV, D, 64, bits)
        nblk = [(k + 63) // 64 for k in klen]
        perm = rng.permutation(sum(nblk) + 2)
        tables = [perm[:nblk[0]], perm[nblk[0]:nblk[0] + nblk[1]]]
        oc = o.PagedKVCache(L, len(perm))
        for b, n in enumerate(klen):
            o.process_kv(oc, tables[b], LAYER, rng.standard_normal((n, HKV, D)).astype(f16), rng.standard_normal((n, HKV, D)).astype(f16),
                         None, None, 0)
        dc = DevCache(L, len(perm), tables)
        dc.upload(oc)
        koff = np.concatenate([[0], np.cumsum([nb * 64 for nb in nblk])]).astype(np.int32)
        cu = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
        # the tensors live as long as the case (gpu_helpers.dev() frees its tensors after every test)
        case = dict(D=D, hist=hists, qlen=qlens, klen=klen, koff=koff, cu=cu, stride=int(koff[-1]) + 64, dc=dc,
                    koff_d=torch.from_numpy(koff).cuda(), klen_d=torch.from_numpy(np.asarray(klen, np.int32)).cuda(),
                    cu_d=torch.from_numpy(cu).cuda(),
                    q_d=torch.from_numpy(rng.standard_normal((int(cu[-1]), HQ * D)).astype(f16)).cuda())
        kf, vf = _flatten(tm, case, None)
        case['kf'], case['vf'] = kf, vf
        case['K'], case['Vt'] = host(kf).view(np.uint16), host(vf).view(np.uint16)
        _CASES[key] = case
    return _CASES[key]


def _skipped_columns(case, window):
    """bool [stride]: token columns of the scratch inside a skipped tile"""
    cols = np.zeros(case['stride'], bool)
    for b in range(2):
        first = max(case['hist'][b] - window + 1, 0)
        for t0 in range(0, case['klen'][b], 64):
            if t0 + 64 <= first:
                cols[case['koff'][b] + t0:case['koff'][b] + t0 + 64] = True
    return cols


def test_the_grid_skips_something_and_keeps_something():
    """the grid below is worth running: cases with no, one and several skipped tiles, none that skips a whole sequence"""
    n_skipped = set()
    for hist, qlen in CASES:
        for w in WINDOWS:
            case = dict(hist=(hist, SECOND[0]), klen=[hist + qlen, sum(SECOND)], stride=1024, koff=[0, 512])
            tiles = int(_skipped_columns(case, w)[:512].sum()) // 64
            assert tiles < -(-(hist + qlen) // 64)
            n_skipped.add(tiles)
    assert {0, 1, 3} <= n_skipped


@pytest.mark.parametrize('hist,qlen', CASES)
@pytest.mark.parametrize('bits', [16, 8, 4])
@pytest.mark.parametrize('D', [64, 128])
def test_flatten_window_skips_exactly_the_unreachable_tiles(tm, cuda, D, bits, hist, qlen):
    case = _case(tm, D, bits, hist, qlen)
    # window = 0: the old call's bytes (cu_q_len may be NULL)
    kf, vf = _poisoned((HKV, case['stride'], D)), _poisoned((HKV, D, case['stride']))
    _ffi.check(tm.tm_flatten_kv_window(kf.data_ptr(), vf.data_ptr(), 1, case['koff_d'].data_ptr(), case['klen_d'].data_ptr(), 2,
                                       max(case['klen']), case['stride'], case['dc'].view(LAYER), None, 0, st()))
    assert np.array_equal(host(kf).view(np.uint16), case['K']) and np.array_equal(host(vf).view(np.uint16), case['Vt'])
    for w in WINDOWS:
        kf, vf = _flatten(tm, case, w)
        skip = _skipped_columns(case, w)
        want_k, want_v = case['K'].copy(), case['Vt'].copy()
        want_k[:, skip, :] = NAN
        want_v[:, :, skip] = NAN
        K, Vt = host(kf).view(np.uint16), host(vf).view(np.uint16)
        assert (K[:, skip, :] == NAN).all() and (Vt[:, :, skip] == NAN).all(), f'window {w}: a skipped tile was written'
        assert np.array_equal(K, want_k) and np.array_equal(Vt, want_v), f'window {w}: a tile that is not skipped differs from tm_flatten_kv'
        got = _attention(tm, case, kf, vf, w)
        ref = _attention(tm, case, case['kf'], case['vf'], w)
        assert not np.isnan(got.view(f16)).any()              # the poison reaches no output: no skipped tile is staged
        assert np.array_equal(got, ref), f'window {w}: attention over the windowed scratch differs in {np.count_nonzero(got != ref)} halves'


def test_flatten_window_refusals(tm, cuda):
    case = _case(tm, 64, 8, 64, 70)
    kf, vf = _poisoned((HKV, case['stride'], 64)), _poisoned((HKV, 64, case['stride']))
    head = (kf.data_ptr(), vf.data_ptr(), 1, case['koff_d'].data_ptr(), case['klen_d'].data_ptr(), 2, max(case['klen']), case['stride'],
            case['dc'].view(LAYER))
    assert tm.tm_flatten_kv_window(*head, case['cu_d'].data_ptr(), -1, st()) == 1
    assert tm.tm_flatten_kv_window(*head, None, 40, st()) == 1           # a window needs the query rows
    torch.cuda.synchronize()
    assert (host(kf).view(np.uint16) == NAN).all() and (host(vf).view(np.uint16) == NAN).all()
