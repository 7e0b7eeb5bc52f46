"""CPU proof of tests/attention_exact_reference.py, the operands of tests/test_gpu_attention_exact.py.

Preconditions: the builder's own assertions (round trip through the KV quantiser, integer scores, a live token per query, dead tokens
150 below the maximum, the fp32 budget, the distance from the fp16 rounding boundaries with its 1-in-1000 cap, agreement with the
oracle's fp64 reference and its tiled prefill restatement) hold for every case the GPU module runs.
Order independence: the oracle's fp32 restatement of the online softmax returns the expected bits whatever the tile size, the split
count and the direction of the walk.
Sensitivity: every error the construction is meant to expose, applied to the reference COMPUTATION, changes the expected bits in
every case that has the feature; the number of changed (sequence, head) pairs is printed."""
import numpy as np
import pytest

from oracle import tm_oracle as o
from tests import attention_exact_reference as r

f16, f32 = np.float16, np.float32
KLEN_SHORT = (1, 63, 64, 65, 129, 257, 1089)                 # the fused-prologue batch of the GPU module


def test_log2_scale_is_an_exact_power_of_two():
    """c_api.hip: scale_log2 = s * 1.4426950408889634f in float32; for s = float32(ln 2 * 2^-k) that is 2^-k, and for neither
    float32 neighbour of float32(ln 2 / 32)"""
    for k in range(6):
        s = f32(np.log(2.0) * 2.0**-k)
        assert f32(s * r.LOG2E) == f32(2.0**-k), k
    s = r.SCALE_B
    assert s == f32(np.log(2.0) * 2.0**-5) and r.scale_log2('B', 128) == f32(2.0**-5)
    for nb in (np.nextafter(s, f32(0)), np.nextafter(s, f32(1))):
        assert f32(nb * r.LOG2E) != f32(2.0**-5)


@pytest.mark.parametrize('D,bits', [(128, 8), (128, 4), (128, 16), (64, 8), (64, 4), (64, 16)])
def test_decode_cases_hold_the_builder_assertions(D, bits):
    for group in r.GROUPS_DECODE:
        for tier in 'AB':
            case = r.decode_case(bits, D, group, tier)
            assert sum(int(s.loose.sum()) for s in case.seqs) * 1000 <= case.total
            # the placed live sets: every pattern somewhere in the case, never more than 32 live tokens
            for s in case.seqs:
                _, _, _, extra = r.reference(case, s, detail=True)
                for hd in extra:
                    nlive = (extra[hd][0][:s.n] > 0).sum(0)
                    assert nlive.min() >= 1 and nlive.max() <= 32
    if D == 128 and bits != 16:
        for tier in 'AB':
            r.decode_case(bits, D, 8, tier, KLEN_SHORT)


@pytest.mark.parametrize('D', [128, 64])
def test_prefill_cases_hold_the_builder_assertions(D):
    for group in r.GROUPS_PREFILL:
        for shape in r.PREFILL_SHAPES:
            for tier in 'AB':
                case = r.prefill_case(D, group, tier, shape)
                assert sum(int(s.loose.sum()) for s in case.seqs) * 1000 <= case.total


def test_vectorised_cache_fill_is_the_oracle_store():
    for bits in (8, 4, 16):
        case = r.decode_case(bits, 64, 4, 'B', (1, 65, 130))
        L = o.BlockLayout(2, case.Hkv, 64, 64, bits)
        tabs = [np.array([3]), np.array([0, 5]), np.array([4, 1, 2])]
        pool = np.zeros((6, L.block_size), np.uint8)
        oc = o.PagedKVCache(L, 6)
        for s, t in zip(case.seqs, tabs):
            r.fill_cache(pool, L, t, 1, s.K, s.V)
            o.process_kv(oc, t, 1, s.K.transpose(1, 0, 2), s.V.transpose(1, 0, 2), None, None, 0)
        assert np.array_equal(pool, oc.pool)


# ---- order independence ---------------------------------------------------------------------------------------------------------
def _bits(x):
    b = np.asarray(x, f16).view(np.uint16).copy()
    b[b == 0x8000] = 0
    return b


@pytest.mark.parametrize('tier', ['A', 'B'])
@pytest.mark.parametrize('bits,D,group', [(8, 128, 8), (4, 128, 8), (16, 128, 4), (8, 64, 6)])
def test_restatement_is_order_independent(bits, D, group, tier):
    """o.attention_tiles + o.attention_merge through o.decode_attention: splits 1, 2, 3, 16, tiles of 16 and 64 tokens, newest-first
    and (on the token-reversed sequence) oldest-first"""
    case = r.decode_case(bits, D, group, tier, KLEN_SHORT)
    scale = None if tier == 'A' else float(r.SCALE_B)
    for s in case.seqs:
        K, V = s.K[:, :s.n], s.V[:, :s.n]
        for flip in (False, True):
            Kf, Vf = (K[:, ::-1], V[:, ::-1]) if flip else (K, V)
            for tile in (16, 64):
                for splits in (1, 2, 3, 16):
                    got = _bits(o.decode_attention(s.q[0], Kf, Vf, scale, splits, tile))
                    assert np.array_equal(got, s.bits[0]), (s.n, flip, tile, splits)


@pytest.mark.parametrize('tier', ['A', 'B'])
def test_prefill_restatement_with_small_tiles(tier):
    case = r.prefill_case(64, 4, tier, r.PREFILL_SHAPES[0])
    for s in case.seqs:
        got = _bits(o.prefill_attention(s.q, s.K, s.V, s.hist, None if tier == 'A' else float(r.SCALE_B), tile=16))
        assert np.array_equal(got, s.bits)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
def _changed(case, muts_of):
    """number of (sequence, head) pairs whose expected bits change under any of the mutations muts_of(s) of that sequence"""
    n = 0
    for s in case.seqs:
        hit = np.zeros(case.Hq, bool)
        for mut in muts_of(s):
            hit |= (r.reference(case, s, mut) != s.bits).any((0, 2))
        n += int(hit.sum())
    return n


def _tile_muts(which, factor):
    def muts(s):
        out = []
        for splits in (2, 3, 16):                             # the 4161-token sequence is left out: 66 tiles say nothing new
            for a, b in o.split_ranges(s.n, splits, 64):
                if b > a and 64 < s.n <= 1089 and (splits < 16 or s.n == 1089):
                    out.append(('tile_factor', (a, a + 64, factor) if which == 'first' else ((b - 1) // 64 * 64, b, factor)))
        return out
    return muts


def _mutations(case):
    """name -> (has the feature, mutations of a sequence)"""
    decode = case.kind == 'decode'
    G = case.Hq // case.Hkv
    m = {
        'drop the newest visible token (decode: ctx - 1; prefill: diagonal - 1)': (True, lambda s: [('ctx_shift', -1)]),
        'let in the token behind the context (decode: ctx; prefill: diagonal + 1)': (True, lambda s: [('ctx_shift', +1)]),
        'use token t + 1\'s V (scale, zero) for token t': (decode and case.bits != 16, lambda s: [('next_v_param', None)]),
        'give head h the live set of head h + 1': (G > 1, lambda s: [('next_head', None)]),
        'skip the rescale once where the max moved': (True, lambda s: [('skip_rescale', -1 if decode else +1)]),
        'treat a dead token as weight 2^-20': (True, lambda s: [('dead_weight', 20)]),
    }
    if decode:
        m['drop the first tile of a split'] = (True, _tile_muts('first', 0.0))
        m['drop the last tile of a split'] = (True, _tile_muts('last', 0.0))
        m['count the first tile of a split twice'] = (True, _tile_muts('first', 2.0))
        m['count the last tile of a split twice'] = (True, _tile_muts('last', 2.0))
    else:
        m['drop a 64-key stage'] = (True, lambda s: [('tile_factor', (a, a + 64, 0.0)) for a in range(0, s.n, 64)])
        m['count a 64-key stage twice'] = (True, lambda s: [('tile_factor', (a, a + 64, 2.0)) for a in range(0, s.n, 64)])
    return m


def _sensitivity(cases):
    totals = {}
    for case in cases:
        for name, (has, muts) in _mutations(case).items():
            if has:
                n = _changed(case, muts)
                assert n > 0, f'"{name}" changes nothing in {case.kind} bits {case.bits} head_dim {case.D} Hq {case.Hq} tier {case.tier}'
                totals[name] = totals.get(name, 0) + n
    for name, n in totals.items():
        print(f'[attention exact sensitivity] {name}: {n} (sequence, head) pairs change')


@pytest.mark.parametrize('D,bits', [(128, 8), (128, 4), (128, 16), (64, 8), (64, 4), (64, 16)])
def test_decode_reference_is_sensitive(D, bits):
    _sensitivity(r.decode_case(bits, D, group, tier) for group in r.GROUPS_DECODE for tier in 'AB')


@pytest.mark.parametrize('D', [128, 64])
def test_prefill_reference_is_sensitive(D):
    _sensitivity(r.prefill_case(D, group, tier, shape) for group in r.GROUPS_PREFILL for shape in r.PREFILL_SHAPES for tier in 'AB')
