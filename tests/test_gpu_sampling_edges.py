"""tm_sample, tm_sample_logprobs, tm_seen_update and tm_logits_process (csrc/sampling.hip) at their structural edges, against
oracle.tm_oracle: bin ownership of the 1024-thread walk (thread, wave and sign boundaries, both ends of the fp16 range),
vocabularies of 1 .. 2049 and beyond 131072 logits (the histogram's second trip), the off-by-one positions of the logprobs list,
degenerate rows through the logprobs path, one workspace shared by calls of different shapes, vocabulary shards whose offset is
16 (mod 32), empty sequences and out-of-range ids in the seen masks, and penalty inputs at the ends of the number format.

Inputs, the bin model and the margin rule live in tests/sampling_edges_reference.py and are proved on the CPU by
tests/test_host_sampling_edges.py: every top_p, min_p and u keeps >= 64 V 2^-53 from the nearest value at which the oracle's answer
would change, so a disagreement is a kernel error and not rounding.  Bounds are those of tests/test_gpu_ops.py: ids and counts
exact, logprobs within 1e-5 + 1e-6 |x|, equal -inf patterns, processed logits bit for bit (NaN by isnan).

Configurations this module caught: none so far.
"""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import sampling_edges_reference as R
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
POISON_VAL, POISON_IDX = 7.0, -5


def _workspace(tm, batch):
    return torch.zeros(tm.tm_sample_workspace(batch), dtype=torch.uint8, device='cuda')


def _sample(tm, c, ws, cap=0, min_p=True):
    """one tm_sample (cap = 0) or tm_sample_logprobs call over the rows of c; every output starts poisoned"""
    B = c.B
    out = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    kept = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    args = (dev(c.logits).data_ptr(), B, c.V, c.ld, dev(c.temperature).data_ptr(), dev(c.top_k).data_ptr(), dev(c.top_p).data_ptr(),
            dev(c.min_p).data_ptr() if min_p else None, dev(c.u).data_ptr(), ws.data_ptr(), st())
    if not cap:
        _ffi.check(tm.tm_sample(out.data_ptr(), kept.data_ptr(), *args))
        return dict(out=host(out), kept=host(kept))
    vals = torch.full((B, cap), POISON_VAL, dtype=torch.float32, device='cuda')
    idx = torch.full((B, cap), POISON_IDX, dtype=torch.int32, device='cuda')
    num = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    sel = torch.full((B,), POISON_VAL, dtype=torch.float32, device='cuda')
    _ffi.check(tm.tm_sample_logprobs(out.data_ptr(), kept.data_ptr(), vals.data_ptr(), idx.data_ptr(), num.data_ptr(), sel.data_ptr(),
                                     cap, *args))
    return dict(out=host(out), kept=host(kept), vals=host(vals), idx=host(idx), num=host(num), sel=host(sel))


def _check_draw(c, r, rows=None):
    """kept and the drawn token of batch rows `rows` equal the oracle's for the rows of c"""
    for i, (ids, p, tok) in enumerate(c.expected()):
        b = i if rows is None else rows[i]
        assert r['kept'][b] == len(ids), f'{c.name} row {b} ({c.tags[i]}): kept {r["kept"][b]} vs {len(ids)}'
        assert r['out'][b] == tok, f'{c.name} row {b} ({c.tags[i]}): token {r["out"][b]} vs {tok}'


def _check_logprobs(c, r, cap, rows=None):
    """the assertions of test_sampling_logprobs_match_oracle; returns the number of rows that drew a token behind the cap"""
    tail_draws = 0
    for i, (ids, p, tok) in enumerate(c.expected()):
        b = i if rows is None else rows[i]
        what = f'{c.name} cap {cap} row {b} ({c.tags[i]})'
        e_ids, e_lp, e_sel = o.sample_logprobs(ids, p, int(r['out'][b]), cap)
        n = len(e_ids)
        g_vals, g_idx = r['vals'][b], r['idx'][b]
        assert r['num'][b] == n == min(len(ids), cap), f'{what}: num {r["num"][b]} vs {n}'
        assert np.array_equal(g_idx[:n], e_ids), f'{what}: candidate order'
        fin = np.isfinite(e_lp)
        assert np.array_equal(np.isfinite(g_vals[:n]), fin) and np.all(g_vals[:n][~fin] == -np.inf), what
        assert np.all(np.abs(g_vals[:n][fin] - e_lp[fin]) <= 1e-5 + 1e-6 * np.abs(e_lp[fin])), what
        assert abs(r['sel'][b] - e_sel) <= 1e-5 + 1e-6 * abs(e_sel) or r['sel'][b] == e_sel, f'{what}: drawn token'
        assert np.all(g_idx[n:] == POISON_IDX) and np.all(g_vals[n:] == POISON_VAL), f'{what}: entries beyond num must stay untouched'
        tail_draws += int(np.flatnonzero(ids == r['out'][b])[0]) >= cap
    return tail_draws


# ------------------------------------------------------------------------------------------------
# section 2: bin ownership
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(R.BOUNDARY_SETS))
def test_bin_boundaries(tm, cuda, name):
    """Four adjacent fp16 values, sixteen tokens each, straddling a thread, a wave, the sign, the top and the bottom of the bin
    walk; top_k, top_p, min_p and u placed on both sides of every group edge (R.boundary_call).  kept and token equal the oracle."""
    c = R.boundary_call(name)
    ws = _workspace(tm, c.B)
    r = _sample(tm, c, ws)
    print(f'{c.name}: kept {r["kept"].tolist()} tokens {r["out"].tolist()}')
    _check_draw(c, r)
    assert not ws.any()


# ------------------------------------------------------------------------------------------------
# section 3: vocabulary sizes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,ld', R.SMALL_VOCABS)
def test_small_vocabularies(tm, cuda, V, ld):
    """V < 8: only the scalar tail of the histogram runs; V < 1024: most threads own no token in pass C; parameters larger than V clamp."""
    c = R.small_vocab_call(V, ld)
    ws = _workspace(tm, c.B)
    r = _sample(tm, c, ws)
    print(f'{c.name}: kept {r["kept"].tolist()} tokens {r["out"].tolist()}')
    _check_draw(c, r)
    assert not ws.any()
    r = _sample(tm, c, ws, cap=R.SMALL_CAP)
    _check_draw(c, r)
    _check_logprobs(c, r, R.SMALL_CAP)
    assert not ws.any()


@pytest.mark.parametrize('V,ld', R.BIG_VOCABS)
def test_large_vocabularies(tm, cuda, V, ld):
    """V > 131072: the histogram's grid-stride loop takes a second trip (137221: with a partial last vector).  A flat row is one bin
    of V members (kept = floor(0.3f V) + 1), one row has its eleven best logits behind id 131072 and draws there."""
    c = R.big_vocab_call(V, ld)
    ws = _workspace(tm, c.B)
    for rep in range(2):                                   # the second call checks that the workspace was left zeroed
        r = _sample(tm, c, ws)
        print(f'{c.name}: kept {r["kept"].tolist()} tokens {r["out"].tolist()}')
        _check_draw(c, r)
        assert r['kept'][R.BIG_FLAT_ROW] == int(np.floor(np.float64(f32(0.3)) * V)) + 1
        assert (r['out'] >= R.SECOND_TRIP).any() and r['out'][R.BIG_HIGH_ROW] >= R.SECOND_TRIP
    assert not ws.any()
    for cap in (1024, 20):
        r = _sample(tm, c, ws, cap=cap)
        _check_draw(c, r)
        assert _check_logprobs(c, r, cap) > 0, 'no row drew a token beyond the cap: the forced-last / sel path was not exercised'
        assert not ws.any()


def _process(tm, V, ld, off, vocab, x, rows):
    """tm_seen_update (packed rows, some of them empty) + tm_logits_process against o.logits_process, bit for bit"""
    B = len(rows)
    words = (vocab + 31) // 32
    seen_ids = [np.asarray(r.get('seen', []), np.int32) for r in rows]
    cu_q = np.concatenate([[0], np.cumsum([len(s) for s in seen_ids])]).astype(np.int32)
    seen = torch.zeros((B, words), dtype=torch.int32, device='cuda')
    if cu_q[-1]:
        _ffi.check(tm.tm_seen_update(seen.data_ptr(), words, dev(np.concatenate(seen_ids)).data_ptr(), dev(cu_q).data_ptr(), B,
                                     int(cu_q[-1]), vocab, st()))
    assert np.array_equal(host(seen).view(np.uint32), R.mask_of(seen_ids, words, vocab))
    ban = np.full((B, R.KMAX_BAD), -1, np.int32)
    end = np.full((B, R.KMAX_END), -1, np.int32)
    for b, r in enumerate(rows):
        ban[b, :len(r.get('bad', []))] = r.get('bad', [])
        end[b, :len(r.get('end', []))] = r.get('end', [])
    arr = lambda k, d, t: np.asarray([r.get(k, d) for r in rows], t)
    rep, k_len, min_len = arr('p', 1.0, f32), arr('k', 5, np.int32), arr('ml', 0, np.int32)
    d_logits = dev(x).clone()
    _ffi.check(tm.tm_logits_process(d_logits.data_ptr(), B, V, ld, off, seen.data_ptr(), words, dev(rep).data_ptr(),
                                    dev(ban).data_ptr(), dev(end).data_ptr(), dev(k_len).data_ptr(), dev(min_len).data_ptr(), st()))
    got = host(d_logits)
    for b, ref in enumerate(R.process_expected(x, V, off, rows)):
        assert R.same_bits_or_nan(got[b, :V], ref), f'row {b} {rows[b].get("p")}: columns {np.flatnonzero(got[b, :V].view(np.uint16) != ref.view(np.uint16))[:8]}'
        assert R.same_bits_or_nan(got[b, V:], x[b, V:]), 'padding touched'
    return got


@pytest.mark.parametrize('V,ld,off,vocab', R.SHARD_CASES)
def test_logits_process_shards(tm, cuda, V, ld, off, vocab):
    """The rows of test_logits_process_matches_oracle on the full Qwen vocabulary and on TP-8 shards of the two largest served
    vocabularies: their offsets are 16 (mod 32), the seen-mask word is read with a non-zero shift."""
    x, rows = R.process_shard_case(V, ld, off, vocab)
    _process(tm, V, ld, off, vocab, x, rows)


# ------------------------------------------------------------------------------------------------
# section 4: logprobs boundaries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', R.LP_CAPS)
def test_logprobs_boundaries(tm, cuda, C):
    """kept = cap - 1 / cap / cap + 1, a list taken entirely from one tie bin, one member from the cut bin, groups that end exactly
    at the cap; cap = 1024: the drawn token at position 1023 (entry 1023 anyway) and 1024 (replaces entry 1023); cap = 5: a draw
    behind the cap forces nothing."""
    c = R.logprobs_call(C)
    ws = _workspace(tm, c.B)
    r = _sample(tm, c, ws, cap=C)
    print(f'{c.name}: kept {r["kept"].tolist()} num {r["num"].tolist()} tokens {r["out"].tolist()}')
    _check_draw(c, r)
    _check_logprobs(c, r, C)
    for b, ((ids, p, tok), (kept, nA, pos)) in enumerate(zip(c.expected(), c.claims)):
        if pos is None:
            continue
        assert r['out'][b] == ids[pos]
        if C == 1024:
            assert r['idx'][b, 1023] == tok and r['vals'][b, 1023] == r['sel'][b]
            assert np.array_equal(r['idx'][b, :1023], ids[:1023])
        else:
            assert np.array_equal(r['idx'][b, :C], ids[:C]) and tok not in r['idx'][b]
        assert abs(r['sel'][b] - np.log(p[pos])) <= 1e-5 + 1e-6 * abs(np.log(p[pos]))
    assert not ws.any()


# ------------------------------------------------------------------------------------------------
# section 5: degenerate rows through the logprobs path
# ------------------------------------------------------------------------------------------------
def test_degenerate_rows_through_logprobs(tm, cuda):
    """The rows of test_sampling_degenerate_rows_get_a_defined_token between ordinary ones, kept_out requested, cap = 8.  All NaN,
    a +inf maximum, all -inf: the defined token, num = 0, sel = 0.0, the list untouched.  NaN entries of an ordinary row carry
    zero probability: the row equals the oracle with NaN -> -inf."""
    gpu, ref, proper = R.degenerate_call()
    cap = R.DEGENERATE_CAP
    ws = _workspace(tm, gpu.B)
    r = _sample(tm, gpu, ws, cap=cap, min_p=False)
    print(f'degenerate: kept {r["kept"].tolist()} num {r["num"].tolist()} tokens {r["out"].tolist()} sel {r["sel"].tolist()}')
    for b, kind in enumerate(R.DEGENERATE_LAYOUT):
        if b in R.DEGENERATE_TOKENS:
            assert r['out'][b] == R.DEGENERATE_TOKENS[b], f'row {b} ({kind}): token {r["out"][b]}'
        if b not in proper:
            assert r['num'][b] == 0 and r['sel'][b] == 0.0, f'row {b} ({kind})'
            assert np.all(r['idx'][b] == POISON_IDX) and np.all(r['vals'][b] == POISON_VAL), f'row {b} ({kind}): list touched'
    _check_draw(ref, r, proper)
    _check_logprobs(ref, r, cap, proper)
    assert not ws.any()


# ------------------------------------------------------------------------------------------------
# section 6: one workspace, calls of different shapes
# ------------------------------------------------------------------------------------------------
def test_workspace_reuse_across_shapes(tm, cuda):
    """The engine calls the sampler with another batch size each step.  One workspace for 13 rows, zeroed once: 13 rows of 151936,
    3 rows of 1000, 13 rows of 9 with logprobs, the 3 rows again.  Each call returns what it returns on a fresh workspace."""
    calls = R.reuse_calls()
    caps = (0, 0, R.SMALL_CAP, 0)
    ws = _workspace(tm, 13)
    for c, cap in zip(calls, caps):
        assert c.B <= 13
        got = _sample(tm, c, ws, cap=cap)
        fresh = _sample(tm, c, _workspace(tm, c.B), cap=cap)
        for k in got:
            assert np.array_equal(got[k], fresh[k]), f'{c.name}: {k} differs from the call on a fresh workspace'
        _check_draw(c, got)
        if cap:
            _check_logprobs(c, got, cap)
    assert not ws.any()


# ------------------------------------------------------------------------------------------------
# section 7: seen masks and processor values
# ------------------------------------------------------------------------------------------------
def test_seen_update_empty_sequences_and_foreign_ids(tm, cuda):
    """cu_q = [0, 0, 5, 5, 9, 9]: the first, a middle and the last sequence are empty; ids -1, vocab and vocab + 40 are ignored,
    duplicates set one bit, ids 31 / 32 sit in two words, vocab - 1 in the last, partial word.  n_tokens = 0 does nothing."""
    cu_q, ids, per_seq, vocab, words = R.packed_seen_case()
    nseq = len(cu_q) - 1
    seen = torch.zeros((nseq + 1, words), dtype=torch.int32, device='cuda')          # one canary row behind
    _ffi.check(tm.tm_seen_update(seen.data_ptr(), words, dev(ids).data_ptr(), dev(cu_q).data_ptr(), nseq, 0, vocab, st()))
    assert not seen.any()
    _ffi.check(tm.tm_seen_update(seen.data_ptr(), words, dev(ids).data_ptr(), dev(cu_q).data_ptr(), nseq, len(ids), vocab, st()))
    got = host(seen).view(np.uint32)
    assert np.array_equal(got[:nseq], R.mask_of(per_seq, words, vocab)) and not got[nseq].any()
    assert not got[[0, 2, 4]].any(), 'an empty sequence got a token'
    # decode rows (no cu_q): one token per row, foreign ids among them
    last = np.asarray([-1, vocab, 31, vocab - 1, vocab + 40], np.int32)
    _ffi.check(tm.tm_seen_update(seen.data_ptr(), words, dev(last).data_ptr(), None, nseq, nseq, vocab, st()))
    want = R.mask_of([list(s) + [t] for s, t in zip(per_seq, last)], words, vocab)
    got = host(seen).view(np.uint32)
    assert np.array_equal(got[:nseq], want) and not got[nseq].any()


@pytest.mark.parametrize('case', range(3))
def test_logits_process_edges(tm, cuda, case):
    """Bad ids on the workgroup edge (2047 / 2048), in the scalar tail (4096, 4098), duplicated, and seen with a penalty (the ban
    wins); a shard at offset 16: ids one outside either end change nothing, its first and last column are banned; the penalty on
    +-0, +-2^-24, +-65504 (65504 / 0.5 = +inf), +-inf and NaN under p = 0.5, 2, and 1, 0, -1, which leave the row as it was."""
    name, V, ld, off, vocab, x, rows = R.process_edge_cases()[case]
    got = _process(tm, V, ld, off, vocab, x, rows)
    if name == 'penalty values':
        for b, p in enumerate(R.PENALTIES):
            if p in (1.0, 0.0, -1.0):
                assert R.same_bits_or_nan(got[b], x[b]), f'p = {p} changed the row'
        assert got[0, 4] == np.inf and got[0].view(np.uint16)[1] == 0x8000
    if name == 'shard+16':
        assert R.same_bits_or_nan(got[0], x[0])
