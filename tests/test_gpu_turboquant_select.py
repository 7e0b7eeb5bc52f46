"""The TurboQuant decode attention kernel (csrc/attention_decode_tq.hip, quant_policy 42) held to WHICH TOKENS each head attends:
the operands of tests/turboquant_select_reference.py make every softmax weight exactly 1 (the live set of the head) or exactly 0, so
the output is the mean of the live V rows and |gpu - expected| <= 2^-10 * max |expected row| (one fp32 butterfly, one fp16 rounding)
-- a mismatch is a wrong token set, a wrong head, a wrong (n, g) pairing or a lost partial, never accumulation order.
tests/test_host_turboquant_select.py shows on the host that each such fault misses this bound by more than a factor 4.

Per GQA group 1 .. 8, 10 (every HPW instantiation, one head chunk and several): 13 sequences of contexts 1 .. 1089 in one launch, Hkv 2,
layer 1 of 2, shuffled block tables with two spare blocks, ragged and rectangular, split counts 1, 2, 3 and 16 (splits without a tile),
the output pre-filled with fp16 NaN, the split-K workspace filled with 0xFF once and never cleared, 0xFF in every byte of the pool the
kernel must not read, look-alive rows behind the context.  The sweep case rolls the live sets of context 300 over every position.

Configurations this module caught: none so far."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from tests import turboquant_reference as tq
from tests import turboquant_select_reference as r
from tests.gpu_helpers import DevCache, dev, host, st

pytestmark = pytest.mark.gpu


def _run(tm, case):
    """every launch of a case -> (launches, worst err / bound); the first (sequence, head) out of bound fails with its explanation"""
    Hq, B, klen = case.Hq, len(case.seqs), case.klen
    hpw, chunks = r.hpw_chunks(case.group)
    L = tq.TqBlockLayout(r.LAYERS, r.HKV)
    tabs, total = r.tables(case)
    dc = DevCache(L, total, tabs)
    dc.pool.copy_(torch.from_numpy(r.fill_pool(case, tabs, total)).cuda())
    q_d = dev(np.stack([s.q.reshape(-1) for s in case.seqs]))
    klen_d = dev(np.asarray(klen, np.int32))
    ws = torch.full((max(1, tm.tm_decode_attention_workspace(B, Hq, max(r.SPLITS))),), 0xFF, dtype=torch.uint8, device='cuda')
    stride = max(len(t) for t in tabs) + 2
    launches, worst = 0, 0.0
    for mode in (0, stride):                                           # ragged and rectangular block tables
        dc.set_tables(tabs, stride=mode)
        for splits in r.SPLITS:
            out = torch.full((B, Hq * r.D), r.NAN16, dtype=torch.int16, device='cuda')
            _ffi.check(tm.tm_decode_attention(out.data_ptr(), q_d.data_ptr(), Hq * r.D, klen_d.data_ptr(), B, Hq, 0.0, splits,
                                              ws.data_ptr(), dc.view(r.LAYER), st()))
            got = host(out).view(np.float16).reshape(B, Hq, r.D)
            launches += 1
            for b, s in enumerate(case.seqs):
                ratio = r.ratios(case, b, got[b])
                worst = max(worst, float(ratio.max()))
                if ratio.max() > 1:
                    h = int(np.argmax(ratio))
                    pytest.fail(f'{case.name} (HPW {hpw} x {chunks} chunks), splits {splits}, {"rectangular" if mode else "ragged"} table, '
                                f'sequence {b} (context {s.ctx}) head {h}: err / bound {ratio[h]:.3f}; '
                                + r.explain(case, b, h, got[b, h], splits))
    print(f'[tq select] {case.name} (HPW {hpw} x {chunks}): {launches} launches, worst err / bound {worst:.3f}')
    return launches, worst


@pytest.mark.parametrize('group', r.GROUPS)
def test_decode_attention_selects(tm, cuda, group):
    _run(tm, r.build(group))


def test_decode_attention_selects_sweep(tm, cuda):
    """context 300, the live sets rolled by 29 positions per sequence: every position is live for one head and dead for another"""
    assert r.coverage_300().all()
    _run(tm, r.build(r.SWEEP_GROUP, True))
