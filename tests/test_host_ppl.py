"""Host logic of Pipeline.get_ppl on the CPU: the Pipeline class driven through a fake engine with a deterministic `score` (the
fake of tests/test_pipeline_host.py plus scoring), so that input forms, grouping by max_batch_size, the split-and-retry on an
out-of-blocks refusal, the float64 mean and the refusals are covered without a GPU.  The real engine behind the same call is
covered by tests/test_gpu_ppl.py."""
import sys

import numpy as np
import pytest

import lmdeploy_amd  # noqa: F401  (loads lmdeploy_amd.pipeline into sys.modules)
from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, _ffi
from tests.test_pipeline_host import FakeEngine

P = sys.modules['lmdeploy_amd.pipeline']


def _nll(seq):
    """per-token NLL of the fake: a pure function of (previous token, token, position), fp32 like the engine's"""
    s = np.asarray(seq, np.int64)
    return ((s[:-1] * 7 + s[1:] * 13 + np.arange(len(s) - 1)) % 97 / 17.0 + 0.01).astype(np.float32)


class ScoringEngine(FakeEngine):
    max_tokens = None     # > 0: a score call whose inputs hold more tokens than this is refused with TM_OOM

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.score_calls = []

    def score(self, seqs):
        assert len(seqs) <= self.B and self.static is None
        self.score_calls.append([list(map(int, s)) for s in seqs])
        if self.max_tokens is not None and sum(len(s) for s in seqs) > self.max_tokens:
            raise _ffi.TmError(11, 'out of KV cache blocks')
        return [_nll(s) for s in seqs]


@pytest.fixture
def pipe(monkeypatch):
    monkeypatch.setattr(P, 'Engine', ScoringEngine)
    monkeypatch.setattr(ScoringEngine, 'max_tokens', None)
    FakeEngine.instances.clear()
    p = P.Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(max_batch_size=3, session_len=64, quant_policy=8))
    yield p
    p.close()


def _mean(seq):
    return float(np.cumsum(_nll(seq), dtype=np.float64)[-1] / (len(seq) - 1))


def test_get_ppl_flat_list_is_one_input(pipe):
    seq = [5, 9, 1, 44, 3]
    res = pipe.get_ppl(seq)
    assert isinstance(res, list) and len(res) == 1 and type(res[0]) is float
    assert res[0] == _mean(seq)


def test_get_ppl_order_and_groups(pipe):
    rng = np.random.default_rng(1)
    seqs = [rng.integers(0, 1024, n).tolist() for n in (2, 17, 5, 40, 3, 9, 30, 2)]
    res = pipe.get_ppl(seqs)
    assert res == [_mean(s) for s in seqs]          # input order, the exact float64 mean
    calls = FakeEngine.instances[-1].score_calls
    assert [len(c) for c in calls] == [3, 3, 2]      # groups of at most max_batch_size, in input order
    assert [s for c in calls for s in c] == seqs


def test_get_ppl_mean_is_float64_sum(pipe):
    seq = list(range(1, 60))
    nll = _nll(seq)
    acc = 0.0
    for v in nll:                                     # position order, float64
        acc += float(v)
    assert pipe.get_ppl([seq])[0] == acc / (len(seq) - 1)


def test_get_ppl_oom_halves_group(pipe, monkeypatch):
    monkeypatch.setattr(ScoringEngine, 'max_tokens', 40)
    seqs = [[i + 1] * 15 for i in range(3)] + [[7] * 12]
    res = pipe.get_ppl(seqs)
    assert res == [_mean(s) for s in seqs]
    calls = [[len(s) for s in c] for c in FakeEngine.instances[-1].score_calls]
    # [15, 15, 15] refused -> [15, 15] + [15]; then [12]
    assert calls == [[15, 15, 15], [15, 15], [15], [12]]


def test_get_ppl_single_input_that_does_not_fit(pipe, monkeypatch):
    monkeypatch.setattr(ScoringEngine, 'max_tokens', 10)
    with pytest.raises(ValueError):
        pipe.get_ppl([[1] * 20])


def test_get_ppl_other_engine_errors_propagate(pipe, monkeypatch):
    def bad(self, seqs):
        raise _ffi.TmError(1, 'invalid')
    monkeypatch.setattr(ScoringEngine, 'score', bad)
    with pytest.raises(_ffi.TmError):
        pipe.get_ppl([[1, 2, 3]])


def test_get_ppl_refusals(pipe):
    with pytest.raises(AssertionError):
        pipe.get_ppl((1, 2, 3))                       # not a list
    with pytest.raises(AssertionError):
        pipe.get_ppl([1])
    with pytest.raises(AssertionError):
        pipe.get_ppl([[1, 2], [3]])
    with pytest.raises(ValueError):
        pipe.get_ppl([[1, 2], [1] * 64])              # len >= session_len
    assert pipe.get_ppl([[1] * 63]) == [_mean([1] * 63)]
    assert FakeEngine.instances[-1].score_calls == [[[1] * 63]]   # the refused calls never reached the engine


def test_get_ppl_tp_refused_before_the_engine(pipe):
    pipe.backend_config.tp = 2
    with pytest.raises(NotImplementedError):
        pipe.get_ppl([[1, 2, 3]])
    assert FakeEngine.instances[-1].score_calls == []


def test_return_ppl_still_refused():
    with pytest.raises(NotImplementedError, match='get_ppl'):
        GenerationConfig(return_ppl=True)
