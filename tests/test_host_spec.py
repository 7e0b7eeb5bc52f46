"""Speculative decoding by prompt lookup on the CPU: SpeculativeConfig's validation and refusals, the model-level refusals of
pipeline(), the Pipeline's routing through a fake engine (a plain greedy call speculates; sampling, logits processors, logprobs,
output_logits, per-request configs and streaming do not), the proposer / acceptance rules of tests/spec_reference.py on hand-made
cases, and the new C-ABI symbols.  The kernels and the engine behind the same calls: tests/test_gpu_spec_attention.py,
tests/test_gpu_spec_engine.py."""
import os
import re
import sys

import numpy as np
import pytest

import lmdeploy_amd  # noqa: F401
from lmdeploy_amd import GenerationConfig, SpeculativeConfig, TurbomindEngineConfig, _ffi
from lmdeploy_amd.turbomind import checkpoint
from tests import spec_reference as sr
from tests.test_pipeline_host import VOCAB, FakeEngine, _expect, _tok

P = sys.modules['lmdeploy_amd.pipeline']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- SpeculativeConfig ------------------------------------------------------------------------------------------------------------
def test_speculative_config_fields_and_defaults():
    c = SpeculativeConfig('ngram')
    assert (c.method, c.model, c.num_speculative_tokens, c.prompt_lookup_max, c.prompt_lookup_min) == ('ngram', '', 1, 3, 1)
    c = SpeculativeConfig(method='ngram', num_speculative_tokens=7, prompt_lookup_max=8, prompt_lookup_min=8)
    assert c.num_speculative_tokens == 7 and c.prompt_lookup_max == 8
    assert lmdeploy_amd.SpeculativeConfig is SpeculativeConfig and 'SpeculativeConfig' in lmdeploy_amd.__all__


@pytest.mark.parametrize('method', ['eagle', 'eagle3', 'deepseek_mtp', 'draft_model', ''])
def test_speculative_config_other_methods_need_a_draft_model(method):
    with pytest.raises(NotImplementedError, match='draft model'):
        SpeculativeConfig(method)


@pytest.mark.parametrize('kw', [dict(num_speculative_tokens=0), dict(num_speculative_tokens=8), dict(num_speculative_tokens=-1),
                                dict(prompt_lookup_min=0), dict(prompt_lookup_max=9), dict(prompt_lookup_max=2, prompt_lookup_min=3),
                                dict(num_speculative_tokens=2.0)])
def test_speculative_config_ranges(kw):
    with pytest.raises(ValueError):
        SpeculativeConfig('ngram', **kw)


def test_speculative_config_ngram_has_no_model():
    with pytest.raises(NotImplementedError):
        SpeculativeConfig('ngram', model='some/draft')


# ---- model-level refusals, before any GPU work --------------------------------------------------------------------------------------
def _cfg(**kw):
    base = dict(hidden=256, layers=2, q_heads=4, kv_heads=2, head_dim=128, inter=512, vocab=1024)
    base.update(kw)
    return checkpoint.ModelConfig(**base)


def test_check_speculative_refusals_by_name():
    checkpoint.check_speculative(_cfg(), 8)
    checkpoint.check_speculative(_cfg(head_dim=64), 0)          # runs the flatten + prefill-attention path
    with pytest.raises(NotImplementedError, match='tp > 1'):
        checkpoint.check_speculative(_cfg(), 8, tp=2)
    with pytest.raises(NotImplementedError, match='42'):
        checkpoint.check_speculative(_cfg(), 42)
    with pytest.raises(NotImplementedError, match='sliding window'):
        checkpoint.check_speculative(_cfg(window=40), 8)
    with pytest.raises(NotImplementedError, match='sliding window'):
        checkpoint.check_speculative(_cfg(layer_windows=[0, 128]), 8)
    with pytest.raises(NotImplementedError, match='sinks'):
        checkpoint.check_speculative(_cfg(attn_sinks=1), 8)
    with pytest.raises(NotImplementedError, match='M-RoPE'):
        checkpoint.check_speculative(_cfg(mrope_section=(16, 24, 24)), 8)


class SpecEngine(FakeEngine):
    """FakeEngine + the speculative surface of Engine: a step emits up to k + 1 of the sequence's deterministic tokens"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.spec_k, self.spec_log, self.totals = 0, [], dict(steps=0, drafted=0, accepted=0, emitted=0)

    def set_speculative(self, k, ngram_max=3, ngram_min=1):
        assert self.static is None
        self.spec_k = k
        self.spec_log.append((k, ngram_max, ngram_min))

    def prefill(self, prompts, max_new_tokens):
        if self.spec_k and any(len(p) + max_new_tokens + self.spec_k > self.session_len for p in prompts):
            raise _ffi.TmError(6, 'too long')
        super().prefill(prompts, max_new_tokens)
        self.armed = self.spec_k > 0
        self.counts = [1] * len(prompts)

    def decode(self, n):
        assert not self.armed, 'a batch admitted with speculation armed must not run plain decode steps'
        super().decode(n)

    def decode_spec(self, steps):
        assert self.armed
        for _ in range(steps):
            for b in range(len(self.static)):
                n = min(self.spec_k + 1, self.max_new - self.counts[b])
                if n > 0:
                    self.counts[b] += n
                    self.totals['steps'] += 1
                    self.totals['drafted'] += self.spec_k
                    self.totals['accepted'] += n - 1
                    self.totals['emitted'] += n

    def fetch_spec(self):
        out = np.zeros((len(self.static), self.max_new), np.int32)
        for b, p in enumerate(self.static):
            out[b, :self.counts[b]] = [_tok(p, j) for j in range(self.counts[b])]
        return out, np.asarray(self.counts, np.int32)

    def spec_stats(self):
        return dict(self.totals)


@pytest.fixture
def pipe(monkeypatch):
    monkeypatch.setattr(P, 'Engine', SpecEngine)
    FakeEngine.instances.clear()
    p = P.Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(max_batch_size=2, session_len=64, quant_policy=8),
                   speculative_config=SpeculativeConfig('ngram', num_speculative_tokens=3, prompt_lookup_max=4, prompt_lookup_min=2))
    yield p
    p.close()


def test_pipeline_refusals(monkeypatch):
    monkeypatch.setattr(P, 'Engine', SpecEngine)
    FakeEngine.instances.clear()
    sc = SpeculativeConfig('ngram')
    with pytest.raises(NotImplementedError, match='chat template'):
        P.Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(), chat_template_config=object())
    with pytest.raises(NotImplementedError, match='sliding window'):
        P.Pipeline('synthetic:tiny_window', backend_config=TurbomindEngineConfig(quant_policy=8), speculative_config=sc)
    with pytest.raises(NotImplementedError, match='42'):
        P.Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(quant_policy=42), speculative_config=sc)
    with pytest.raises(NotImplementedError, match='sinks|sliding window'):
        P.Pipeline('synthetic:gpt_oss_20b', backend_config=TurbomindEngineConfig(model_format='hf'), speculative_config=sc)
    with pytest.raises(TypeError):
        P.Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(), speculative_config=dict(method='ngram'))
    assert FakeEngine.instances == []            # every refusal came before an engine existed
    p = P.Pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(max_batch_size=2, session_len=64))
    with pytest.raises(ValueError):
        p.speculative_stats()                    # no speculative_config


def test_greedy_call_speculates(pipe):
    eng = FakeEngine.instances[-1]
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, VOCAB, n).tolist() for n in (5, 9)]
    out = pipe(prompts, GenerationConfig(max_new_tokens=10, ignore_eos=True))
    assert [r.token_ids for r in out] == [_expect(p, 10)[0] for p in prompts]
    assert all(r.finish_reason == 'length' and r.generate_token_len == 10 for r in out)
    assert eng.spec_log == [(3, 4, 2)]
    st = pipe.speculative_stats()
    assert st['emitted'] == st['accepted'] + st['steps'] == 2 * 9 and st['speculated_calls'] == 1 and st['plain_calls'] == 0


def test_stop_id_inside_an_accepted_run(pipe):
    prompt = [3, 1, 4, 1, 5]
    stop = _tok(prompt, 6)                       # steps emit tokens 1-4, 5-8: the stop id sits inside the second run
    assert stop not in [_tok(prompt, j) for j in range(6)]
    r = pipe(prompt, GenerationConfig(max_new_tokens=12, ignore_eos=True, stop_token_ids=[stop]))
    assert r.token_ids == _expect(prompt, 12, {stop})[0] and r.generate_token_len == 6 and r.finish_reason == 'stop'


@pytest.mark.parametrize('kw', [dict(do_sample=True, random_seed=5), dict(logprobs=2), dict(output_logits='generation'),
                                dict(min_new_tokens=2), dict(bad_token_ids=[7])])
def test_other_calls_run_the_plain_path(pipe, kw):
    eng = FakeEngine.instances[-1]
    prompt = [2, 7, 1, 8]
    r = pipe(prompt, GenerationConfig(max_new_tokens=6, ignore_eos=True, **kw))
    assert r.token_ids == _expect(prompt, 6)[0]
    assert eng.spec_log == [(0, 4, 2)]           # switched off for this prefill: decode() ran (SpecEngine.decode asserts it)
    st = pipe.speculative_stats()
    assert st['steps'] == 0 and st['plain_calls'] == 1 and st['speculated_calls'] == 0


def test_continuous_and_streaming_calls_do_not_speculate(pipe):
    eng = FakeEngine.instances[-1]
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, VOCAB, n).tolist() for n in (4, 6, 8)]        # more prompts than batch slots: the scheduler
    g = GenerationConfig(max_new_tokens=5, ignore_eos=True)
    assert [r.token_ids for r in pipe(prompts, g)] == [_expect(p, 5)[0] for p in prompts]
    list(pipe.stream_infer(prompts[:1], g))
    assert [r.token_ids for r in pipe(prompts[:2], [g, g])] == [_expect(p, 5)[0] for p in prompts[:2]]
    assert eng.spec_log == [(0, 3, 1)] * 3 and pipe.speculative_stats()['plain_calls'] == 3


def test_no_room_for_the_verify_rows_decodes_plainly(pipe):
    eng = FakeEngine.instances[-1]
    prompt = list(range(1, 55))                  # 54 + 8 + 3 > 64 >= 54 + 8
    r = pipe(prompt, GenerationConfig(max_new_tokens=8, ignore_eos=True))
    assert r.token_ids == _expect(prompt, 8)[0] and eng.spec_log[-1][0] == 0
    st = pipe.speculative_stats()
    assert st['speculated_calls'] == 0 and st['plain_calls'] == 1


# ---- the proposer and acceptance rules ----------------------------------------------------------------------------------------------
def test_propose_no_match():
    assert sr.ngram_propose([1, 2, 3, 4, 5], 3, 3, 1, 10) == []
    assert sr.ngram_propose([7], 3, 3, 1, 10) == []                       # nothing in front of the suffix


def test_propose_overlap():
    # "a a a a": suffix (a, a, a) matches at i = 0 (i + 3 <= L - 1), the continuation is the last a -- overlap with the suffix is allowed
    assert sr.ngram_propose([9, 9, 9, 9], 3, 3, 1, 10) == [9]
    assert sr.ngram_propose([9, 9, 9, 9], 3, 2, 1, 10) == [9]             # n = 2: latest start i = 1, one token follows
    assert sr.ngram_propose([9, 9, 9, 9], 3, 1, 1, 10) == [9]             # n = 1: latest start i = 2


def test_propose_longest_n_wins():
    h = [1, 2, 3, 50, 9, 3, 60, 1, 2, 3]
    assert sr.ngram_propose(h, 2, 3, 1, 10) == [50, 9]                    # (1, 2, 3) at 0, although (3) alone occurs later, at 5
    assert sr.ngram_propose(h, 2, 1, 1, 10) == [60, 1]                    # n_max = 1: the latest 3


def test_propose_latest_occurrence_wins():
    h = [4, 5, 10, 4, 5, 20, 4, 5]
    assert sr.ngram_propose(h, 1, 2, 2, 10) == [20]
    assert sr.ngram_propose(h, 3, 2, 2, 10) == [20, 4, 5]


def test_propose_continuation_shorter_than_k():
    assert sr.ngram_propose([4, 5, 6, 4, 5], 5, 2, 1, 10) == [6, 4, 5]    # runs into the end of the history
    assert sr.ngram_propose([1, 2, 1], 4, 3, 1, 10) == [2, 1]


def test_propose_cap_by_remaining():
    h = [4, 5, 10, 11, 12, 4, 5]
    assert sr.ngram_propose(h, 3, 2, 1, 10) == [10, 11, 12]
    assert sr.ngram_propose(h, 3, 2, 1, 3) == [10, 11]                    # a step emits n_draft + 1 <= remaining tokens
    assert sr.ngram_propose(h, 3, 2, 1, 2) == [10]
    assert sr.ngram_propose(h, 3, 2, 1, 1) == [] and sr.ngram_propose(h, 3, 2, 1, 0) == []


def test_accept_rule():
    assert sr.accept([5, 6, 7, 8], [5, 6, 7], 3, 10) == [5, 6, 7, 8]      # everything accepted: k + 1 tokens
    assert sr.accept([5, 6, 9, 8], [5, 6, 7], 3, 10) == [5, 6, 9]         # the model's own token replaces the first wrong draft
    assert sr.accept([1, 6, 7, 8], [5, 6, 7], 3, 10) == [1]
    assert sr.accept([5, 6, 7, 8], [5, 6, 7], 1, 10) == [5, 6]            # only n_draft drafts count
    assert sr.accept([5, 6, 7, 8], [5, 6, 7], 0, 10) == [5]
    assert sr.accept([5, 6, 7, 8], [5, 6, 7], 3, 2) == [5, 6]             # cut at remaining
    assert sr.accept([5, 6, 7, 8], [5, 6, 7], 3, 0) == []


def test_simulation_equals_greedy_and_reaches_k_plus_one_in_a_cycle():
    # (the latest earlier occurrence of the suffix lies one period back, so a draft holds min(k, period) tokens: period 9 > 7)
    cyc = list(range(11, 20))
    nxt = lambda h: cyc[(cyc.index(h[-1]) + 1) % 9] if h[-1] in cyc else 11        # noqa: E731
    for k in (1, 3, 7):
        out, per_step, _ = sr.simulate(nxt, [1, 2, 3], nxt([1, 2, 3]), 60, k, 3, 1)
        greedy, h = [], [1, 2, 3]
        for _ in range(60):
            greedy.append(nxt(h))
            h.append(greedy[-1])
        assert out == greedy and sum(per_step) == 59
        assert max(per_step) == k + 1 and per_step[-2] == k + 1              # inside the cycle every draft is right


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('tm_verify_attention', 'tm_verify_attention_workspace', 'tm_spec_propose', 'tm_spec_accept', 'tm_engine_set_speculative',
               'tm_engine_decode_spec', 'tm_engine_verify', 'tm_engine_fetch_spec', 'tm_engine_fetch_spec_logits', 'tm_engine_spec_stats')


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'tm_mi355x.h')).read()
    lib = _ffi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr), f'{name} is not declared in tm_mi355x.h'
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(lib, name)
        res, args = _ffi._SIGNATURES[name]
        n_args = len(re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, hdr, re.S).group(1).split(','))
        assert len(args) == n_args, f'{name}: {len(args)} ctypes arguments for {n_args} declared'
    assert _ffi._SIGNATURES['tm_verify_attention_workspace'][0] is _ffi.c_size_t
    assert lib.tm_verify_attention_workspace(12, 4, 2) == 12 * 4 * 2 * (128 + 2) * 4
    assert lib.tm_verify_attention_workspace(12, 4, 2) == lib.tm_decode_attention_workspace(12, 4, 2)


def test_engine_wrapper_has_the_speculative_methods():
    from lmdeploy_amd.turbomind.engine import Engine
    for m in ('set_speculative', 'decode_spec', 'verify', 'fetch_spec', 'fetch_spec_logits', 'spec_stats'):
        assert callable(getattr(Engine, m))
