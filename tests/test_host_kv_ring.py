"""KV block ring of sliding-window models, host side (lmdeploy_amd/csrc/scheduler.h), driven on the CPU through
tm_sched_* and tm_kv_ring_blocks exactly as the engine drives it: with a ring of R blocks a request owns
min(ceil((prompt + max_new) / 64), R) blocks, so requests whose whole context exceeds the pool are accepted, admitted and run side by
side; ring_blocks = 0 is the scheduler without the feature."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from lmdeploy_amd import _ffi

FINISH, CANCEL, INVALID, OOM = 7, 8, 1, 11


class Sched:
    def __init__(self, max_batch, num_blocks, session_len, ring=None):
        self.lib = _ffi.load()
        self.h = C.c_void_p()
        self.pool = num_blocks
        self.ids = []
        _ffi.check(self.lib.tm_sched_create(C.byref(self.h), max_batch, num_blocks, session_len))
        if ring is not None:
            _ffi.check(self.lib.tm_sched_set_ring(self.h, ring))

    def submit(self, n, max_new, eos=-1):
        ids = np.arange(n, dtype=np.int32)
        rid = C.c_int64(0)
        rc = self.lib.tm_sched_submit(self.h, ids.ctypes.data, n, max_new, eos, C.byref(rid))
        if rc == 0:
            self.ids.append(rid.value)
        return rc, rid.value

    def admit(self, budget=1 << 30):
        ids, slots, n = (C.c_int64 * 64)(), (C.c_int * 64)(), C.c_int(0)
        _ffi.check(self.lib.tm_sched_admit(self.h, budget, ids, slots, 64, C.byref(n)))
        return [(ids[i], slots[i]) for i in range(n.value)]

    def on_token(self, slot, tok):
        f = C.c_int(0)
        _ffi.check(self.lib.tm_sched_on_token(self.h, slot, tok, C.byref(f)))
        return bool(f.value)

    def cancel(self, rid):
        s = C.c_int(-1)
        return self.lib.tm_sched_cancel(self.h, rid, C.byref(s)), s.value

    def blocks(self, rid):
        nb = C.c_int(-1)
        _ffi.check(self.lib.tm_sched_query(self.h, rid, None, None, None, C.byref(nb)))
        return nb.value

    def admit_ready(self):
        r = C.c_int(0)
        _ffi.check(self.lib.tm_sched_admit_ready(self.h, C.byref(r)))
        return bool(r.value)

    def counts(self):
        a, w, f = C.c_int(0), C.c_int(0), C.c_int(0)
        _ffi.check(self.lib.tm_sched_counts(self.h, C.byref(a), C.byref(w), C.byref(f)))
        return a.value, w.value, f.value

    def conserved(self):
        """free + owned == pool"""
        return self.counts()[2] + sum(self.blocks(r) for r in self.ids) == self.pool

    def __del__(self):
        self.lib.tm_sched_destroy(self.h)


def test_requests_beyond_the_pool_run_side_by_side():
    s = Sched(max_batch=4, num_blocks=8, session_len=4096, ring=3)
    a, b = s.submit(300, 20)[1], s.submit(300, 20)[1]            # 5 blocks whole-context each: 10 > 8
    assert s.admit() == [(a, 0), (b, 1)]
    assert s.blocks(a) == 3 and s.blocks(b) == 3
    assert s.counts() == (2, 0, 2) and s.conserved()


def test_small_request_owns_what_it_needs():
    s = Sched(max_batch=4, num_blocks=8, session_len=4096, ring=3)
    a, b, c = s.submit(100, 28)[1], s.submit(10, 10)[1], s.submit(129, 63)[1]      # 2, 1 and exactly 3 blocks
    assert [x[0] for x in s.admit()] == [a, b, c]
    assert (s.blocks(a), s.blocks(b), s.blocks(c)) == (2, 1, 3)
    assert s.counts() == (3, 0, 2) and s.conserved()


def test_conservation_over_a_call_sequence():
    s = Sched(max_batch=2, num_blocks=8, session_len=4096, ring=3)
    assert s.conserved()
    r = [s.submit(n, m)[1] for n, m in ((300, 20), (1000, 3), (70, 2), (2000, 100), (5, 1))]
    assert s.conserved() and s.counts() == (0, 5, 8)
    assert s.admit() == [(r[0], 0), (r[1], 1)] and s.conserved() and s.counts()[2] == 2
    assert s.admit_ready() is False                              # no slot
    for t in range(2):
        assert not s.on_token(1, t) and s.conserved()
    assert s.on_token(1, 9) and s.conserved()                    # r[1] finished by length: its ring returns
    assert s.counts() == (1, 3, 5) and s.blocks(r[1]) == 0
    assert s.admit_ready() is True
    assert s.admit() == [(r[2], 1)] and s.blocks(r[2]) == 2 and s.conserved()
    assert s.cancel(r[0]) == (0, 0) and s.conserved() and s.counts() == (1, 2, 6)
    assert s.admit() == [(r[3], 0)] and s.blocks(r[3]) == 3 and s.conserved()      # 33 blocks whole-context
    assert s.cancel(r[4]) == (0, -1) and s.conserved()           # cancelled while waiting
    assert s.lib.tm_sched_abort_all(s.h, 5) == 0
    assert s.conserved() and s.counts() == (0, 0, 8)
    assert all(s.blocks(x) == 0 for x in r)


def test_a_request_larger_than_the_pool_is_accepted():
    s = Sched(max_batch=2, num_blocks=8, session_len=4096, ring=3)
    rc, rid = s.submit(600, 40)                                  # 10 blocks whole-context > 8
    assert rc == 0
    assert s.admit() == [(rid, 0)] and s.blocks(rid) == 3
    # a ring larger than the pool still can never fit
    s2 = Sched(max_batch=2, num_blocks=2, session_len=4096, ring=3)
    assert s2.submit(600, 40)[0] == OOM
    assert s2.submit(100, 28)[0] == 0                            # 2 blocks


def test_ring_off_is_the_scheduler_without_it():
    """ring_blocks = 0 (explicitly, or never set): the counts of tests/test_scheduler.py"""
    for ring in (None, 0):
        s2 = Sched(max_batch=2, num_blocks=2, session_len=1000, ring=ring)
        assert s2.submit(100, 100)[0] == OOM                     # test_submit_status_codes
        s = Sched(max_batch=2, num_blocks=10, session_len=4096, ring=ring)
        r = [s.submit(n, m)[1] for n, m in ((100, 28), (64, 1), (10, 10), (300, 20))]   # test_fifo_admission_slots_and_blocks
        assert s.admit() == [(r[0], 0), (r[1], 1)]
        assert s.counts() == (2, 2, 6) and s.blocks(r[0]) == 2 and s.blocks(r[1]) == 2
        assert s.on_token(1, 7) is True and s.counts() == (1, 2, 8)
        assert s.admit() == [(r[2], 1)] and s.admit() == []
        for t in range(28):
            s.on_token(0, t)
        assert s.admit() == [(r[3], 0)] and s.blocks(r[3]) == 5
        assert s.counts() == (2, 0, 4) and s.conserved()
        s8 = Sched(max_batch=4, num_blocks=8, session_len=4096, ring=ring)
        a, b = s8.submit(300, 20)[1], s8.submit(300, 20)[1]      # 5 + 5 > 8: one at a time
        assert s8.admit() == [(a, 0)] and s8.blocks(a) == 5 and s8.admit_ready() is False
        assert s8.submit(600, 40)[0] == OOM


def test_set_ring_only_before_the_first_submit():
    s = Sched(max_batch=2, num_blocks=8, session_len=4096)
    assert s.lib.tm_sched_set_ring(s.h, 4) == 0
    assert s.lib.tm_sched_set_ring(s.h, 3) == 0                  # still nothing submitted
    assert s.lib.tm_sched_set_ring(s.h, -1) == INVALID
    assert s.submit(0, 5)[0] == INVALID                          # a refused submit is a submit nobody saw
    assert s.lib.tm_sched_set_ring(s.h, 3) == 0
    rid = s.submit(300, 20)[1]
    assert s.lib.tm_sched_set_ring(s.h, 5) == INVALID
    assert s.lib.tm_sched_set_ring(s.h, 0) == INVALID
    assert s.admit() == [(rid, 0)] and s.blocks(rid) == 3        # the ring set before the submit holds


def test_ring_size():
    """R = ceil((W - 1 + C) / 64) + 1: the keys [hist - W + 1, hist + q), q <= C, are at most W - 1 + C tokens and a run of n tokens
    touches at most ceil((n - 1) / 64) + 1 <= ceil(n / 64) + 1 blocks.  (40, 64): 103 -> 2 + 1; (64, 64): 127 -> 2 + 1; (65, 64): 128 ->
    2 + 1; (66, 64): 129 -> 3 + 1; (4096, 8192): 12287 -> 192 + 1."""
    lib = _ffi.load()

    def ring(w, c):
        r = C.c_int(-1)
        _ffi.check(lib.tm_kv_ring_blocks(w, c, C.byref(r)))
        return r.value

    assert {(w, c): ring(w, c) for w, c in ((40, 64), (64, 64), (65, 64), (66, 64), (4096, 8192))} == {
        (40, 64): 3, (64, 64): 3, (65, 64): 3, (66, 64): 4, (4096, 8192): 193}
    for w, c in ((1, 1), (1, 64), (40, 64), (100, 37), (4096, 8192), (777, 1000)):
        r = ring(w, c)
        assert r == -(-(w - 1 + c) // 64) + 1
        assert r * 64 >= w + 64                                  # decode: the window and the block being written
        # the widest run of resident keys, at its worst alignment, fits R distinct blocks
        n = w - 1 + c
        assert max((s + n - 1) // 64 - s // 64 + 1 for s in range(64)) <= r
    r = C.c_int(0)
    assert lib.tm_kv_ring_blocks(0, 64, C.byref(r)) == INVALID and lib.tm_kv_ring_blocks(40, 0, C.byref(r)) == INVALID


def test_synthetic_tiny_window_is_tiny_with_a_window():
    from lmdeploy_amd.pipeline import SYNTHETIC
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.engine import make_model_config
    tiny, win = dict(SYNTHETIC['tiny']), dict(SYNTHETIC['tiny_window'])
    assert win.pop('window') == 40 and 'window' not in tiny
    assert {k: v for k, v in win.items() if k != 'rope'} == {k: v for k, v in tiny.items() if k != 'rope'}
    assert vars(win['rope']) == vars(tiny['rope'])
    assert make_model_config(checkpoint.ModelConfig(**SYNTHETIC['tiny_window']), 0).attn_window == 40


def test_ring_scheduler_under_sanitizers(tmp_path):
    """the random call stream of tests/cpp/scheduler_sanitizer.cpp on a scheduler with a ring and a pool smaller than most requests'
    whole context (tests/cpp/scheduler_ring_sanitizer.cpp), AddressSanitizer + UndefinedBehaviorSanitizer, stand-alone on the CPU"""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    src = os.path.join(os.path.dirname(__file__), 'cpp', 'scheduler_ring_sanitizer.cpp')
    exe = str(tmp_path / 'sched_ring_san')
    build = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe, src],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    for args in (['1'], ['2', 'abort'], ['3']):
        run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.startswith('ok seed'), run.stdout + run.stderr
