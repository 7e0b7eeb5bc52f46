"""bench.py's two modes on a small configuration: a plain run does only what `value` needs (set-up, warm-up, the timed steps, the JSON
line), `--full` adds the measurements beyond it after the timed steps (eager per-kernel profile, roofline objects, the continuation to
1024 generated tokens).  The rocprofv3 child passes and the CPU baseline stay off here (--no-traffic, --no-cpu-baseline): they only
add to what the --full line carries."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--gpus', '1', '--steps', '4', '--warmup', '2', '--layers', '2', '--batch', '8', '--prompt-len', '96', '--tune', '0']
EXTRAS = ('kernel_ms_per_step', 'roofline', 'gemm_roofline', 'value_1k_out', 'value_full_run', 'cpu_baseline')


def _line(extra):
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + SMALL + extra, env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=400)
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = pr.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith('{'), lines[:3]
    d = json.loads(lines[0])
    assert d['steps'] == 4 and d['warmup'] == 2 and d['unit'] == 'tokens/s' and d['higher_is_better'] is True
    assert d['value'] > 0 and d['value'] == pytest.approx(8 * 1e3 / d['ms_per_step'], rel=5e-3)
    return d


@pytest.mark.timeout(450)
def test_plain_run_carries_no_extras(cuda):
    d = _line([])
    assert not set(EXTRAS) & set(d), sorted(set(EXTRAS) & set(d))
    assert set(d['config']['gemm_tilings']) == {'w_qkv', 'wo', 'w1w3', 'w2'} and d['ttft_p50_ms'] > 0


@pytest.mark.timeout(450)
def test_full_run_adds_the_extras(cuda):
    d = _line(['--full', '--no-traffic', '--no-cpu-baseline'])
    assert d['kernel_ms_per_step']['attention'] > 0 and d['kernel_ms_per_step']['gemm_qkv'] > 0
    assert d['roofline']['in_graph_trace'] == 'skipped' and d['gemm_roofline']['achieved'] > 0
    assert d['value_full_run']['steps'] == 1024 - (1 + 2 + 8) and d['value_1k_out'] == d['value_full_run']['value'] > 0
    assert 'cpu_baseline' not in d
