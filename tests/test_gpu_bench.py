"""bench.py on a small batch: a plain run prints only the headline line, --dump-outputs writes the last timed step's outputs
identically from run to run, --full adds the side measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--instructions', '20'] + list(args),
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    lines, dumps = [], []
    for k in range(2):
        d = str(tmp_path / f'run{k}')
        lines.append(_bench('--steps', '3', '--warmup', '1', '--dump-outputs', d))
        dumps.append(_load(d))
    for line in lines:
        assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
        assert line['unit'] == 'photoelectrons/s' and line['higher_is_better'] is True and line['dtype'] == 'f64'
        assert 'roofline' not in line and 'cpu_baseline' not in line
    a, b = dumps
    assert sorted(a) == sorted(b) and {'counts', 'records_data', 'records_time', 'truth'} <= set(a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    n = lines[0]['config']['records_per_step']
    assert n > 0 and np.array_equal(a['records_index'], np.arange(n)) and a['records_data'].shape == (n, 110)
    assert a['channel_records'].sum() == n
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        if name == 'truth_timing':          # electron-time mean and spread: sums of floating-point atomics
            np.testing.assert_allclose(a[name], b[name], rtol=1e-9, equal_nan=True)
        else:
            assert a[name].tobytes() == b[name].tobytes(), name


def test_full_run_adds_the_side_measurements():
    line = _bench('--steps', '2', '--warmup', '1', '--full', '--cpu-sample', '2', '--no-copy-ceiling')
    assert line['steps'] == 2 and line['ms_per_step'] > 0
    assert line['roofline']['kernels_ms'] and line['config']['ms_per_step_incl_d2h_of_records'] > 0
    assert line['cpu_baseline']['value'] > 0
