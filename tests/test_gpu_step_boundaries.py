"""Step boundaries and fill groups (wfs_engine.hip read_scal, FillGroup): the way a size reaches the host and the number of
dispatches that clear buffers must not change a byte of what a step computes.

* Both modes, same bytes: every batch runs on an engine created under WFS_HOST_SYNC=copy (copy + synchronise at every boundary) and
  on one created without it (k_publish into the mapped scalar block, the host spins on the sequence word).  The batches are the
  smallest that cross every boundary of wfs_run and wfs_load_optical.
* One handle, changing sizes: mixed_batch(20), then (3), then (40) -- 20, 2 and 40 instructions, mixed_batch makes S1 + S2 pairs -- on
  one engine against a fresh engine each; the shrinking step is the one a fill group sized from a stale count, or a sequence word
  out of step, would break.

records(), counts and truth() are compared exactly, as the two modes must give them.  (The mean and the spread of the electron times,
truth()[1][:, 1] and [:, 4], are quotients of sums made by double-precision atomics; on these batches four fresh engines in one
mode gave identical bits, and so did the two modes, so nothing is relaxed.)

The default engine must really have published: the profiled step lists one "k_publish" entry per boundary that did (none for one
that fell back to the copy), so its count is the number of boundaries the batch crosses, and zero under WFS_HOST_SYNC=copy.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from wfsim_amd import workloads as W
from wfsim_amd.engine import Engine
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _host_sync(mode):
    """WFS_HOST_SYNC as wfs_create reads it: 'copy', or None for the default (unset)"""
    old = os.environ.pop('WFS_HOST_SYNC', None)
    if mode is not None:
        os.environ['WFS_HOST_SYNC'] = mode
    try:
        yield
    finally:
        os.environ.pop('WFS_HOST_SYNC', None)
        if old is not None:
            os.environ['WFS_HOST_SYNC'] = old


def _engine(cfg, mode):
    with _host_sync(mode):
        return Engine(cfg, Resource(cfg))


def _result(eng, counts):
    acc, ts = eng.truth()
    return dict(counts=dict(counts), records=eng.records().tobytes(), acc=acc, ts=ts)


def _run_generated(eng, cfg, ins, gid0=0):
    order, key, cluster = schedule(ins, cfg)
    s_ins = ins[order]
    ip = instruction_params(s_ins, cfg, Resource(cfg), device_maps=eng.device_maps)
    eng.load_instructions(s_ins, (gid0 + order).astype(np.uint32), cluster, key, ip)
    return _result(eng, eng.run())


def _run_optical(eng, cfg):
    ins, channels, timings = W.optical_instructions(200, 1000.0, 3)
    order, key, cluster = schedule(ins, cfg)
    eng.load_optical(ins[order], order.astype(np.uint32), cluster, key, channels, timings, int(1e6))
    return _result(eng, eng.run())


MIXED = {20: 0, 3: 1000, 40: 2000}       # instructions asked of mixed_batch -> first_gid (disjoint)


@functools.lru_cache(maxsize=None)
def _fresh(case, mode):
    """one batch on a fresh engine; computed once per (batch, mode) and shared"""
    if case == 's2':
        cfg = W.bench_config(seed=3)
        return _run_generated(_engine(cfg, mode), cfg, W.s2_batch(3, electrons=2000))
    if case == 's2_ap':
        cfg = W.bench_config(seed=3, pmt_afterpulses=True)
        return _run_generated(_engine(cfg, mode), cfg, W.s2_batch(3, electrons=2000))
    if case == 'nveto':
        cfg = W.nveto_config(seed=31)
        return _run_optical(_engine(cfg, mode), cfg)
    n = int(case[len('mixed'):])
    cfg = W.mixed_config(seed=3)
    return _run_generated(_engine(cfg, mode), cfg, W.mixed_batch(n, MIXED[n]), MIXED[n])


def _assert_same(a, b):
    assert a['counts'] == b['counts']
    assert a['counts']['n_records'] > 0 and len(a['records']) == 244 * a['counts']['n_records']
    assert a['records'] == b['records']
    assert np.array_equal(a['acc'], b['acc'])
    for col in (1, 4):
        d = np.abs(a['ts'][:, col] - b['ts'][:, col])
        print(f'truth timing column {col}: largest difference {np.nanmax(d) if d.size else 0.0!r}')
    assert np.array_equal(a['ts'], b['ts'], equal_nan=True)


@pytest.mark.parametrize('case', ['s2', 's2_ap', 'mixed20', 'nveto'])
def test_both_modes_same_bytes(case):
    """s2: tile path, the boundaries of gen_electrons, run_geometry and both of run_records; s2_ap: the one of gen_afterpulses on
    top; mixed20: block generator, order repair (gen_order), resident rows, noise; nveto: the one of wfs_load_optical"""
    _assert_same(_fresh(case, 'copy'), _fresh(case, None))


def test_one_handle_changing_sizes():
    cfg = W.mixed_config(seed=3)
    eng = _engine(cfg, None)
    for n in (20, 3, 40):
        got = _run_generated(eng, cfg, W.mixed_batch(n, MIXED[n]), MIXED[n])
        _assert_same(got, _fresh(f'mixed{n}', None))


@pytest.mark.parametrize('case,boundaries', [('s2', 4), ('s2_ap', 6), ('nveto', 3)])
def test_default_mode_publishes_every_boundary(case, boundaries):
    """boundaries inside wfs_run: gen_electrons, run_geometry and the two of run_records (s2); with PMT afterpulses gen_afterpulses
    and, because afterpulse tiles are put into generation order, gen_order on top (s2_ap); an optical batch has no generation (its
    load-time boundary lies outside the profiled step)"""
    for mode, expect in (('copy', 0), (None, boundaries)):
        if case == 'nveto':
            cfg = W.nveto_config(seed=31)
            eng = _engine(cfg, mode)
            eng.set_profiling(True)
            _run_optical(eng, cfg)
        else:
            cfg = W.bench_config(seed=3, pmt_afterpulses=(case == 's2_ap'))
            eng = _engine(cfg, mode)
            eng.set_profiling(True)
            _run_generated(eng, cfg, W.s2_batch(3, electrons=2000))
        times = eng.kernel_times()
        assert times.get('k_publish', (0.0, 0))[1] == expect, (mode, times)
        assert 'fills_geometry' in times and 'fills_rows' in times
