"""Every device buffer of a handle goes back when the handle is destroyed (wfs_devbuf.h: a DevBuf frees itself; ~wfs_handle owns the
rest; MI355X only).

The measure is wfs_device_allocations: the library's own count of live buffers and their bytes, process-wide.  It is exact, where the
card's free-memory figure moves under other processes.  Every test compares with the figure it recorded at its start, not with zero: an
engine that a fixture elsewhere in the session keeps open does not matter (unreachable ones are collected first, so that none of
them goes in the middle of a test)."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests.helpers import (OPTICAL_CHAINS, ap_tables_from_golden, golden, make_engine, optical_chain_config, replay_chain_on_engine,
                           with_fma)
from tests.test_gpu_pattern_maps import instructions
from tests.test_gpu_scalar_maps import point_map_config
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.engine import device_allocations
from wfsim_amd.itp_map import InterpolatingMap
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu


@pytest.fixture
def baseline():
    gc.collect()
    return device_allocations()


def test_destroy_returns_every_buffer(baseline):
    """the sum channel on: its six buffers (sum_lo .. sum_chunk_off) were the ones wfs_destroy's list had missed"""
    cfg = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20, emit_sum_signal=True), False)
    d = golden('chain_he.npz')         # the chain of tests/test_gpu_sum_signal.py
    out = []
    for cycle in range(2):
        eng = make_engine(cfg)
        assert eng.emits_sum_records
        replay_chain_on_engine(eng, d, cfg, debug=False)
        s = eng.sum_signal()
        assert len(s['group']) > 0 and len(s['data']) > 0
        out.append((eng.records().tobytes(), {k: v.tobytes() for k, v in s.items()}))
        live = device_allocations()
        assert live[0] > baseline[0] and live[1] > baseline[1]
        eng.close()
        assert device_allocations() == baseline, cycle
    assert len(out[0][0]) > 0 and out[0] == out[1]


def _generated_with_tables_and_maps():
    """a generator batch under PMT-afterpulse tables (ApElem) and point-list pattern maps (PatternMap: values, points, cell index);
    a grid and a spline registered as scalar maps (ScalarMap) and evaluated"""
    cfg = point_map_config(0, seed=11, s2_secondary_sc_gain=30.0, enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap_tables_from_golden())
    res = Resource(cfg)
    eng = make_engine(cfg, resource=res)
    assert eng.device_maps == {'s1', 's2'} and eng.params['enable_pmt_ap']
    grid = InterpolatingMap(dict(coordinate_system=[['x', [0, 1, 3]], ['y', [0, 1, 3]]], map=np.arange(9.0).reshape(3, 3)))
    r, z = np.linspace(0, 67, 8), np.linspace(-150, 0, 9)
    spline = InterpolatingMap(dict(coordinate_system=[['r', [0, 67, 8]], ['z', [-150, 0, 9]]], map=np.cos(r / 40)[:, None] + 0.001 * z[None, :]),
                              method='RectBivariateSpline')
    ids = [eng.register_scalar_map(m)[0] for m in (grid, spline)]
    assert len(set(ids)) == 2
    for mid, pos in zip(ids, ([[0.3, 0.4], [0.9, 0.1]], [[10.0, -20.0], [50.0, -100.0]])):
        assert np.all(np.isfinite(eng.eval_scalar_map(mid, np.asarray(pos))))
    ins = instructions(20, 40)
    order, key, cluster = schedule(ins, cfg)
    s_ins = ins[order]
    ip = instruction_params(s_ins, cfg, res, device_maps=eng.device_maps)
    assert np.all(ip['cdf_row'] == -1)
    eng.load_instructions(s_ins, order.astype(np.uint32), cluster, key, ip)
    assert eng.run()['n_records'] > 0
    return eng


def _injected_photons():
    cfg = xenonnt_test_config()
    eng = make_engine(cfg)
    assert replay_chain_on_engine(eng, golden('chain_s2.npz'), cfg, debug=False)['n_records'] > 0
    return eng


def _optical():
    d = golden(OPTICAL_CHAINS['main'])
    cfg = optical_chain_config('main', seed=61)
    ins = d['instructions']
    order, key, cluster = schedule(ins, cfg)
    eng = make_engine(cfg)
    eng.load_optical(ins[order], order.astype(np.uint32), cluster, key, d['channels'], d['timings'], int(d['cutoff']))
    assert eng.run()['n_records'] > 0
    return eng


@pytest.mark.parametrize('make', [_generated_with_tables_and_maps, _injected_photons, _optical])
def test_destroy_after_every_input_kind(baseline, make):
    eng = make()
    assert device_allocations()[0] > baseline[0]
    eng.close()
    assert device_allocations() == baseline


def test_user_tables_replaced(baseline):
    """wfs_set_delay_models twice: one table buffer per table (x_alias) beside buffers whose number does not depend on the tables, so
    the live count may move by the difference of the table counts at the most -- the tables of the first call are gone"""
    eng = make_engine(xenonnt_test_config())

    def set_tables(n):
        base, vmin = np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
        off = 3 * np.arange(n + 1, dtype=np.int64)
        pmf = np.tile([0.25, 0.5, 0.25], n)
        eng._check(eng.lib.wfs_set_delay_models(eng._h, C.c_int32(n), *[C.c_void_p(a.ctypes.data) for a in (base, off, pmf, vmin)]))
        return device_allocations()[0]

    before = device_allocations()[0]
    first = set_tables(5)
    assert first >= before + 5
    second = set_tables(2)
    assert second <= first + (2 - 5)
    third = set_tables(7)
    assert third <= second + (7 - 2)
    eng.close()
    assert device_allocations() == baseline
