"""Sequences of loads, runs and setters on one handle (wfs_batch.h: the batch and the run are reset as a whole; MI355X only).

A handle must compute for a batch what a fresh handle of the same config computes for it, whatever it held before: counts, record
bytes and truth are compared with a fresh engine given that batch alone (tests/test_gpu_step_boundaries.py: _assert_same), never
with the same handle's earlier output except where a test says so.  Every batch is a handful of instructions.

* Kinds in turn.  The config is workloads.mixed_config: the XENONnT TPC with PMT afterpulses and noise.  All three inputs load on it:
  its 494 channels take the photons of chain_s2.npz and the 120 channels that optical_instructions names, and with afterpulse tables
  set both the instruction and the optical batch get afterpulse sets.  (The optical chains' own config, optical_chain_config('main'),
  has 120 channels: wfs_load_photons refuses the chain's photons on channels 120 .. 493 there.)
* A load that fails leaves no batch: the arrays of the failing call are those of the good batch before it with one value spoiled, so
  nothing a wrong implementation ran would be of another size than its buffers.
* A setter that changes the row layout after a complete run leaves the records readable and refuses the rows until the next run.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.helpers import chain_sets, golden, make_engine
from tests.test_gpu_step_boundaries import _assert_same, _result
from wfsim_amd import workloads as W
from wfsim_amd.engine import WfsError
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu

E_STATE = -4          # WFS_E_STATE (include/wfsim_amd.h)
KINDS = ['mixed', 'photons', 'optical', 's2', 'photons']          # instructions, photons, optical, instructions, photons


@functools.lru_cache(maxsize=None)
def _cfg():
    return W.mixed_config(seed=3)


def _instruction_args(eng, ins):
    cfg = _cfg()
    order, key, cluster = schedule(ins, cfg)
    s_ins = ins[order]
    return s_ins, order.astype(np.uint32), cluster, key, instruction_params(s_ins, cfg, Resource(cfg), device_maps=eng.device_maps)


@functools.lru_cache(maxsize=None)
def _photon_args():
    """the arrays replay_chain_on_engine hands to load_photons for chain_s2.npz (every channel of the config is live)"""
    cfg, d = _cfg(), golden('chain_s2.npz')
    assert (np.asarray(cfg['gains'])[d['ph_ch']] > 0).all()
    set_cluster, set_tmin = chain_sets(d, cfg)
    dpe = np.array(d['ph_dpe'], dtype=np.uint8)
    for k in np.where(d['call_has_gains'])[0]:
        dpe[d['call_ph_off'][k]:d['call_ph_off'][k + 1]] = 0
    return set_cluster, set_tmin, np.asarray(d['call_ph_off'], np.int64), np.asarray(d['ph_t'], np.int64), np.asarray(d['ph_ch'], np.int16), \
        np.asarray(d['ph_gain'], np.float64), dpe


def _load(eng, kind):
    if kind == 'photons':
        eng.load_photons(*_photon_args())
    elif kind == 'optical':
        ins, channels, timings = W.optical_instructions(200, 1000.0, 3)
        order, key, cluster = schedule(ins, _cfg())
        eng.load_optical(ins[order], order.astype(np.uint32), cluster, key, channels, timings, int(1e6))
    else:
        eng.load_instructions(*_instruction_args(eng, W.mixed_batch(20) if kind == 'mixed' else W.s2_batch(3, electrons=2000)))


def _load_and_run(eng, kind):
    _load(eng, kind)
    return _result(eng, eng.run())


@functools.lru_cache(maxsize=None)
def _fresh(kind):
    """the batch on a fresh engine; computed once and shared"""
    eng = make_engine(_cfg())
    out = _load_and_run(eng, kind)
    eng.close()
    return out


def test_kinds_in_turn_on_one_handle():
    """an injected batch behind an afterpulse batch, an instruction batch behind an optical one, and back"""
    eng = make_engine(_cfg())
    assert eng.params['enable_pmt_ap']
    for step, kind in enumerate(KINDS):
        got = _load_and_run(eng, kind)
        print(step, kind, got['counts'])
        _assert_same(got, _fresh(kind))
    # afterpulse sets: twice the primary sets for the instruction and the optical batch, none for the photons
    assert _fresh('mixed')['counts']['n_pulse_sets'] == 2 * 20 and _fresh('optical')['counts']['n_pulse_sets'] == 2 * 200
    assert _fresh('photons')['counts']['n_pulse_sets'] == len(_photon_args()[0]) and _fresh('photons')['counts']['n_instructions'] == 0
    eng.close()


@pytest.mark.parametrize('kind', ['mixed', 's2', 'photons', 'optical'])
def test_run_twice(kind):
    """a second run() of the loaded batch gives the bytes of the first (this handle's own), which are the fresh engine's"""
    eng = make_engine(_cfg())
    first = _load_and_run(eng, kind)
    second = _result(eng, eng.run())
    _assert_same(second, first)
    _assert_same(first, _fresh(kind))
    eng.close()


def _assert_no_batch(eng, n):
    with pytest.raises(WfsError, match=f'error {E_STATE}: no batch loaded'):
        eng.run()
    assert eng.lib.wfs_set_instruction_aft(eng._h, C.c_int64(n), C.c_void_p(0)) == E_STATE


def test_failed_photon_load_leaves_no_batch():
    eng = make_engine(_cfg())
    _assert_same(_load_and_run(eng, 'photons'), _fresh('photons'))
    args = list(_photon_args())
    ch = args[4].copy()
    ch[len(ch) // 2] = eng.params['n_tpc']
    args[4] = ch
    with pytest.raises(WfsError, match='photon channel out of range'):
        eng.load_photons(*args)
    _assert_no_batch(eng, 0)
    _assert_same(_load_and_run(eng, 'photons'), _fresh('photons'))
    eng.close()


def test_failed_instruction_load_leaves_no_batch():
    eng = make_engine(_cfg())
    _assert_same(_load_and_run(eng, 'mixed'), _fresh('mixed'))
    s_ins, gid, cluster, key, ip = _instruction_args(eng, W.mixed_batch(20))
    bad = s_ins.copy()
    bad['amp'][7] = -1
    with pytest.raises(WfsError, match='negative amp'):
        eng.load_instructions(bad, gid, cluster, key, ip)
    _assert_no_batch(eng, len(s_ins))
    _assert_same(_load_and_run(eng, 'mixed'), _fresh('mixed'))
    eng.close()


def _copy_rows_rc(eng):
    n = eng.counts['n_rows']
    g, ch = np.zeros(n, np.int32), np.zeros(n, np.int32)
    left, right, off = (np.zeros(n, np.int64) for _ in range(3))
    return eng.lib.wfs_copy_rows(eng._h, *[C.c_void_p(a.ctypes.data) for a in (g, ch, left, right, off)], C.c_int64(n))


def test_view_changed_after_a_complete_run():
    """XENONnT with a zero HE factor and a noise table of 494 columns has no HE rows; a float table of 753 columns (beyond he_first =
    500) brings them: row_slots goes from 494 to 494 + 253.  The debug bit keeps the finished rows, so wfs_copy_rows has rows to decode."""
    cfg = _cfg()
    assert int(cfg.get('high_energy_deamplification_factor', 0)) == 0 and cfg['noise_data'].shape[1] == 494
    noise = np.random.default_rng(8).normal(0.0, 2.2, (3000, 753))
    ins = W.mixed_batch(20)

    def engine_and_run(c):
        eng = make_engine(c)
        eng.set_debug(True)
        eng.load_instructions(*_instruction_args(eng, ins))
        return eng, _result(eng, eng.run())

    eng, before = engine_and_run(cfg)
    he_first = eng.params['he_first']
    assert not eng.emits_he_records and _copy_rows_rc(eng) == 0 and eng.rows()['channel'].max() < he_first
    assert eng.lib.wfs_set_noise_float(eng._h, C.c_void_p(noise.ctypes.data), C.c_int32(noise.shape[0]), C.c_int32(noise.shape[1])) == 0
    assert eng.records().tobytes() == before['records']          # (this handle's own records: they are not decoded with the layout)
    assert _copy_rows_rc(eng) == E_STATE
    after = _result(eng, eng.run())
    assert _copy_rows_rc(eng) == 0 and eng.rows()['channel'].max() >= he_first
    fresh, want = engine_and_run(dict(cfg, noise_data=noise))
    assert fresh.emits_he_records
    _assert_same(after, want)
    assert after['records'] != before['records']
    # the switch set to the value it has: the layout is the same, the last run stays readable
    assert eng.lib.wfs_set_sum_signal(eng._h, C.c_int32(0)) == 0
    assert _copy_rows_rc(eng) == 0 and eng.records().tobytes() == want['records']
    eng.close()
    fresh.close()
