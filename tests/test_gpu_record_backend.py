"""The shared record back end (order_records, pack_finished_rows, two_step of wfs_engine.hip): a sorted run, a lone-hit pass
and an overlay pass launch what they launched before the back end was shared, and one scratch buffer serves all three in any order.

The (name, launches) lists below were recorded by running ``_first_order`` of this file on the commit before the change (the library of
that commit under this file, profiles/record_backend_parent.json holds them); they are not taken from the code under test.  The
records of the passes are held to the restatements of tests/lone_hits.py and tests/overlay.py, and those of the second ordering, in
which the scratch buffer grows inside each kind of pass, to the bytes of the first.
"""
import json
import os

import numpy as np
import pytest

from tests import dark_counts as DK
from tests import lone_hits as LH
from tests import overlay as OV
from tests.helpers import host_tables, make_engine, with_fma
from tests.test_gpu_lone_hits import _base, _lone_of, _seam_windows
from tests.test_gpu_noise_model import _photon_sets
from tests.test_lone_hits_cpu import NEAR_LIMIT, SEED
from wfsim_amd import dark_counts as DC
from wfsim_amd.config import kernel_params, xenonnt_test_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS = (15000, 115000, 116000)          # s0, s1, s_limit of the lone pass behind the run (the pass of the seam tests)

# (name, launches) of wfs_kernel_times on one handle with profiling on: after the sorted run, after the lone pass behind it (the
# entries of the pass come behind the run's), after the overlay behind that.  Recorded on the parent commit.
KERNEL_TIMES = {
    'run': [('fills_input', 1), ('k_scan_reduce', 4), ('k_scan_spine', 4), ('k_scan_down', 4), ('fills_geometry', 1),
            ('k_tile_geom', 1), ('k_groups', 1), ('k_tile_rows', 1), ('k_group_final', 1), ('k_row_len', 1), ('k_publish', 3),
            ('fills_pulses', 1), ('k_tile_desc', 1), ('k_pulse_tiny', 1), ('k_pulse_wave', 1), ('fills_rows', 1), ('k_row_desc', 1),
            ('k_truth_reduce', 1), ('k_zle', 1), ('k_rec_keys', 1), ('record_sort', 1), ('k_invert_perm', 1), ('k_pack_desc', 1),
            ('k_pack', 1)],
    'lone': [('fills_input', 1), ('k_scan_reduce', 8), ('k_scan_spine', 8), ('k_scan_down', 8), ('fills_geometry', 1),
            ('k_tile_geom', 1), ('k_groups', 1), ('k_tile_rows', 1), ('k_group_final', 1), ('k_row_len', 1), ('k_publish', 3),
            ('fills_pulses', 1), ('k_tile_desc', 1), ('k_pulse_tiny', 1), ('k_pulse_wave', 1), ('fills_rows', 1), ('k_row_desc', 1),
            ('k_truth_reduce', 1), ('k_zle', 1), ('k_rec_keys', 2), ('record_sort', 1), ('k_invert_perm', 2), ('k_pack_desc', 2),
            ('k_pack', 1), ('k_lone_scan', 1), ('k_lone_rows', 1), ('fills_lone', 1), ('k_lone_desc', 1), ('k_row_empty', 1),
            ('k_pack_res', 1)],
    'overlay': [('fills_input', 1), ('k_scan_reduce', 8), ('k_scan_spine', 8), ('k_scan_down', 8), ('fills_geometry', 1),
            ('k_tile_geom', 1), ('k_groups', 1), ('k_tile_rows', 1), ('k_group_final', 1), ('k_row_len', 1), ('k_publish', 3),
            ('fills_pulses', 1), ('k_tile_desc', 1), ('k_pulse_tiny', 1), ('k_pulse_wave', 1), ('fills_rows', 1), ('k_row_desc', 1),
            ('k_truth_reduce', 1), ('k_zle', 1), ('k_rec_keys', 2), ('record_sort', 1), ('k_invert_perm', 2), ('k_pack_desc', 2),
            ('k_pack', 1), ('k_lone_scan', 1), ('k_lone_rows', 1), ('fills_lone', 1), ('k_lone_desc', 1), ('k_row_empty', 1),
            ('k_pack_res', 1), ('k_ov_check', 1), ('k_ov_keys', 1), ('k_ov_valid', 1), ('k_ov_pulses', 1), ('k_ov_ends', 1),
            ('k_ov_heads', 1), ('k_ov_merged', 1), ('k_ov_count', 1), ('k_ov_out_keys', 1), ('k_ov_fill', 1)],
}


def _launches(eng):
    return [(name, n) for name, (_, n) in eng.kernel_times().items()]


def _engine():
    eng = make_engine(_base(enable_noise=False))
    eng.set_record_order(True)
    eng.set_profiling(True)
    return eng


def _sets(eng):
    windows, _ = _seam_windows(_lone_of(eng), eng.params)
    return _photon_sets(windows, np.asarray(_base()['gains'], dtype=np.float64))[0]


def _background(p, rec):
    """a handful of recorded pulses: one that ends inside the run's first pulse, one inside a simulated pulse, one on the sum channel
    and one far from every window"""
    rng = np.random.default_rng(9)
    mk = lambda ch, s, n: (int(ch), int(s), (p['baseline'] - 700 + rng.integers(-20, 21, size=n)).astype(np.int16))      # noqa: E731
    first = rec[np.argmin(rec['time'])]
    mid = rec[(rec['record_i'] == 0) & (rec['length'] > 40)][-1]
    return [mk(first['channel'], first['time'] // p['dt'] - 100, 130), mk(mid['channel'], mid['time'] // p['dt'] + 5, 20),
            mk(p['sum_channel'], first['time'] // p['dt'] - 50, 400), mk(3, first['time'] // p['dt'] - 9000, 5)]


def _first_order():
    """run, lone pass, overlay of the run's records where the device holds them: records and launches of each"""
    eng = _engine()
    sets = _sets(eng)
    eng.load_photons(*sets)
    eng.run()
    run, k_run = eng.records(), _launches(eng)
    lone, k_lone = eng.lone_hits(*PASS), _launches(eng)
    B = _background(eng.params, run)
    ov, k_ov = eng.overlay_records(OV.fragments(B, eng.params['dt'])), _launches(eng)
    p = dict(eng.params)
    eng.close()
    return dict(sets=sets, B=B, params=p, run=run, lone=lone, overlay=ov, kernel_times=dict(run=k_run, lone=k_lone, overlay=k_ov))


@pytest.fixture(scope='module')
def first():
    return _first_order()


@pytest.mark.gpu
def test_launches_are_the_parents(first):
    """the (name, launches) pairs of the three situations against the lists recorded on the parent commit: the run's sort is timed as
    record_sort, the lone pass's is not, no rocPRIM call of the overlay is"""
    for what in ('run', 'lone', 'overlay'):
        print(what, first['kernel_times'][what])
        assert first['kernel_times'][what] == KERNEL_TIMES[what], what
    run, lone, ov = (dict(first['kernel_times'][what]) for what in ('run', 'lone', 'overlay'))
    assert all(k in run for k in ('record_sort', 'k_rec_keys', 'k_invert_perm', 'k_pack_desc')) and 'k_pack_res' not in run
    assert lone['record_sort'] == run['record_sort'] == ov['record_sort'] == 1 and lone['k_invert_perm'] == 2 and lone['k_pack_res'] == 1 and 'k_ov_fill' in ov


def test_the_literals_are_the_recorded_lists():
    """profiles/record_backend_parent.json: what the parent commit launched, as recorded there"""
    with open(os.path.join(ROOT, 'profiles', 'record_backend_parent.json')) as f:
        rec = json.load(f)['kernel_times']
    assert {k: [tuple(x) for x in v] for k, v in rec.items()} == KERNEL_TIMES and all(len(v) > 5 for v in KERNEL_TIMES.values())


@pytest.mark.gpu
def test_records_of_the_first_order(first):
    """the run in (time, channel) order; the overlay of its records the restatement's, byte for byte"""
    p, run = first['params'], first['run']
    assert len(run) > 1 and np.array_equal(np.lexsort((run['channel'], run['time'])), np.arange(len(run)))
    assert len(first['lone']) > 1
    base = OV.base_array(p['n_rows'], p['baseline'], {})
    want = OV.merge_intervals(OV.pulses_of(run, p['dt']), first['B'], p['baseline'], base, p['dt'])
    assert len(first['overlay']) == len(want) >= len(run) and first['overlay'].tobytes() == want.tobytes()


@pytest.mark.gpu
def test_scratch_grows_inside_each_kind_of_pass(first):
    """a fresh handle takes the passes in the other order -- the overlay (of the first order's records, from the host), a run, a lone
    pass -- so that the one scratch buffer is first made by the overlay's calls and grows under the others: the same bytes"""
    eng = _engine()
    dt = first['params']['dt']
    ov = eng.overlay_records(OV.fragments(first['B'], dt), sim=first['run'])
    assert ov.tobytes() == first['overlay'].tobytes()
    eng.load_photons(*first['sets'])
    eng.run()
    assert eng.records().tobytes() == first['run'].tobytes()
    assert eng.lone_hits(*PASS).tobytes() == first['lone'].tobytes()
    # ... and once more against the run, now that every buffer has its size
    assert eng.overlay_records(OV.fragments(first['B'], dt)).tobytes() == first['overlay'].tobytes()
    eng.close()
    # a lone pass first: its two sorts make the buffer
    eng = _engine()
    eng.lone_hits(PASS[0], PASS[0] + 2000, PASS[0] + 2500)
    eng.load_photons(*first['sets'])
    eng.run()
    assert eng.records().tobytes() == first['run'].tobytes() and eng.lone_hits(*PASS).tobytes() == first['lone'].tobytes()
    eng.close()


# ---------------------------------------------------------------------------------------------------- 0, 1 and 2 records of a pass
# Passes on channel 5 alone (the configuration of tests/test_lone_hits_cpu.py) against no rows, s0 at the first photon of a chain:
# (s0, s1 - s0) -> rows, records of the host model.  A pass of one record or none takes no sort, one of two the sort of two keys.
FEW = {'row_without_a_record': (91263, 1, 1, 0), 'one_record': (89879, 1, 1, 1), 'two_records': (89879, 306, 2, 2), 'no_seed_owned': (89951, 100, 0, 0)}


def _few_config():
    cfg = with_fma(xenonnt_test_config(seed=SEED, enable_noise=False), False)
    rates = np.zeros(6)
    rates[5] = NEAR_LIMIT * DC.max_rate(kernel_params(cfg)['dt'])
    return cfg, rates


def _few_model(lone, p, thr, s0, width):
    rows = lone.rows(5, s0, s0 + width, s0 + width + 500)
    data = [LH.finish(lone.term(r), p['baseline']) for r in rows]
    return rows, LH.records_of_rows(rows, data, lambda ch: int(thr[ch]), p['trigger_window'], p['dt'])


@pytest.mark.parametrize('name', sorted(FEW))
def test_the_model_yields_the_few_records(name):
    """on the CPU: the chosen passes hold exactly the rows and records they were chosen for"""
    cfg, rates = _few_config()
    p = kernel_params(cfg)
    lone = LH.Lone(DK.Dark.of_config(cfg, DC.thresholds(rates, 494, p['dt'])), p['trigger_window'])
    s0, width, n_rows, n_rec = FEW[name]
    rows, rec = _few_model(lone, p, host_tables(cfg)['thr_zle'], s0, width)
    assert (len(rows), len(rec)) == (n_rows, n_rec)


@pytest.mark.gpu
def test_passes_of_zero_one_and_two_records():
    cfg, rates = _few_config()
    eng = make_engine(dict(cfg, dark_count_rate=rates))
    eng.set_profiling(True)
    lone = LH.Lone(DK.Dark.of_engine(eng), eng.params['trigger_window'])
    for name, (s0, width, n_rows, n_rec) in sorted(FEW.items()):
        rows, want = _few_model(lone, eng.params, eng.tables['thr_zle'], s0, width)
        got = eng.lone_hits(s0, s0 + width, s0 + width + 500)
        assert len(eng.lone_hit_rows()) == len(rows) == n_rows and len(got) == len(want) == n_rec, name
        assert got.tobytes() == want.tobytes(), name
    eng.close()
