"""The CPU oracle on reference runs of DESIGNED photon lists (tests/golden/pulse_edges.npz, pulse_edges_geometry.npz; case table and exact
arithmetic in tests/pulse_edges.py; made by tests/golden/make_golden.py pulse_edges).  CPU only.

Every case sits on a boundary of the HIP pulse kernels (tile classes, k_pulse_dense instantiations, the tap_block threshold, chunk and
segment seams), carries explicit gains and was checked, in exact rational arithmetic, to hold no sample near a rounding tie -- so both
arithmetic forms of add_current must give the reference's rows, with no sample left out of the comparison.

Currents in the fused form: within B / c2a of the EXACT value per sample, B = gamma(n + 1) sum |term| c2a (derived; tests/pulse_edges.py).
Measured on these fixtures (oracle, on the commit that adds them): fused currents at most 2 ulp of the tile maximum away from the
reference's (main) and 3 ulp (geometry), 0.50 of the derived bound -- inside FMA_CURRENT_TOL_ULP, which stays the tolerance of the golden
chains and is not asserted here.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import pulse_edges as PE
from tests.helpers import (golden, make_oracle, replay_chain_on_oracle, with_fma, pulse_edges_config, PULSE_EDGES, FMA_CURRENT_TOL_ULP)

TRUTH_INT = ['n_photon', 'n_pe', 'n_photon_trigger', 'n_pe_trigger']
TRUTH_F64 = ['raw_area', 'raw_area_trigger']
_cache = {}


def fixture(name):
    """(arrays, config, dt, exact currents / bounds per pulse, shapes per pulse)"""
    if name not in _cache:
        d = golden(name)
        cfg = pulse_edges_config(name)
        dt = int(cfg.get('sample_duration', 10))
        _cache[name] = (d, cfg, dt, PE.fixture_exact(d, d['templates'], float(d['current_2_adc']), dt), PE.tile_shapes(d, dt))
    return _cache[name]


def designed_ties(d):
    return set(zip(d['tie_pulse'].tolist(), d['tie_sample'].tolist()))


def check_currents(cur, cur_off, d, exact, shapes, fma, pulses=None, what=''):
    """currents of pulses (fixture numbering `pulses`, default all) against the reference's and the exact ones.  Exact form: bit-exact,
    4 ulp of the tile maximum for tiles with >= 3 photons in one ns (the reference merges their gains in the order of numpy's unstable
    argsort, see test_add_current_bit_exact).  Both forms: within the derived bound of the exact value.  Returns the largest difference
    from the reference's currents in ulp of the tile maximum and the largest |error| / bound."""
    c2a = float(d['current_2_adc'])
    worst_ulp, worst_bound = 0.0, 0.0
    for i, j in enumerate(range(len(d['pl_ch'])) if pulses is None else pulses):
        ref = d['pl_current'][d['pl_cur_off'][j]:d['pl_cur_off'][j + 1]]
        c = cur[cur_off[i]:cur_off[i] + len(ref)]
        ulp = np.abs(c - ref).max() / np.spacing(np.abs(ref).max())
        if not fma:
            if shapes[j][3] >= 3:
                assert ulp <= 4, f'{what} pulse {j}: {ulp} ulp of the tile maximum'
            else:
                assert np.array_equal(c, ref), f'{what} pulse {j}: max diff {np.abs(c - ref).max()}'
        b = PE.currents_within_bound(c, exact[j], c2a)
        assert b <= 1.0, f'{what} pulse {j}: current error {b} x the derived bound'
        worst_ulp, worst_bound = max(worst_ulp, ulp), max(worst_bound, b)
    return worst_ulp, worst_bound


def case_of_pulse(d):
    calls = np.repeat(np.arange(len(d['call_pulse_off']) - 1), np.diff(d['call_pulse_off']))
    return [str(d['case_names'][d['call_case'][k]]) for k in calls]


def assert_rows_and_zle(r, d, what):
    names = case_of_pulse(d)
    assert np.array_equal(r['row_ch'], d['row_ch']) and np.array_equal(r['row_left'], d['row_left']) and np.array_equal(r['row_right'], d['row_right'])
    if not np.array_equal(r['row_data'], d['row_data']):
        bad = np.flatnonzero(r['row_data'] != d['row_data'])
        row = np.searchsorted(d['row_data_off'], bad[0], side='right') - 1
        dig = np.searchsorted(d['dg_row_off'], row, side='right') - 1
        raise AssertionError(f'{what}: {len(bad)} row samples differ, first in window {dig} ({d["group_names"][dig]}) channel {d["row_ch"][row]}; '
                             f'cases of the window: {sorted(set(n for n, g in zip(names, np.repeat(d["call_group"], np.diff(d["call_pulse_off"]))) if g == dig))}')
    for k in ['digit', 'ch', 'left', 'right', 'data_off', 'data']:
        assert np.array_equal(r['zl_' + k], d['zle_' + k]), (what, k)


@pytest.mark.parametrize('name', PULSE_EDGES)
def test_replay_exact_form(name):
    """bit-exact against the reference: pulse bounds, photon counts, currents, window edges, rows, ZLE tuples, integer truth columns;
    the area sums at rtol 1e-12"""
    d, cfg, dt, exact, shapes = fixture(name)
    orc = make_oracle(with_fma(cfg, False))
    r = replay_chain_on_oracle(orc, d)
    for a, b in [('pl_ch', 'pl_ch'), ('pl_left', 'pl_left'), ('pl_right', 'pl_right'), ('pl_nph', 'pl_photons'), ('dg_left', 'dg_left'), ('dg_right', 'dg_right')]:
        assert np.array_equal(r[a], d[b]), a
    check_currents(r['cur'], r['pl_cur_off'], d, exact, shapes, fma=False, what=name)
    assert_rows_and_zle(r, d, name)
    tr = r['truth'].reshape(-1, 12)
    for j, f in enumerate(TRUTH_INT):
        assert np.array_equal(tr[:, j], d['call_truth_' + f].astype(np.float64)), f
        assert np.array_equal(tr[:, 6 + j], d['call_truth_' + f + '_bottom'].astype(np.float64)), f + '_bottom'
    for j, f in enumerate(TRUTH_F64):
        assert np.allclose(tr[:, 4 + j], d['call_truth_' + f], rtol=1e-12, atol=0), f
        assert np.allclose(tr[:, 10 + j], d['call_truth_' + f + '_bottom'], rtol=1e-12, atol=0), f + '_bottom'


@pytest.mark.parametrize('name', PULSE_EDGES)
def test_replay_fused_form(name):
    """rows and ZLE equal to the reference's; currents within the derived bound of the exact rational value -- and so are the
    reference's own currents, which checks the bound; the two forms do differ"""
    d, cfg, dt, exact, shapes = fixture(name)
    ref_ulp, ref_bound = check_currents(d['pl_current'], d['pl_cur_off'], d, exact, shapes, fma=True, what=name + ' (reference)')
    assert ref_ulp == 0
    orc = make_oracle(with_fma(cfg, True))
    r = replay_chain_on_oracle(orc, d)
    assert np.array_equal(r['pl_left'], d['pl_left']) and np.array_equal(r['pl_right'], d['pl_right']) and np.array_equal(r['pl_nph'], d['pl_photons'])
    ulp, bound = check_currents(r['cur'], r['pl_cur_off'], d, exact, shapes, fma=True, what=name + ' (fused)')
    print(f'{name}: fused currents at most {ulp:.2f} ulp of the tile maximum from the reference ({FMA_CURRENT_TOL_ULP} stated for the golden chains), '
          f'{bound:.3f} of the derived bound; the reference itself {ref_bound:.3f} of the bound')
    assert ulp > 0
    assert_rows_and_zle(r, d, name + ' (fused)')


@pytest.mark.parametrize('name', PULSE_EDGES)
def test_no_sample_near_a_rounding_tie(name):
    """recomputed from the committed data: apart from the two designed ties, every sample's exact current x c2a is farther than 4 B from
    a half-integer -- so any summation order, fused or not, rounds like the reference"""
    d, cfg, dt, exact, shapes = fixture(name)
    bad, ratio, dist = PE.near_ties(exact, designed_ties(d))
    assert not bad, [(case_of_pulse(d)[j], s) for j, s in bad]
    assert float(dist) == float(d['min_tie_distance']) and ratio > 4
    for j, s in designed_ties(d):
        assert exact[j]['dist'][s] < Fraction(1, 10 ** 9)          # the exact product is within ~1e-15 of the tie the doubles hit


@pytest.mark.parametrize('name', PULSE_EDGES)
def test_designed_ties_round_half_to_even(name):
    d, cfg, dt, exact, shapes = fixture(name)
    c2a = np.float64(d['current_2_adc'])
    base = int(cfg['digitizer_reference_baseline'])
    dig_of_row = np.repeat(np.arange(len(d['dg_left'])), np.diff(d['dg_row_off']))
    call_of_pulse = np.repeat(np.arange(len(d['call_pulse_off']) - 1), np.diff(d['call_pulse_off']))
    assert sorted(k % 2 for k in d['tie_k']) == [0, 1]
    for j, s, k in zip(d['tie_pulse'], d['tie_sample'], d['tie_k']):
        cur = d['pl_current'][d['pl_cur_off'][j]:d['pl_cur_off'][j + 1]]
        assert cur[s] * c2a == k + 0.5
        g = int(d['call_group'][call_of_pulse[j]])
        row = int(np.flatnonzero((dig_of_row == g) & (d['row_ch'] == d['pl_ch'][j]))[0])
        data = d['row_data'][d['row_data_off'][row]:d['row_data_off'][row + 1]]
        at = int(d['pl_left'][j]) + int(s) - (int(d['dg_left'][g]) + int(d['row_left'][row]))
        assert base - data[at] == (k if k % 2 == 0 else k + 1), (k, base - data[at])


def _builder(name, d):
    c2a = float(d['current_2_adc'])
    ties = PE.find_ties(d['templates'], c2a)
    thr = PE.truth_threshold_gain(d['templates'].max(axis=1), c2a, 15)
    return (PE.main_cases if name == 'pulse_edges.npz' else PE.geometry_cases)(thr, ties), thr


@pytest.mark.parametrize('name', PULSE_EDGES)
def test_cases_have_their_intended_shapes(name):
    """computed from the fixture: every named case has the (photons, start bins), class, occupied cells, batch maxima, row length and
    seam offsets it was designed for"""
    d, cfg, dt, exact, shapes = fixture(name)
    main = name == 'pulse_edges.npz'
    b, thr = _builder(name, d)
    assert [c['name'] for c in b.cases] == [str(x) for x in d['case_names']] and list(b.groups) == [str(x) for x in d['group_names']]
    assert len(set(d['case_names'].tolist())) == len(d['case_names'])
    assert np.all(np.diff(d['dg_left']) * dt >= 1_000_000) and len(d['dg_left']) == len(b.groups)        # one window per group, >= 1 ms apart
    c2a, base, tw = float(d['current_2_adc']), int(cfg['digitizer_reference_baseline']), int(cfg['trigger_window'])
    dig_of_row = np.repeat(np.arange(len(d['dg_left'])), np.diff(d['dg_row_off']))
    seen = set()
    for k, case in enumerate(b.cases):
        e = case['expect']
        a, z = int(d['call_ph_off'][k]), int(d['call_ph_off'][k + 1])
        assert np.array_equal(d['ph_t'][a:z], np.concatenate([t for t, _, _ in case['tiles']])), case['name']      # the designed times
        assert d['set_tmin'][k] == case['set_tmin'] and d['set_cluster'][k] == case['group'] == d['call_group'][k]
        pulses = range(int(d['call_pulse_off'][k]), int(d['call_pulse_off'][k + 1]))
        assert len(pulses) == len(case['tiles'])
        sh = [shapes[j] for j in pulses]
        gains = d['ph_gain'][a:z]
        g = case['group']
        in_group = [j for j in range(len(shapes)) if d['call_group'][np.searchsorted(d['call_pulse_off'], j, side='right') - 1] == g]
        if 'shape' in e:
            assert sh[0][:2] == tuple(e['shape']), (case['name'], sh[0])
        if 'cls' in e and main:
            assert all(PE.tile_class(s[0], s[1]) == e['cls'] for s in sh), (case['name'], sh)
            assert all(PE.tile_class(shapes[j][0], shapes[j][1]) == e['cls'] for j in in_group), case['name']      # a single-class group
        if 'max_per_ns' in e:
            assert sh[0][3] == e['max_per_ns']
        if 'cells' in e:
            assert sh[0][2] == e['cells'] and sh[0][1] + 21 <= 64          # one wave sees every cell of the tile
        if 'variant' in e:
            mx_nb, mx_ph = max(shapes[j][1] for j in in_group), max(shapes[j][0] for j in in_group)
            assert all(PE.tile_class(shapes[j][0], shapes[j][1]) == 'dense' for j in in_group)
            assert PE.dense_variant(mx_nb, mx_ph)[:2] == tuple(e['variant']), (case['name'], mx_nb, mx_ph)
        rows = [int(np.flatnonzero((dig_of_row == g) & (d['row_ch'] == d['pl_ch'][j]))[0]) for j in pulses]
        if 'row_length' in e:
            assert d['row_right'][rows[0]] - d['row_left'][rows[0]] + 1 == e['row_length']
        if 'seam' in e:
            side, off = e['seam']
            row_left = int(d['dg_left'][g]) + int(d['row_left'][rows[0]])
            j = pulses[0]
            assert (int(d['pl_left'][j]) if side == 'left' else int(d['pl_right'][j])) - row_left == off, case['name']
            if case['name'] == 'f_seam_last':
                assert d['row_right'][rows[0]] - d['row_left'][rows[0]] + 1 == 3000
            for name_, seam in (('straddles_1280', 1280), ('straddles_2048', 2048)):
                if case['name'].endswith(name_):
                    assert int(d['pl_left'][j]) - row_left < seam - 1 and int(d['pl_right'][j]) - row_left > seam
        if e.get('shared_row'):
            assert sum(1 for j in in_group if d['pl_ch'][j] == d['pl_ch'][pulses[0]]) >= 4
        if 'tie' in e:
            assert sh[0][:2] == (1, 1) and e['tie'] in d['tie_k']
        if e.get('saturates'):
            data = d['row_data'][d['row_data_off'][rows[0]]:d['row_data_off'][rows[0] + 1]]
            assert data.min() == 0 and sh[0][:2] == (2049, 1)          # the clamp value (rawdata.py:272)
        if 'below_baseline' in e:
            j = pulses[0]
            adc = np.around(d['pl_current'][d['pl_cur_off'][j]:d['pl_cur_off'][j + 1]] * c2a).max()
            assert e['below_baseline'][0] <= adc - base <= e['below_baseline'][1] and adc < 2 ** 31 and sh[0][0] <= 64      # fits i32, not i16
            data = d['row_data'][d['row_data_off'][rows[0]]:d['row_data_off'][rows[0] + 1]]
            assert data.min() == 0
        if e.get('truth_sides'):
            over = gains > thr[d['ph_t'][a:z] % dt]
            assert 0 < over.sum() < len(over) and d['call_truth_n_photon_trigger'][k] == over.sum() and d['call_truth_n_photon'][k] == len(over)
        if 'before_tmin' in e:
            assert d['set_tmin'][k] - d['ph_t'][a:z].min() == e['before_tmin']
        if 'tmin_mod' in e:
            assert d['set_tmin'][k] % dt == e['tmin_mod'] == d['ph_t'][a:z].min() % dt
        if e.get('epoch'):
            assert d['ph_t'][a:z].min() == PE.EPOCH
        if e.get('negative'):
            assert d['ph_t'][a:z].min() < 0 and d['pl_left'][pulses[0]] < 0
        if case['name'] == 'e_negative_gain':
            assert gains[0] < 0 and d['row_data'][d['row_data_off'][rows[0]]:d['row_data_off'][rows[0] + 1]].max() > base
        if case['name'] == 'e_gain_range':
            assert gains.min() < 2e3 and gains.max() >= 1e9
        seen.add(case['name'])
    if main:
        # every class boundary of wfs_kernels.h:149-157, both sides
        T, S, W = (PE.TINY_MAX_PHOTONS, PE.TINY_MAX_BINS), (PE.SPARSE_MAX_PHOTONS, PE.SPARSE_MAX_BINS), (PE.WAVE_MAX_PHOTONS, PE.WAVE_MAX_BINS)
        want = {T: 'tiny', (T[0] + 1, T[1]): 'sparse', (T[0], T[1] + 1): 'sparse', S: 'sparse', (S[0] + 1, S[1]): 'wave', (S[0], S[1] + 1): 'wave',
                W: 'wave', (W[0] + 1, 2): 'dense', (W[0], W[1] + 1): 'dense', (1, 1): 'tiny'}
        have = {s[:2] for s in shapes}
        for shape, cls in want.items():
            assert shape in have and PE.tile_class(*shape) == cls and f'a_{shape[0]}x{shape[1]}_{cls}' in seen, shape
        variants = {tuple(c['expect']['variant']) for c in b.cases if 'variant' in c['expect']}
        assert variants == {(128, True), (256, True), (128, False), (256, False)}
        nbs = {s[1] for s in shapes}
        assert {235, 236, 237} <= nbs and PE.dense_variant(2100, 2049)[2] == PE.NWIN_MAX and -(-(2100 + 21) // 256) > PE.NWIN_MAX
        assert {s[2] for s, n in zip(shapes, case_of_pulse(d)) if n.startswith('c_tap_4')} == {PE.TAP_SPARSE_MAX - 1, PE.TAP_SPARSE_MAX, PE.TAP_SPARSE_MAX + 1}
    else:
        assert {235, 236, 237} <= {s[1] for s in shapes} and max(s[0] for s in shapes) == 2049


def test_subset_of_a_fixture_replays_like_the_whole():
    """the restriction to one case group (the replay unit of the GPU tests) carries the group's reference outputs"""
    d, cfg, dt, exact, shapes = fixture('pulse_edges.npz')
    total = 0
    for gname in d['group_names']:
        sub = PE.subset(d, PE.group_calls(d, str(gname)))
        orc = make_oracle(with_fma(cfg, True))
        r = replay_chain_on_oracle(orc, sub)
        assert len(sub['dg_left']) == 1 and np.array_equal(r['dg_left'], sub['dg_left'])
        assert np.array_equal(r['row_data'], sub['row_data']) and np.array_equal(r['zl_data'], sub['zle_data']), gname
        assert np.array_equal(r['zl_left'], sub['zle_left'])
        total += len(sub['row_data'])
    assert total == len(d['row_data'])
