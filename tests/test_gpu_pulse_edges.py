"""Every pulse kernel of the HIP path on reference runs of designed edge photon lists (MI355X only).

tests/golden/pulse_edges.npz and pulse_edges_geometry.npz (tests/pulse_edges.py: the case table; tests/test_pulse_edges_reference.py: the
same fixtures on the oracle, their intended shapes and the no-near-tie condition).  A case group is one digitise window and one replay
unit: the dense and sparse kernels are chosen from batch maxima, so a group built for one k_pulse_dense instantiation runs alone.
Per group and arithmetic form:
  * accumulator path, debug on, as dispatched and with force_dense: bounds, photons, currents (exact form: bit-exact, 4 ulp of the tile
    maximum for >= 3 photons in one ns; fused form: within the derived bound of the exact rational value), windows, rows, ZLE, records,
    truth -- against the REFERENCE; the kernel the group was built for is the one that ran (kernel_times)
  * resident rows (k_row_pulse), 1024- and 256-sample segments: intervals and truth against the reference, records equal to the
    accumulator run's bytes
add_current.npz (direct calls of the reference's add_current) goes through the device, and the pulse half of k_s2_tile answers to the
oracle on the photons the device reports.  The log names the tile kernels of every group (pytest -s).

Many photons in one ns (the saturated tiles: 2049 photons in one bin, 226 of them in one ns with 10 ns samples, 416 with 5 ns).  The
reference sums their gains in the order of numpy's unstable argsort; the 4 ulp of the tile maximum this suite keeps for tiles with >= 3
photons in one ns were derived for a few photons per ns.  On the CPU, for the 416-photon tile: the reference's own currents are 2 ulp
from the exact rational ones, a sequential sum in a random order is more than 4 ulp from the reference in 2.5 % of 200 orders (largest
6), a correctly rounded merge 1 ulp.  k_pulse_generic used to merge a cell's gains with plain atomic adds, in an order that changes from
run to run: five runs of that tile measured 2, 3, 4, 4 and 5 ulp.  It now splits every gain at a power of two so that the merged gain does
not depend on the order (wfs_kernels.h) and is the correctly rounded sum.  k_pulse_dense still merges with atomic adds: its 226-photon
tile measured at most 2 ulp on the device, and 0 of 200 random orders exceed 4 ulp on the CPU (largest 2).
"""
import numpy as np
import pytest

from tests import pulse_edges as PE
from tests.helpers import (golden, make_engine, make_oracle, replay_chain_on_engine, canonical_intervals, with_fma, assert_currents_close,
                           pulse_edges_config, PULSE_EDGES)
from tests.test_gpu_parity import _check_chain_mode, _nonempty_groups
from tests.test_pulse_edges_reference import fixture, check_currents, TRUTH_INT, TRUTH_F64
from wfsim_amd.config import xenonnt_test_config

pytestmark = pytest.mark.gpu

GROUPS = [(name, str(g)) for name in PULSE_EDGES for g in golden(name)['group_names']]
_engines = {}


def _engine(name, fma, mode, monkeypatch=None):
    """one engine per fixture, arithmetic form and digitisation path ('acc': accumulator rows; 'res' / 'res256': resident rows with the
    default / the 256-sample segment, which the library reads from WFS_RES_MAX_LEN when the engine is made), profiling on"""
    key = (name, fma, mode)
    if key not in _engines:
        cfg = with_fma(dict(pulse_edges_config(name), row_resident=mode != 'acc'), fma)
        if mode == 'res256':
            monkeypatch.setenv('WFS_RES_MAX_LEN', '256')
        eng = make_engine(cfg)
        eng.set_profiling(True)
        _engines[key] = (eng, cfg)
    return _engines[key]


def _tile_kernels(eng):
    return sorted(k for k in eng.kernel_times() if k in PE.TILE_KERNELS)


def _check_truth(eng, sub):
    acc, ts = eng.truth()
    for j, f in enumerate(TRUTH_INT):
        assert np.array_equal(acc[:, j], sub['call_truth_' + f]), f
        assert np.array_equal(acc[:, 6 + j], sub['call_truth_' + f + '_bottom']), f + '_bottom'
    for j, f in enumerate(TRUTH_F64):
        assert np.allclose(acc[:, 4 + j], sub['call_truth_' + f], rtol=1e-12, atol=0), f
        assert np.allclose(acc[:, 10 + j], sub['call_truth_' + f + '_bottom'], rtol=1e-12, atol=0), f + '_bottom'


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
@pytest.mark.parametrize('name,group', GROUPS, ids=[f'{n[:-4]}-{g}' for n, g in GROUPS])
def test_group_on_its_kernels(name, group, fma, monkeypatch):
    d, cfg0, dt, exact, shapes = fixture(name)
    main = name == 'pulse_edges.npz'
    sub = PE.subset(d, PE.group_calls(d, group))
    sh = [shapes[j] for j in sub['pl_index']]
    classes = sorted({PE.tile_class(s[0], s[1]) for s in sh})
    worst = {}

    def currents(tag):
        def f(p, order):
            worst[tag] = check_currents(p['current'], p['cur_off'][order], d, exact, shapes, fma, pulses=sub['pl_index'], what=f'{group} ({tag})')
        return f

    # ---- accumulator path, debug on: as dispatched, then every tile through the dense kernel
    eng, cfg = _engine(name, fma, 'acc')
    _check_chain_mode(None, cfg, force_dense=False, d=sub, eng=eng, currents=currents('dispatched'))
    _check_truth(eng, sub)
    ran = _tile_kernels(eng)
    records = eng.records().tobytes()
    if main:
        assert ran == sorted(PE.KERNEL_OF_CLASS[c] for c in classes), (group, ran, classes)
        if group.startswith('class_'):
            assert classes == [group[6:]]
        if group.startswith('dense_'):
            # the batch maxima, from what the device reports, meet the dispatch condition the group was built for
            p = eng.pulses()
            nb = p['right'] - p['left'] + 1 - (int(cfg['samples_to_store_before']) + int(cfg['samples_to_store_after']) + 22)
            tpb, resident, n_win = PE.dense_variant(int(nb.max()), int(p['n_photons'].max()))
            want = dict(dense_128_res=(128, True), dense_256_res=(256, True), dense_128_win=(128, False), dense_256_win=(256, False), dense_256_win_one_chunk=(256, False))[group]
            assert classes == ['dense'] and (tpb, resident) == want, (group, int(nb.max()), int(p['n_photons'].max()))
            assert n_win == dict(dense_256_win=PE.NWIN_MAX).get(group, 1)          # (the windowed form with ONE window per tile too)
    else:
        assert ran == ['k_pulse_generic'], ran
    _check_chain_mode(None, cfg, force_dense=True, d=sub, eng=eng, currents=currents('force_dense'))
    _check_truth(eng, sub)
    forced = _tile_kernels(eng)
    assert forced == (['k_pulse_dense'] if main else ['k_pulse_generic']), forced
    assert eng.records().tobytes() == records
    # ---- resident rows
    qualifies = [s[0] <= PE.WAVE_MAX_PHOTONS and s[1] <= PE.WAVE_MAX_BINS for s in sh]
    by_channel = {}
    for j, q in zip(sub['pl_index'], qualifies):
        by_channel[int(d['pl_ch'][j])] = by_channel.get(int(d['pl_ch'][j]), True) and q
    ref_itv = canonical_intervals(sub['zle_digit'], sub['zle_ch'], sub['zle_left'], sub['zle_right'], sub['zle_data_off'], sub['zle_data'])
    res_ran = {}
    for mode in ('res', 'res256'):
        eng_r, cfg_r = _engine(name, fma, mode, monkeypatch)
        replay_chain_on_engine(eng_r, sub, cfg_r, debug=False)
        kt = eng_r.kernel_times()
        res_ran[mode] = sorted(k for k in kt if k in PE.TILE_KERNELS or k == 'k_row_pulse')
        if main:
            assert ('k_row_pulse' in kt) == any(by_channel.values()), (group, mode, sorted(kt))
            if all(by_channel.values()):
                assert not (set(kt) & PE.TILE_KERNELS), (group, mode, sorted(kt))       # every row of the group is made by k_row_pulse
        else:
            assert 'k_row_pulse' not in kt          # (k_pulse_generic geometries keep the accumulator path)
        g, keep = _nonempty_groups(eng_r)
        gmap = {int(gi): j for j, gi in enumerate(keep)}
        z = eng_r.intervals()
        got = canonical_intervals([gmap[int(x)] for x in z['group']], z['channel'], z['left'], z['right'], z['data_off'], z['data'])
        assert got == ref_itv, (group, mode)
        assert eng_r.records().tobytes() == records, (group, mode)
        _check_truth(eng_r, sub)
    print(f'\n{name[:-4]} / {group} / {"fused" if fma else "exact"}: classes {classes} ran {ran}; force_dense {forced}; resident {res_ran["res"]}, 256-sample segments '
          f'{res_ran["res256"]}; currents vs reference (ulp of the tile maximum, fraction of the derived bound): dispatched {worst["dispatched"][0]:.2f}, '
          f'{worst["dispatched"][1]:.3f}; force_dense {worst["force_dense"][0]:.2f}, {worst["force_dense"][1]:.3f}')


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
def test_add_current_vectors_on_the_device(fma):
    """tests/golden/add_current.npz: six direct calls of the reference's Pulse.add_current, each as a one-channel pulse set through
    wfs_load_photons.  Exact form: the rule of test_add_current_bit_exact; fused form: within FMA_CURRENT_TOL_ULP of the reference (as
    test_add_current_fused asks of the oracle) and within the derived bound of the exact rational current; the rounded ADC values equal"""
    from fractions import Fraction
    g = golden('add_current.npz')
    tab = golden('tables.npz')
    c2a = float(tab['current_2_adc'])
    TF = [[Fraction(float(x)) for x in row] for row in tab['templates']]
    cfg = with_fma(xenonnt_test_config(), fma)
    eng = make_engine(cfg)
    eng.set_profiling(True)
    for i in range(int(g['n'])):
        t, gain, left, ref = g[f't{i}'], g[f'g{i}'], int(g[f'left{i}']), g[f'cur{i}']
        for force_dense in (False, True):
            eng.set_debug(True, force_dense)
            eng.load_photons(np.zeros(1, np.int32), np.array([t.min()], np.int64), np.array([0, len(t)], np.int64), t, np.full(len(t), 300, np.int16),
                             gain, np.zeros(len(t), np.uint8))
            eng.run()
            p = eng.pulses(currents=True)
            assert len(p['left']) == 1 and p['left'][0] == left and p['right'][0] - left + 1 == len(ref) and p['n_photons'][0] == len(t)
            cur = p['current'][p['cur_off'][0]:p['cur_off'][0] + len(ref)]
            _, counts = np.unique(t, return_counts=True)
            ulp = np.abs(cur - ref).max() / np.spacing(np.abs(ref).max())
            print(f'add_current case {i} ({"fused" if fma else "exact"}, force_dense {force_dense}): {_tile_kernels(eng)} {ulp:.2f} ulp of the tile maximum')
            if fma:
                assert_currents_close(cur, ref, f'case {i}')
            elif counts.max() <= 2 or i == 1:
                assert np.array_equal(cur, ref), f'case {i}: max diff {np.abs(cur - ref).max()}'
            else:
                assert ulp <= 4, f'case {i}'
            ex, mag, n = PE.exact_tile(t, gain, left, len(ref), 10, TF)
            C = Fraction(c2a)
            e = dict(cur=ex, n=n, B=[PE.gamma(n[s] + 1) * mag[s] * C if n[s] else Fraction(0) for s in range(len(ref))])
            assert PE.currents_within_bound(cur, e, c2a) <= 1.0, f'case {i}'
            assert np.array_equal(np.around(cur * c2a), np.around(ref * c2a))


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
def test_s2_tile_pulses_against_the_oracle_on_reported_photons(fma):
    """k_s2_tile cannot take injected photons.  A batch of tile-generated S2s whose tiles hold 1 to about 2000 photons keeps its photons
    (debug bit 4 only: k_s2_tile makes the pulses); the photons the device reports go to the oracle's pulse_call with preassigned
    gains, whose arithmetic the designed fixtures pin on the reference -- the records must be the same bytes, whatever the generators
    agree on"""
    from tests.test_gpu_generation import _instructions, MS
    from wfsim_amd.physics import instruction_params
    from wfsim_amd.resource import Resource
    from wfsim_amd.scheduler import schedule
    cfg = with_fma(dict(xenonnt_test_config(s2_secondary_sc_gain=100.0), tile_local_min_photons=0, seed=91), fma)
    amps = [1, 4, 40, 150, 700, 2000, 5000, 9000, 11000]
    ins = _instructions([dict(type=2, time=2 * MS * (i + 1), x=1.0 * i, y=-2.0, z=-5.0 - 2 * i, amp=a) for i, a in enumerate(amps)])
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    eng = make_engine(cfg)
    eng.set_profiling(True)
    eng.set_debug(False)                 # (make_engine keeps the photons: bit 4 alone)
    eng.load_instructions(s_ins, gid, cluster, key, instruction_params(s_ins, cfg, res))
    counts = eng.run()
    kt = eng.kernel_times()
    assert 'k_s2_tile' in kt and 'k_pulse_dense' not in kt, sorted(kt)
    ph = eng.photons()
    assert counts['n_pulse_sets'] == len(amps)
    sizes = np.concatenate([np.bincount(ph['ch'][a:b], minlength=494) for a, b in zip(ph['set_off'][:-1], ph['set_off'][1:])])
    sizes = sizes[sizes > 0]
    print(f'k_s2_tile tiles: {len(sizes)}, photons per tile {sizes.min()} .. {sizes.max()}; kernels {sorted(kt)}')
    assert sizes.min() == 1 and 1024 < sizes.max() <= 2048 and np.any((sizes > 64) & (sizes <= 256)) and np.any((sizes > 4) & (sizes <= 32))
    g = eng.groups()
    assert (g['right'] >= g['left']).sum() == len(amps)          # every S2 in a window of its own
    orc = make_oracle(cfg)
    for i in range(len(amps)):
        a, b = ph['set_off'][i], ph['set_off'][i + 1]
        assert np.all(np.diff(ph['ch'][a:b]) >= 0)
        orc.pulse_call(2, i, ph['t'][a:b], ph['ch'][a:b], ph['dpe'][a:b], ph['gain'][a:b], True)
        orc.digitize_and_zle(0)
    assert counts['n_records'] > 1000
    assert eng.records().tobytes() == orc.pack_records().tobytes()
