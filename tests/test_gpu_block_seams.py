"""The block photon generator at the seams of its front end (MI355X only): the designed cases of tests/block_seams.py -- the 2048-photon
block grid, the 512-emitter window, blocks that begin inside a Philox quad, wide blocks at an instruction's first and last photon, head /
ranges / tail layouts, every order class for heads, tails, fullsort tiles and afterpulse tiles, (block, channel) segments, run sets, the
emitter front end (tests/test_block_seams_cpu.py shows which case stands on which seam) -- and secondary gains on both sides of the Poisson
table (POIS_LAM_MAX = 217: k_s2_photons, PTRS).

Device against the CPU oracle on the same Philox streams.  Every tile must be in the ORACLE'S ORDER photon by photon
(tests/helpers.py: assert_tiles_in_oracle_order); digitise windows, record bytes, n_pe, the 12 truth columns set by set, the photon
offsets of the instructions; no tile-local kernel where the block generator is meant.  Every launch is checked."""
import numpy as np
import pytest

from tests import block_seams as B
from tests import hot_patterns as H
from tests.helpers import make_engine
from tests.test_gpu_hot_patterns import _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')
    monkeypatch.delenv('WFS_BRIGHT_MAX_BINS', raising=False)


def _device(cfg, res, s, eng=None, profiling=False):
    eng = eng or make_engine(cfg, resource=res)
    if profiling:
        eng.set_profiling(True)
    eng.load_instructions(s['s_ins'], s['gid'], s['cluster'], s['key'], s['ip'], run_set=s['run_set'])
    return eng, eng.run()


def _run_both(case):
    """tests/test_gpu_generation.py::_run_both for a case of tests/block_seams.py: both sides receive the same batch (ip overrides applied)"""
    cfg, res, s, orc, o = B.oracle_case(case)
    eng, counts = _device(cfg, res, s)
    return cfg, s, orc, o, eng, counts


def _assert_case(case, cfg, s, orc, o, eng, counts):
    _compare(cfg, None, orc, o, eng, counts, s)          # tiles in the oracle's order, windows, record bytes, n_pe, truth rows by set identity
    t = B.block_table(o, s['s_ins'], cfg)
    assert np.array_equal(eng.instruction_photon_offsets(), t['ins_ph0'])
    if case['block']:
        assert not eng.tile_kernels().any()
    return t


CASES = B.cases()


@pytest.mark.parametrize('name', list(CASES))
def test_block_seam_case_matches_oracle(name):
    case = CASES[name]
    cfg, s, orc, o, eng, counts = _run_both(case)
    t = _assert_case(case, cfg, s, orc, o, eng, counts)
    print(f'{name}: {counts["n_photons"]} photons, {t["n_blocks"]} blocks ({int(t["fast"].sum())} fast), {int(t["fullsort"].sum())} fullsort instructions')
    if case['ap'] is not None:
        assert (o['call_kind'] == 3).any()


# ------------------------------------------------------------------------------------------------ gains on both sides of the Poisson table
GAINS = [216.9, 217.0, float(np.nextafter(217.0, np.inf)), 218.0, 300.0, 1000.0, 9.99, 10.0, 1e-3, 0.0]
AMPS = [60, 60, 60, 60, 60, 60, 400, 400, 3000, 50]


def _gain_case(gains=GAINS, run_sets=False, spread=0.0, seed=41):
    """S2s of the given secondary gains (ip['sc_gain'] per instruction) with S1s between them in loaded order (their emitters keep the NaN of
    em_zg: k_s2_photons must not touch them).  run_sets: the S2s 100 ns apart in one Pulse call, the S1s between them in key order."""
    rows = []
    drift = int(5.0 / B.xenonnt_test_config()['drift_velocity_liquid'])          # key of an S2 at z = -5: time + drift
    for k, (g, a) in enumerate(zip(gains, AMPS)):
        if run_sets:
            rows += [B.s2(a, gain=g, p=0.9, time=B.MS + 100 * k), B.s1(200 + 10 * k, exact=False, time=B.MS + drift + 100 * k + 50)]
        else:
            rows += [B.s2(a, gain=g, p=0.9), B.s1(200 + 10 * k, exact=False)]
    return B._case(rows, seed=seed, run_sets=run_sets, flat=True, s2_gain_spread=spread)


@pytest.mark.parametrize('run_sets,spread', [(False, 0.0), (True, 0.0), (False, 2.5), (True, 2.5)])
def test_gains_on_both_sides_of_the_poisson_table(run_sets, spread):
    """gains 216.9, 217, the next double, 218, 300, 1000 (table | PTRS), 9.99, 10 (numpy's own switch of methods), 1e-3 and 0; with
    s2_gain_spread = 2.5 both draws add int(2.5 z) and negative sums are clamped (gain 1e-3: about half of the electrons)"""
    case = _gain_case(run_sets=run_sets, spread=spread)
    cfg, res, s = B.prepared(case)
    orc, o = H.run_oracle(cfg, None, res, s)
    eng, counts = _device(cfg, res, s, profiling=True)
    t = _assert_case(case, cfg, s, orc, o, eng, counts)
    kt = eng.kernel_times()
    assert 'k_s2_photons' in kt and kt['k_s2_photons'][1] >= 1, sorted(kt)
    is_s2 = s['s_ins']['type'] == 2
    g = s['ip']['sc_gain'][is_s2]
    assert np.array_equal(np.sort(g), np.sort(GAINS)) and (g > 217.0).sum() == 4
    nph = t['ins_nph'][is_s2]
    assert nph[g >= 216.9].min() > 5000
    if spread == 0.0:
        assert nph[g == 0.0].sum() == 0
    else:
        assert nph[g == 1e-3].sum() > 300          # only the positive int(2.5 z) are left
    if run_sets:
        assert counts['n_pulse_sets'] < len(s['s_ins'])


def test_one_engine_across_the_poisson_table_limit():
    """One engine, three batches: gains on both sides of 217 (em_zg filled, k_s2_photons runs), every gain <= 217 with the same emitters (no
    fill, no k_s2_photons), the first batch again.  Each result is that of a fresh engine; k_s2_photons shows in batches 1 and 3 only."""
    mixed = _gain_case()
    low = _gain_case(gains=[min(g, 217.0) if g > 100 else g for g in GAINS])
    assert np.array_equal(mixed['ins']['amp'], low['ins']['amp'])
    eng = None
    seen = []
    for case in (mixed, low, mixed):
        cfg, res, s = B.prepared(case)
        eng, counts = _device(cfg, res, s, eng=eng, profiling=True)
        got = dict(counts=dict(counts), records=eng.records().tobytes(), ph=eng.photons(), kt=eng.kernel_times())
        new, ncounts = _device(cfg, res, s, profiling=True)
        assert got['counts'] == dict(ncounts)
        assert got['records'] == new.records().tobytes() and len(got['records']) > 0
        ph = new.photons()
        for f in ('set_off', 't', 'ch', 'gain', 'dpe'):
            assert np.array_equal(got['ph'][f], ph[f]), f
        assert ('k_s2_photons' in got['kt']) == ('k_s2_photons' in new.kernel_times())
        seen.append(got)
    assert 'k_s2_photons' in seen[0]['kt'] and 'k_s2_photons' not in seen[1]['kt'] and 'k_s2_photons' in seen[2]['kt'], [sorted(x['kt']) for x in seen]
    assert seen[0]['records'] == seen[2]['records'] and seen[0]['records'] != seen[1]['records']
    assert seen[0]['counts']['n_photons'] > seen[1]['counts']['n_photons']
