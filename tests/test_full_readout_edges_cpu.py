"""Full readout on the designed rows of tests/golden/zle_edges.npz: what the GPU pin of tests/test_gpu_full_readout_edges.py rests on,
checked on the oracle alone (tests/full_readout_edges.py builds the batches).  CPU only.

Per family and form the anchored oracle -- two photons of gain 0 on every TPC channel at the carrier pair's times -- must have one
window per case with the designed range and ix_rand, the case channel's row where the reference had it (shifted by an even number of
samples), and, for every case, on its channel and its HE channel, the reference's records byte for byte.  No case is left out.  The
seams each case reaches are those tests/test_zle_edges_reference.py::test_every_case_reaches_its_seam proves on the same rows: same
range, same ix_rand, same column, hence the same finished samples; they are not restated here.
"""
import numpy as np
import pytest

from tests import full_readout_edges as FE
from tests import zle_edges as ZE
from tests.noise_model import oracle_rows
from tests.test_gpu_noise_model import _oracle_photons, _as_records
from tests.test_zle_edges_reference import fixture

_runs = {}


def _run(name, form):
    """the anchored and the plain oracle on one batch: windows, rows (without their samples) and records"""
    if (name, form) not in _runs:
        b = FE.batch(name, form)
        out = {}
        for key, calls in (('full', b['anchored']), ('plain', b['calls'])):
            orc = _oracle_photons(b['cfg'], calls, b['ix'])
            o = {k: orc.get(k) for k in ('dg_left', 'dg_right', 'dg_ix_rand', 'dg_row_off', 'row_ch', 'row_left', 'row_right')}
            out[key] = dict(o=o, rows={(w, ch): (first, n) for w, ch, first, n in oracle_rows(o)}, rec=_as_records(orc.pack_records()))
            orc.close()
        _runs[(name, form)] = out
    return _runs[(name, form)]


@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_carrier(name):
    a, cfg, fam, rows, index = fixture(name)
    ch = FE.carrier_of(name)
    assert ch >= ZE.FIRST_BOTTOM and ch < fam.he_first
    assert ch not in {c['channel'] for c in fam.cases} and ch not in fam.special and ch not in ZE.SPECIAL_CHANNELS
    assert not cfg['noise_data'][:, ch].any() and cfg['gains'][ch] > 0
    # a PMT of gain 0 has no row in the oracle and a row of noise in the engine: its column is zero, neither side has a record there
    dead = np.flatnonzero(np.asarray(cfg['gains']) <= 0)
    assert not set(dead.tolist()) & {c['channel'] for c in fam.cases}
    for c in dead:
        assert not cfg['noise_data'][:, c].any()
        assert fam.he_first + c >= fam.columns or not cfg['noise_data'][:, fam.he_first + c].any()


@pytest.mark.parametrize('form', FE.FORMS)
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_anchored_oracle_gives_the_reference_rows_and_records(name, form):
    b = FE.batch(name, form)
    fam, r = b['fam'], _run(name, form)
    o, full, plain = r['full']['o'], r['full']['rows'], r['plain']['rows']
    assert len(o['dg_left']) == len(b['cases']) == len(fam.cases) == len(r['plain']['o']['dg_left'])
    assert np.array_equal(o['dg_ix_rand'], b['ix']) and np.array_equal(r['plain']['o']['dg_ix_rand'], b['ix'])
    live = np.asarray(b['cfg']['gains'])[:int(b['p']['n_tpc'])] > 0
    for k, c in enumerate(b['cases']):
        case = c['case']
        left, right = FE.designed_window(c)
        assert (int(o['dg_left'][k]), int(o['dg_right'][k])) == (left, right), (name, form, case['name'])
        assert c['ix_rand'] == fam.windows[case['window']]['ix_rand']
        assert c['rows'] and case['channel'] in c['rows']
        for ch, (first, row) in c['rows'].items():
            assert full[(k, ch)] == (first, len(row['data'])), (name, form, case['name'], ch)
            assert first == case['row_abs'] + c['offset'] // fam.dt and len(row['data']) == case['length']
        # every live TPC channel has a row of that range
        assert sum(1 for ch in np.flatnonzero(live) if full.get((k, int(ch))) == full[(k, case['channel'])]) == int(live.sum())
        if form == 'transposed':
            assert ((k, case['channel']) in plain) == c['real'], (name, case['name'])
        else:
            (first, n), (f0, n0) = plain[(k, case['channel'])], full[(k, case['channel'])]
            assert f0 <= first and first + n <= f0 + n0
            if not c['real'] and case['length'] - fam.min_len >= 2:         # the row's own pulse begins behind the row and is shorter
                assert first == f0 + (case['length'] - fam.min_len) // 2 and n == fam.min_len < n0
        assert (k, b['carrier']) in plain
    assert FE.assert_case_records(r['full']['rec'], b, 'anchored oracle') == len(ZE.expected_records(fixture(name)[0], fam.dt))
    assert np.all(np.diff((r['full']['rec']['time'] + ZE.GROUP_SPACING // 2) // ZE.GROUP_SPACING) >= 0)      # window by window


@pytest.mark.parametrize('form', FE.FORMS)
def test_no_case_is_left_out(form):
    """481 cases and 2499 case records over the 14 families"""
    n_cases = sum(len(FE.batch(name, form)['cases']) for name in ZE.FAMILIES)
    n_rec = sum(FE.assert_case_records(_run(name, form)['full']['rec'], FE.batch(name, form)) for name in ZE.FAMILIES)
    assert len(ZE.FAMILIES) == 14 and n_cases == FE.N_CASES and n_rec == FE.N_CASE_RECORDS
    real = [c['case']['name'] for name in ZE.FAMILIES for c in FE.batch(name, form)['cases'] if c['real']]
    assert real and all(n.startswith(('pulse_peak_', 'clamp_pulse_', 'he_huge_pulse_')) for n in real)
