"""Full readout on the designed rows of tests/golden/zle_edges.npz (MI355X only): k_row_empty and the rows k_rows_widen widens on the
seams the reference's rows were designed for.

tests/full_readout_edges.py builds, per family, one batch with one digitise window per case, in two forms: 'transposed' -- the case's
weak pair sits on a carrier channel with an all-zero noise column, so the case channel has no pulse and its row is made by
k_row_empty -- and 'widened' -- the case channel gets two weak photons in one bin in the middle of the range besides, so its row has
one tile that is shorter than the row and begins behind its first sample.  The engine runs the input as it is with full_readout=True
and the reference's ix_rand of every window injected; tests/test_full_readout_edges_cpu.py shows on the CPU that the anchored oracle
then has the reference's rows and records on every case channel.  Exact equality everywhere:
  * the whole batch's record bytes against the anchored oracle's, the case channels' records against the REFERENCE's
    (full_readout_edges.assert_case_records: one definition for the CPU and the GPU tests)
  * accumulator rows with the debug copy: rows() lists the rows with pulses at the window's range; in 'widened' every case row sample
    by sample against the reference's finished row (the finished 32768 whole)
  * resident rows with the default and the 256-sample segment, device record order, and the switch off on the same input
The log names rows, intervals and records per path (pytest -s).
"""
import numpy as np
import pytest

from tests import full_readout_edges as FE
from tests import zle_edges as ZE
from tests.helpers import make_engine
from tests.noise_model import oracle_rows
from tests.test_gpu_noise_model import _as_records, _oracle_photons
from tests.test_gpu_parity import _nonempty_groups
from tests.test_gpu_zle_edges import _resident_admitted

pytestmark = pytest.mark.gpu

_engines, _expected = {}, {}


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _oracle(name, form):
    """records of the anchored and of the plain oracle and the plain oracle's rows, computed once per family and form"""
    for k in [k for k in _expected if k[0] != name]:
        del _expected[k]
    if (name, form) not in _expected:
        b = FE.batch(name, form)
        full = _oracle_photons(b['cfg'], b['anchored'], b['ix'])
        plain = _oracle_photons(b['cfg'], b['calls'], b['ix'])
        o = {k: plain.get(k) for k in ('dg_left', 'dg_right', 'dg_row_off', 'row_ch', 'row_left', 'row_right')}
        _expected[(name, form)] = dict(full=full.pack_records().tobytes(), plain=plain.pack_records().tobytes(), plain_rows=oracle_rows(o),
                                       dg_left=full.get('dg_left'), dg_right=full.get('dg_right'))
        full.close(), plain.close()
    return _expected[(name, form)]


def _replay(eng, b, debug=False):
    eng.set_debug(debug)
    eng.load_photons(*b['sets'])
    return eng.run()


def _engine(name, form, mode, monkeypatch):
    """one engine per family, form and digitisation path ('acc': accumulator rows; 'res' / 'res256': resident rows asked for, with the
    default / the 256-sample segment, read from WFS_RES_MAX_LEN when the engine is made), full readout and profiling on, the
    reference's noise start indices set.  Engines of one family at a time are kept."""
    for k in [k for k in _engines if k[0] != name]:
        _engines.pop(k).close()
    if (name, form, mode) not in _engines:
        b = FE.batch(name, form)
        if mode == 'res256':
            monkeypatch.setenv('WFS_RES_MAX_LEN', '256')
        else:
            monkeypatch.delenv('WFS_RES_MAX_LEN', raising=False)
        eng = make_engine(dict(b['cfg'], row_resident=int(mode != 'acc'), full_readout=True))
        eng.set_profiling(True)
        _replay(eng, b)                                    # (the windows of the batch: the start indices go in per window)
        g, keep = _nonempty_groups(eng)
        assert len(keep) == len(b['cases'])
        ix = np.full(len(g['left']), -1, dtype=np.int64)
        ix[keep] = b['ix']
        eng.set_noise_offsets(ix)
        _engines[(name, form, mode)] = eng
    return _engines[(name, form, mode)]


def _slots(b):
    """row slots of a window: the TPC channels, and the HE rows of the top channels where they can differ from a flat baseline (an HE
    factor, or noise columns for them: wfs_engine.hip he_rows)"""
    he_rows = int(b['p']['he_factor']) != 0 or b['fam'].columns > b['fam'].he_first
    assert he_rows == b['name'].startswith('he')
    return int(b['p']['n_tpc']) + (int(b['p']['n_top']) if he_rows else 0)


def _check_windows(eng, b, e):
    g, keep = _nonempty_groups(eng)
    assert np.array_equal(g['left'][keep], e['dg_left']) and np.array_equal(g['right'][keep], e['dg_right']) and np.array_equal(g['ix_rand'][keep], b['ix'])
    return {int(gi): j for j, gi in enumerate(keep)}


def _first_difference(rec, exp):
    if len(rec) != len(exp):
        return f'{len(rec)} records against {len(exp)}'
    j = int(np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(rec, exp)])[0])
    return f'record {j} differs (channel {exp["channel"][j]}, fragment {exp["record_i"][j]} of a pulse of {exp["pulse_length"][j]} at time {exp["time"][j]})'


def _check_records(eng, b, e, what):
    rec = eng.records()
    if rec.tobytes() != e['full']:
        FE.assert_case_records(rec, b, what)            # (names the case, if a case channel differs)
        raise AssertionError(f'{what}: {_first_difference(rec, _as_records(np.frombuffer(e["full"], np.uint8)))}')
    return rec, FE.assert_case_records(rec, b, what)


@pytest.mark.parametrize('form', FE.FORMS)
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_accumulator_rows(name, form, monkeypatch):
    """debug off, then debug on: the rows with pulses sample by sample, the same record bytes"""
    b, e = FE.batch(name, form), _oracle(name, form)
    fam = b['fam']
    eng = _engine(name, form, 'acc', monkeypatch)
    counts = _replay(eng, b)
    kt = eng.kernel_times()
    assert {'k_row_empty', 'k_rows_widen', 'k_pack_res'} <= set(kt) and 'k_row_pulse' not in kt, sorted(kt)
    assert counts['n_rows'] == len(b['cases']) * _slots(b)
    _check_windows(eng, b, e)
    rec, n_case = _check_records(eng, b, e, 'accumulator rows, debug off')
    n_itv = counts['n_intervals']
    # ---- debug on
    counts = _replay(eng, b, debug=True)
    gmap = _check_windows(eng, b, e)
    r = eng.rows()
    got = {(gmap[int(r['group'][k])], int(r['channel'][k])): (int(r['left'][k]), r['data'][r['data_off'][k]:r['data_off'][k] + r['right'][k] - r['left'][k] + 1].astype(np.int64))
           for k in range(len(r['group']))}
    assert len(got) == len(r['group']) and set(got) == {(w, ch) for w, ch, _, _ in e['plain_rows']}         # the rows WITH pulses ...
    for (w, ch), (left, data) in got.items():
        first, row = b['cases'][w]['rows'][b['cases'][w]['case']['channel']]
        assert int(e['dg_left'][w]) + left == first and len(data) == len(row['data']), (name, form, w, ch)       # ... at the window's range
    compared = 0
    for w, c in enumerate(b['cases']):
        for ch, (first, row) in c['rows'].items():
            if (w, ch) not in got:
                assert form == 'transposed' and not c['real']
                continue
            data = got[(w, ch)][1]
            if not np.array_equal(data, row['data']):
                i = int(np.flatnonzero(data != row['data'])[0])
                raise AssertionError(f'{name} / {form}: case {c["case"]["name"]} channel {ch}: sample {i} is {data[i]}, the reference has {row["data"][i]}')
            compared += 1
    assert compared == (sum(len(c['rows']) for c in b['cases']) if form == 'widened' else sum(len(c['rows']) for c in b['cases'] if c['real']))
    assert eng.records().tobytes() == rec.tobytes() and counts['n_intervals'] == n_itv
    print(f'\n{name} / {form}: accumulator rows, debug off and on: {len(b["cases"])} windows, {counts["n_rows"]} rows ({len(got)} with pulses, {compared} case rows '
          f'compared sample by sample), {n_itv} intervals, {len(rec)} records ({n_case} of them the reference\'s)')


@pytest.mark.parametrize('mode', ['res', 'res256'])
@pytest.mark.parametrize('form', FE.FORMS)
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_resident_rows(name, form, mode, monkeypatch):
    """row_resident=1: the rows with pulses through k_row_pulse where the engine's rule admits resident rows (every window has one
    that qualifies: the carrier's), through the accumulators elsewhere -- the accumulator run's record bytes either way"""
    b, e = FE.batch(name, form), _oracle(name, form)
    eng_a = _engine(name, form, 'acc', monkeypatch)
    _replay(eng_a, b)
    records = eng_a.records().tobytes()
    eng = _engine(name, form, mode, monkeypatch)
    counts = _replay(eng, b)
    kt = eng.kernel_times()
    assert {'k_row_empty', 'k_rows_widen', 'k_pack_res'} <= set(kt), sorted(kt)
    assert ('k_row_pulse' in kt) == _resident_admitted(b['fam']), (name, form, mode, sorted(kt))
    assert counts['n_rows'] == len(b['cases']) * _slots(b)
    _check_windows(eng, b, e)
    rec, n_case = _check_records(eng, b, e, mode)
    assert rec.tobytes() == records
    print(f'\n{name} / {form} / {mode}: {counts["n_rows"]} rows, {counts["n_intervals"]} intervals, {len(rec)} records ({n_case} the reference\'s); resident rows '
          f'{"admitted" if _resident_admitted(b["fam"]) else "off by the rule"}; kernels {sorted(k for k in kt if k in ("k_row_empty", "k_rows_widen", "k_row_pulse", "k_pack_res", "k_zle", "k_pack"))}')


@pytest.mark.parametrize('mode', ['acc', 'res'])
@pytest.mark.parametrize('form', FE.FORMS)
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_device_record_order(name, form, mode, monkeypatch):
    """set_record_order(True): the records leave in (time, channel) order through k_rec_keys -- a stable sort of the unsorted run"""
    b = FE.batch(name, form)
    eng = _engine(name, form, mode, monkeypatch)
    _replay(eng, b)
    plain = eng.records()
    eng.set_record_order(True)
    try:
        _replay(eng, b)
        assert 'k_rec_keys' in eng.kernel_times()
        ordered = eng.records()
    finally:
        eng.set_record_order(False)
    want = plain[np.lexsort((plain['channel'], plain['time']))]          # (lexsort is stable)
    assert len(ordered) == len(want) and ordered.tobytes() == want.tobytes(), (name, form, mode)
    assert np.any(np.diff(plain['time']) < 0)                               # (the unsorted run is not in time order already)


@pytest.mark.parametrize('mode', ['acc', 'res'])
@pytest.mark.parametrize('form', FE.FORMS)
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_switch_off_same_input(name, form, mode, monkeypatch):
    """the same engine on the same input with the switch off: the plain oracle's records, neither kernel of full readout ran"""
    b, e = FE.batch(name, form), _oracle(name, form)
    eng = _engine(name, form, mode, monkeypatch)
    eng.set_full_readout(False)
    try:
        counts = _replay(eng, b)
        kt = eng.kernel_times()
        rec = eng.records()
    finally:
        eng.set_full_readout(True)
    assert not {'k_row_empty', 'k_rows_widen'} & set(kt), sorted(kt)
    assert counts['n_rows'] == len(e['plain_rows'])
    if rec.tobytes() != e['plain']:
        raise AssertionError(f'{name} / {form} / {mode}, switch off: {_first_difference(rec, _as_records(np.frombuffer(e["plain"], np.uint8)))}')
    assert e['plain'] != e['full']
