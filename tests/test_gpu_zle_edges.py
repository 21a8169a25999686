"""The back end of a row on reference runs of rows DESIGNED sample by sample (MI355X only): finishing a sample, k_zle in its three forms,
the interval slots k_row_len reserves, k_rec_keys and the three packers.

tests/golden/zle_edges.npz (tests/zle_edges.py: the case table and the noise-table builder; tests/test_zle_edges_reference.py: the same
fixture on the oracle, and the coverage table that says every case reaches its seam).  A family -- one configuration with one noise table
-- is replayed as ONE batch: all its windows, so rows of every length and path sit next to each other in the accumulator and the loads
that run past a row's end read a neighbour's samples.  The reference's ix_rand of every window is injected (set_noise_offsets).  Exact
equality everywhere.  Per family:
  * accumulator rows, debug off: k_zle on ZleFast where the hold-off is at least 63 and the table at least 512 samples (the general
    form otherwise), k_pack on its fast loads (the general path for tables below 512): intervals against the reference's tuples, records
    against the numpy restatement of strax_interface.py:425-435 on those tuples
  * accumulator rows, debug on (k_zle's vector form): rows() sample by sample against the reference's finished rows as well, records
    the bytes of the debug-off run
  * resident rows, 1024- and 256-sample segments: k_row_pulse and k_pack_res are the kernels that ran wherever the engine's rule admits
    resident rows (hold-off >= 63, table >= 512, no HE rows) and are absent elsewhere; intervals and record bytes as above
  * device record order (k_rec_keys): a stable sort by (time, channel) of the unsorted run

The engine hands interval samples out as int16: the one designed sample above 32767 is compared there as the low 16 bits (what the
record holds too); rows() keeps it whole.  The log names rows, intervals and records per path (pytest -s).
"""
import numpy as np
import pytest

from tests import zle_edges as ZE
from tests.helpers import make_engine, replay_chain_on_engine, canonical_intervals
from tests.test_gpu_parity import _nonempty_groups
from tests.test_zle_edges_reference import fixture

pytestmark = pytest.mark.gpu

_engines = {}


def _engine(name, mode, monkeypatch):
    """one engine per family and digitisation path ('acc': accumulator rows; 'res' / 'res256': resident rows asked for, with the default /
    the 256-sample segment, which the library reads from WFS_RES_MAX_LEN when the engine is made), profiling on, the reference's noise
    start indices set.  Engines of one family at a time are kept."""
    for k in [k for k in _engines if k[0] != name]:
        _engines.pop(k)[0].close()
    if (name, mode) not in _engines:
        a, cfg0, fam, rows, index = fixture(name)
        cfg = dict(cfg0, row_resident=mode != 'acc')
        if mode == 'res256':
            monkeypatch.setenv('WFS_RES_MAX_LEN', '256')
        else:
            monkeypatch.delenv('WFS_RES_MAX_LEN', raising=False)
        eng = make_engine(cfg)
        eng.set_profiling(True)
        replay_chain_on_engine(eng, a, cfg, debug=False)            # (the windows of the batch: the start indices go in per window)
        g = eng.groups()
        ix = np.full(len(g['left']), -1, dtype=np.int64)
        ix[g['right'] >= g['left']] = a['dg_ix_rand']
        eng.set_noise_offsets(ix)
        _engines[(name, mode)] = (eng, cfg)
    return _engines[(name, mode)]


def _resident_admitted(fam):
    """the engine's rule for resident rows (wfs_engine.hip run_geometry: res_on)"""
    return fam.hold >= ZE.FAST_HOLD and fam.N >= ZE.NOISE_MIN_FAST and not fam.name.startswith('he')


def _reference_intervals(a):
    return canonical_intervals(a['zle_digit'], a['zle_ch'], a['zle_left'], a['zle_right'], a['zle_data_off'], a['zle_data'].astype(np.int16))


def _check_intervals_and_records(eng, a, cfg, what):
    g, keep = _nonempty_groups(eng)
    assert np.array_equal(g['left'][keep], a['dg_left']) and np.array_equal(g['right'][keep], a['dg_right']), what
    assert np.array_equal(g['ix_rand'][keep], a['dg_ix_rand']), what
    gmap = {int(gi): j for j, gi in enumerate(keep)}
    z = eng.intervals()
    got = canonical_intervals([gmap[int(x)] for x in z['group']], z['channel'], z['left'], z['right'], z['data_off'], z['data'])
    ref = _reference_intervals(a)
    assert len(got) == len(ref), (what, len(got), len(ref))
    for x, y in zip(got, ref):
        assert x == y, (what, 'window, channel, left, right', x[:4], y[:4])
    exp = ZE.expected_records(a, int(cfg.get('sample_duration', 10)))
    rec = eng.records()
    assert len(rec) == len(exp), (what, len(rec), len(exp))
    if rec.tobytes() != exp.tobytes():
        j = int(np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(rec, exp)])[0])
        raise AssertionError(f'{what}: record {j} differs (channel {exp["channel"][j]}, fragment {exp["record_i"][j]} of a pulse of {exp["pulse_length"][j]} '
                             f'at sample {exp["time"][j] // 10})')
    return len(ref), len(exp)


@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_accumulator_rows(name, monkeypatch):
    """debug off, then debug on: the rows sample by sample, the same record bytes"""
    a, _, fam, rows, index = fixture(name)
    eng, cfg = _engine(name, 'acc', monkeypatch)
    replay_chain_on_engine(eng, a, cfg, debug=False)
    kt = eng.kernel_times()
    assert 'k_zle' in kt and 'k_pack' in kt and 'k_row_pulse' not in kt and 'k_pack_res' not in kt, sorted(kt)
    n_itv, n_rec = _check_intervals_and_records(eng, a, cfg, f'{name} (accumulator rows, debug off)')
    records = eng.records().tobytes()
    # ---- debug on
    replay_chain_on_engine(eng, a, cfg, debug=True)
    g, keep = _nonempty_groups(eng)
    gmap = {int(gi): j for j, gi in enumerate(keep)}
    r = eng.rows()
    got = {(gmap[int(r['group'][k])], int(r['channel'][k])): (int(r['left'][k]), r['data'][r['data_off'][k]:r['data_off'][k] + r['right'][k] - r['left'][k] + 1].astype(np.int64))
           for k in range(len(r['group']))}
    assert len(got) == len(rows) == len(r['group'])
    for row in rows:
        left, data = got[(row['window'], row['channel'])]
        assert left == row['abs'] - int(a['dg_left'][row['window']]) and len(data) == len(row['data']), (name, row['window'], row['channel'])
        if not np.array_equal(data, row['data']):
            i = int(np.flatnonzero(data != row['data'])[0])
            who = [c['name'] for c in fam.cases if c['window'] == row['window'] and c['channel'] in (row['channel'], row['channel'] - fam.he_first)]
            raise AssertionError(f'{name}: window {row["window"]} channel {row["channel"]} {who}: sample {i} is {data[i]}, the reference has {row["data"][i]}')
    assert _check_intervals_and_records(eng, a, cfg, f'{name} (accumulator rows, debug on)') == (n_itv, n_rec)
    assert eng.records().tobytes() == records
    print(f'\n{name}: accumulator rows, debug off and on: {len(rows)} rows, {len(a["row_data"])} samples, {n_itv} intervals, {n_rec} records; '
          f'ZleFast {"yes" if fam.hold >= ZE.FAST_HOLD and fam.N >= ZE.NOISE_MIN_FAST else "no"} (debug off), fast loads {"yes" if fam.N >= ZE.NOISE_MIN_FAST else "no"}')


@pytest.mark.parametrize('mode', ['res', 'res256'])
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_resident_rows(name, mode, monkeypatch):
    """row_resident=True: k_row_pulse / k_pack_res where the engine's rule admits resident rows, the accumulator kernels alone where it
    does not (short tables, short hold-offs, HE rows) -- the same intervals and record bytes either way"""
    a, _, fam, rows, index = fixture(name)
    eng_a, cfg_a = _engine(name, 'acc', monkeypatch)
    replay_chain_on_engine(eng_a, a, cfg_a, debug=False)
    records = eng_a.records().tobytes()
    eng, cfg = _engine(name, mode, monkeypatch)
    replay_chain_on_engine(eng, a, cfg, debug=False)
    kt = eng.kernel_times()
    if _resident_admitted(fam):
        assert 'k_row_pulse' in kt and 'k_pack_res' in kt, (name, mode, sorted(kt))
    else:
        assert 'k_row_pulse' not in kt and 'k_pack_res' not in kt and 'k_zle' in kt and 'k_pack' in kt, (name, mode, sorted(kt))
    n_itv, n_rec = _check_intervals_and_records(eng, a, cfg, f'{name} ({mode})')
    assert eng.records().tobytes() == records, (name, mode)
    counts = eng.counts
    print(f'\n{name} / {mode}: {len(rows)} rows, {n_itv} intervals, {n_rec} records; resident rows {"admitted" if _resident_admitted(fam) else "off by the rule"}; '
          f'kernels {sorted(k for k in kt if k in ("k_row_pulse", "k_pack_res", "k_zle", "k_pack", "k_rec_keys"))}; counts {counts["n_rows"]} rows')


@pytest.mark.parametrize('mode', ['acc', 'res'])
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_device_record_order(name, mode, monkeypatch):
    """set_record_order(True): the records leave in (time, channel) order through k_rec_keys -- a stable sort of the unsorted run"""
    a, _, fam, rows, index = fixture(name)
    eng, cfg = _engine(name, mode, monkeypatch)
    replay_chain_on_engine(eng, a, cfg, debug=False)
    plain = eng.records()
    eng.set_record_order(True)
    try:
        replay_chain_on_engine(eng, a, cfg, debug=False)
        assert 'k_rec_keys' in eng.kernel_times()
        ordered = eng.records()
    finally:
        eng.set_record_order(False)
    want = plain[np.lexsort((plain['channel'], plain['time']))]          # (lexsort is stable)
    assert len(ordered) == len(want) and ordered.tobytes() == want.tobytes(), (name, mode)
    assert np.any(np.diff(plain['time']) < 0) or len(plain) < 2             # (the unsorted run is not in time order already)
