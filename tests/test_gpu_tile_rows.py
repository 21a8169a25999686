"""Rows read in place from the tile buffers of k_s2_tile and k_s2_bright (`src = 1` descriptors) at designed ZLE seams (MI355X only).

tests/tile_rows.py holds the sources, the families and the case table; tests/test_tile_rows_cpu.py says, from the oracle alone, that
every case reaches its seam and that nothing but the designed spikes makes a hit on a case row.  Here every source runs under every
family on the device, the oracle's ix_rand of every window injected (set_noise_offsets).  Exact equality everywhere: record bytes
against the oracle's, intervals() against its tuples, rows() sample by sample where the debug copy is on.  The paths:
  * debug copy off: k_zle on ZleFast where the hold-off is at least 63 and the table at least 512 rows, k_pack on its fast loads
  * debug copy on: the vector form of k_zle; the rows sample by sample
  * row_resident on, 1024- and (where the engine's rule admits resident rows) 256-sample segments: rows of one tile stay in their
    tile's buffer and rows that share tile-made pulses on accumulators (a finished tile keeps its row off the resident path); the S1
    rows of `mixed_window` go resident beside them
  * device record order (k_rec_keys)
That the rows WERE read in place is asserted: tile_kernels() names k_s2_tile / k_s2_bright for every tile the helper expected, k_tile_add
ran for `mixed_window` alone, and n_raw_samples counts the oracle's row samples.  The restatement of ins_bcap (acc_off % 4 of a case)
rests on the first and last electron of every instruction: electron_stats() against the oracle's.
"""
import numpy as np
import pytest

from tests import tile_rows as TR
from tests import zle_edges as ZE
from tests.helpers import canonical_intervals, make_engine, make_oracle
from tests.sum_signal import SUM_CHANNEL, assert_sum_rows, expected_sum_rows
from tests.test_gpu_parity import _nonempty_groups
from wfsim_amd.config import kernel_params

pytestmark = pytest.mark.gpu
PAIRS = [(s, f) for s in TR.SOURCES for f in TR.FAMILIES]


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _run(eng, s, debug):
    eng.set_debug(debug)
    eng.load_instructions(s['s_ins'], s['gid'], s['cluster'], s['key'], s['ip'])
    return eng.run()


def _engine(cfg, s, ix, mode, monkeypatch):
    """an engine on one digitisation path ('acc', 'res': row_resident on, 'res256': with 256-sample segments), profiling on, the
    noise start index of every window set"""
    if mode == 'res256':
        monkeypatch.setenv('WFS_RES_MAX_LEN', '256')
    else:
        monkeypatch.delenv('WFS_RES_MAX_LEN', raising=False)
    eng = make_engine(dict(cfg, row_resident=mode != 'acc'))
    eng.set_profiling(True)
    if ix is not None:
        _run(eng, s, False)                                 # (the windows of the batch: the start indices go in per window)
        g = eng.groups()
        full = np.full(len(g['left']), -1, dtype=np.int64)
        full[g['right'] >= g['left']] = ix
        eng.set_noise_offsets(full)
    return eng


def _check(eng, o, orc, what, sums=()):
    """intervals and record bytes against the oracle (the sum row, which the oracle does not make, against tests/sum_signal.py)"""
    g, keep = _nonempty_groups(eng)
    assert np.array_equal(g['left'][keep], o['dg_left']) and np.array_equal(g['right'][keep], o['dg_right']), what
    gmap = {int(gi): j for j, gi in enumerate(keep)}
    z = eng.intervals()
    sel = np.flatnonzero(z['channel'] != SUM_CHANNEL)
    got = sorted((gmap[int(z['group'][k])], int(z['channel'][k]), int(z['left'][k]), int(z['right'][k]),
                  np.asarray(z['data'][z['data_off'][k]:z['data_off'][k + 1]], dtype=np.int64).tobytes()) for k in sel)
    ref = canonical_intervals(o['zl_digit'], o['zl_ch'], o['zl_left'], o['zl_right'], o['zl_data_off'], o['zl_data'].astype(np.int16))
    assert len(got) == len(ref), (what, len(got), len(ref))
    for x, y in zip(got, ref):
        assert x == y, (what, 'window, channel, left, right', x[:4], y[:4])
    rec = eng.records()
    if sums:
        assert_sum_rows(eng, sums)
        rec = rec[rec['channel'] != SUM_CHANNEL]
    exp = np.frombuffer(orc.pack_records().tobytes(), dtype=rec.dtype)
    assert len(rec) == len(exp), (what, len(rec), len(exp))
    if rec.tobytes() != exp.tobytes():
        j = int(np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(rec, exp)])[0])
        raise AssertionError(f'{what}: record {j} differs (channel {exp["channel"][j]}, fragment {exp["record_i"][j]} of a pulse of {exp["pulse_length"][j]} '
                             f'at sample {exp["time"][j] // 10})')
    return len(ref), len(exp)


def _check_rows(eng, fam, o, sums, what):
    """rows() of a debug run sample by sample: every TPC row of the oracle (HE rows where the engine has them, the sum row)"""
    g, keep = _nonempty_groups(eng)
    gmap = {int(gi): j for j, gi in enumerate(keep)}
    want = {k: (v[0] - int(o['dg_left'][k[0]]), v[1]) for k, v in TR.finished_rows(o).items()}
    for e in sums:
        want[(e['window'], SUM_CHANNEL)] = (e['left'] - int(o['dg_left'][e['window']]), e['finished'])
    r = eng.rows()
    seen = set()
    for k in range(len(r['group'])):
        key = (gmap[int(r['group'][k])], int(r['channel'][k]))
        left, data = want[key]
        got = r['data'][r['data_off'][k]:r['data_off'][k] + r['right'][k] - r['left'][k] + 1].astype(np.int64)
        assert int(r['left'][k]) == left and len(got) == len(data), (what, key)
        if not np.array_equal(got, data):
            i = int(np.flatnonzero(got != data)[0])
            who = [c['name'] for c in fam.cases if (c['window'], c['channel']) == key]
            raise AssertionError(f'{what}: window {key[0]} channel {key[1]} {who}: sample {i} is {got[i]}, the oracle has {data[i]}')
        seen.add(key)
    assert {k for k in want if k[1] < fam.n_tpc or k[1] == SUM_CHANNEL} <= seen, what
    return len(seen)


def _assert_read_in_place(eng, fam, o, sums, what):
    g = fam.g
    kinds = eng.tile_kernels()
    direct = [r for r in g['rows'].values() if r['ch'] < fam.n_tpc and r['direct']]
    bad = [(r['window'], r['ch'], int(kinds[r['ins'], r['ch']]), r['kind']) for r in direct if kinds[r['ins'], r['ch']] != r['kind']]
    assert len(direct) >= 250 and not bad, (what, bad[:5])
    kt = eng.kernel_times()
    assert ('k_tile_add' in kt) == (fam.source == 'mixed_window'), (what, sorted(kt))
    for src, kernel in TR.KERNEL.items():
        if fam.source == src:
            assert kernel in kt and ('k_s2_tile' if kernel == 'k_s2_bright' else 'k_s2_bright') not in kt, (what, sorted(kt))
    tpc = sum(r['L'] for r in g['rows'].values() if r['ch'] < fam.n_tpc)
    assert eng.counts['n_raw_samples'] == tpc + sum(len(e['S']) for e in sums), (what, eng.counts['n_raw_samples'], tpc)
    es = eng.electron_stats()
    for q, c in enumerate(TR.HP.primary_calls(o)):          # what the restatement of ins_bcap rests on
        e = o['e_t'][o['call_e_off'][c]:o['call_e_off'][c + 1]]
        if not g['fused'][q]:
            continue
        assert (int(es[q, 2]), int(es[q, 3])) == (int(e.min()), int(e.max())), (what, q, es[q])


def _resident_admitted(fam):
    """the engine's rule for resident rows (wfs_engine.hip run_geometry: res_on)"""
    return fam.hold >= ZE.FAST_HOLD and fam.N >= ZE.NOISE_MIN_FAST and fam.name not in ('he801', 'sum801')


@pytest.mark.parametrize('source,family', PAIRS)
def test_designed_seams(source, family, monkeypatch):
    fam, cfg, orc, o = TR.oracle_run(source, family)
    s = fam.g['sched']
    sums = expected_sum_rows(o, kernel_params(cfg), orc.tables['thr_zle'], noise=cfg['noise_data'], ix_rand=fam.ix) if family == 'sum801' else []
    what = f'{source} / {family}'
    # ---- debug copy off, then on
    eng = _engine(cfg, s, fam.ix, 'acc', monkeypatch)
    _run(eng, s, False)
    assert np.array_equal(eng.groups()['ix_rand'][_nonempty_groups(eng)[1]], fam.ix)
    kt = eng.kernel_times()
    assert 'k_zle' in kt and 'k_pack' in kt and 'k_row_pulse' not in kt, (what, sorted(kt))
    _assert_read_in_place(eng, fam, o, sums, what)
    n_itv, n_rec = _check(eng, o, orc, what + ' (debug off)', sums)
    records = eng.records().tobytes()
    _run(eng, s, True)
    n_rows = _check_rows(eng, fam, o, sums, what + ' (debug on)')
    assert _check(eng, o, orc, what + ' (debug on)', sums) == (n_itv, n_rec) and eng.records().tobytes() == records
    # ---- device record order
    plain = eng.records()
    eng.set_record_order(True)
    try:
        _run(eng, s, False)
        assert 'k_rec_keys' in eng.kernel_times()
        ordered = eng.records()
    finally:
        eng.set_record_order(False)
    want = plain[np.lexsort((plain['channel'], plain['time']))]          # (lexsort is stable)
    assert len(ordered) == len(want) and ordered.tobytes() == want.tobytes(), what
    eng.close()
    # ---- resident rows asked for: rows of one tile stay where they are
    for mode in ('res', 'res256') if _resident_admitted(fam) else ('res',):
        eng = _engine(cfg, s, fam.ix, mode, monkeypatch)
        _run(eng, s, False)
        kt = eng.kernel_times()
        # (a tile whose pulse exists already keeps its row off the resident path, k_tile_rows: the shared rows of `mixed_window` stay
        # on accumulators; the rows of its small S1 go resident beside them)
        resident = source == 'mixed_window' and _resident_admitted(fam)
        assert ('k_row_pulse' in kt) == resident and ('k_pack_res' in kt) == resident, (what, mode, sorted(kt))
        _assert_read_in_place(eng, fam, o, sums, f'{what} ({mode})')
        assert _check(eng, o, orc, f'{what} ({mode})', sums) == (n_itv, n_rec) and eng.records().tobytes() == records
        eng.close()
    print(f'\n{what}: {len(fam.cases)} cases on {n_rows} rows, {n_itv} intervals, {n_rec} records per path; ZleFast '
          f'{"yes" if fam.hold >= ZE.FAST_HOLD and fam.N >= ZE.NOISE_MIN_FAST else "no"} (debug off), fast loads {"yes" if fam.N >= ZE.NOISE_MIN_FAST else "no"}')


@pytest.mark.parametrize('source', TR.NOISELESS)
def test_without_noise(source, monkeypatch):
    """enable_noise off (the benchmark's instantiation of the row kernels): per-channel thresholds that leave the 1, 2 or 3 deepest
    samples of every pulse as its only hits"""
    cfg, hits = TR.noiseless_config(source)
    fam = TR.Family(source, 'tw50')
    s = fam.g['sched']
    orc = make_oracle(cfg)
    orc.simulate(s['s_ins'], s['gid'], s['ip'])
    o = orc.results()
    assert len(o['zl_ch']) >= len(hits) > 400
    records = None
    for mode in ('acc', 'res', 'res256'):
        eng = _engine(cfg, s, None, mode, monkeypatch)
        _run(eng, s, False)
        _assert_read_in_place(eng, fam, o, [], f'{source} without noise ({mode})')
        n = _check(eng, o, orc, f'{source} without noise ({mode})')
        records = records or eng.records().tobytes()
        assert eng.records().tobytes() == records
        if mode == 'acc':
            _run(eng, s, True)
            _check_rows(eng, fam, o, [], f'{source} without noise (debug on)')
            assert _check(eng, o, orc, f'{source} without noise (debug on)') == n
            plain = eng.records()
            eng.set_record_order(True)
            _run(eng, s, False)
            ordered = eng.records()
            assert ordered.tobytes() == plain[np.lexsort((plain['channel'], plain['time']))].tobytes()
        eng.close()
    print(f'\n{source} without noise: {len(hits)} rows, {n[0]} intervals, {n[1]} records per path')
