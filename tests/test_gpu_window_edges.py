"""The digitise-window rule of the HIP path (k_tile_geom, k_groups, k_tile_rows, k_group_final, k_row_len, the host's batch cuts and
wfs_set_window_carry) on reference runs of designed instruction spacings (MI355X only).

tests/golden/window_edges.npz (nVeto configuration, right_raw_extension 2000) and window_edges_tpc.npz (bundled TPC configuration,
right_raw_extension 100000): the reference's RawDataOptical with pmt_transit_time_spread 0 on the case table of tests/window_edges.py;
tests/test_window_edges_reference.py holds the fixtures' intended content and pins the oracle and the host scheduler on them.  As that
file's coverage test computes from the fixtures' own instruction times and pulse ends, the decisions (tmin - last_pulse_end_time -
right_raw_extension; the cache is digitised when > 0) sit at
    window_edges.npz      78 decisions:  6 at -1 ns,  6 at 0 ns,  10 at +1 ns
    window_edges_tpc.npz  33 decisions:  3 at -1 ns,  3 at 0 ns,   3 at +1 ns
Before these fixtures the decision nearest to the threshold in any reference run of the suite was 131 ns away (chain_optical_cutoff.npz;
160 ns in chain_optical.npz, about 9 x 10^5 ns in chain_s1.npz), and no batch of more clusters than k_groups has threads was compared
with anything exact.

Here: the recorded photons and gains replayed (debug copies on: pulses, windows, rows, ZLE intervals, data, and k_groups' flag of every
cluster against the reference's verdict; debug copies off, both row paths, both arithmetic forms: records fragment by fragment), our own
optical path on the stored inputs, the same cut into batches, the carry set directly, and the stream tiled to 1023 .. 3073 clusters --
more than k_groups has threads, so that a thread walks several clusters -- with clusters without pulses shifting every decision through
every position of a thread's range.  All comparisons are integer or byte equality.
"""
import numpy as np
import pytest

import wfsim_amd
from tests import window_edges as WE
from tests.helpers import golden, make_engine, make_oracle, replay_chain_on_engine, replay_chain_on_oracle, window_edges_config, with_fma
from tests.test_gpu_parity import _check_chain_mode, _nonempty_groups
from wfsim_amd.dtypes import raw_record_dtype

pytestmark = pytest.mark.gpu

NAMES = ['nveto', 'tpc']
GROUPS_TPB = 1024           # threads of k_groups (wfsim_amd/csrc/wfs_kernels.h)
_engines, _fixtures, _full = {}, {}, {}


def fixture(name):
    if name not in _fixtures:
        d = golden(WE.FIXTURES[name])
        cfg = window_edges_config(name)
        dt, rext = int(cfg['sample_duration']), int(cfg['right_raw_extension'])
        _fixtures[name] = (d, cfg, dt, rext, WE.fixture_decisions(d, rext, dt))
    return _fixtures[name]


def engine(name, fma=True, row_resident=False):
    key = (name, fma, row_resident)
    if key not in _engines:
        cfg = with_fma(window_edges_config(name, row_resident=row_resident), fma)
        _engines[key] = (make_engine(cfg), cfg)
    eng, cfg = _engines[key]
    eng.set_window_carry(0, 0)
    eng.set_profiling(False)
    return eng, cfg


def cluster_flags(eng, n_clusters):
    """k_groups' verdict per cluster of the last batch: whether it opened a new group"""
    g = eng.cluster_groups(n_clusters)
    return np.diff(np.concatenate([[0], g])) > 0


def assert_records_are_the_zle_tuples(rec, d, dt):
    """the records are the fixture's ZLE tuples fragment by fragment, in the reference's yield order"""
    spr = np.dtype(raw_record_dtype())['data'].shape[0]
    plen = d['zle_right'] - d['zle_left'] + 1
    nfrag = -(-plen // spr)
    assert len(rec) == nfrag.sum()
    iv = np.repeat(np.arange(len(plen)), nfrag)
    frag = np.arange(len(rec)) - np.repeat(np.cumsum(nfrag) - nfrag, nfrag)
    assert np.array_equal(rec['record_i'], frag) and np.array_equal(rec['channel'], d['zle_ch'][iv])
    assert np.array_equal(rec['time'], dt * (d['zle_left'][iv] + spr * frag))
    assert np.array_equal(rec['pulse_length'], plen[iv]) and np.array_equal(rec['length'], np.minimum(spr, plen[iv] - spr * frag))
    assert np.all(rec['dt'] == dt) and np.all(rec['baseline'] == 0)
    data = np.concatenate([rec['data'][k][:rec['length'][k]] for k in range(len(rec))])
    assert np.array_equal(data, d['zle_data'])
    assert all(not rec['data'][k][rec['length'][k]:].any() for k in range(len(rec)))


# ------------------------------------------------------------------------------------------------ replay of the recorded photons
@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
@pytest.mark.parametrize('name', NAMES)
def test_replay_with_debug_copies(name, fma):
    """pulses, groups() left / right, rows, ZLE intervals and data equal the fixture (_check_chain_mode); every cluster's flag out of
    k_groups is the reference's verdict on that decision"""
    d, cfg0, dt, rext, dec = fixture(name)
    eng, cfg = engine(name, fma)
    _check_chain_mode(None, cfg, d=d, eng=eng)
    flags = cluster_flags(eng, len(dec))
    assert flags.tolist() == [x['flush'] for x in dec]
    assert eng.counts['n_groups'] == sum(x['flush'] for x in dec) + 1


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
@pytest.mark.parametrize('row_resident', [True, False], ids=['resident', 'accumulators'])
@pytest.mark.parametrize('name', NAMES)
def test_replay_records(name, row_resident, fma):
    """without debug copies, rows resident (k_row_pulse) and in the accumulators: records and windows equal the fixture"""
    d, cfg0, dt, rext, dec = fixture(name)
    eng, cfg = engine(name, fma, row_resident)
    replay_chain_on_engine(eng, d, cfg, debug=False)
    rec = eng.records()
    assert_records_are_the_zle_tuples(rec, d, dt)
    g, keep = _nonempty_groups(eng)
    assert np.array_equal(g['left'][keep], d['dg_left']) and np.array_equal(g['right'][keep], d['dg_right'])
    assert cluster_flags(eng, len(dec)).tolist() == [x['flush'] for x in dec]
    eng.set_profiling(True)
    eng.run()
    kt = eng.kernel_times()
    assert ('k_row_pulse' in kt) == row_resident, sorted(kt)
    assert eng.records().tobytes() == rec.tobytes()


# ------------------------------------------------------------------------------------------------ our own optical path
def run_optical(cfg, ins, channels, timings, max_batch_quanta=None, log=None):
    """(windows [(left, right)], record bytes, the RawDataOptical) of wfsim_amd.RawDataOptical.iter_windows; log: list that receives the
    (start, stop) of every batch the host considered"""
    rd = wfsim_amd.RawDataOptical(cfg, channels=channels, timings=timings)
    if max_batch_quanta is not None:
        rd.max_batch_quanta = max_batch_quanta
    if log is not None:
        batch_end = rd._batch_end

        def logged(start, *a, **k):
            stop = batch_end(start, *a, **k)
            log.append((int(start), int(stop)))
            return stop
        rd._batch_end = logged
    windows = list(rd.iter_windows(ins))
    rec = np.concatenate([w['records'] for w in windows]) if windows else np.zeros(0, dtype=raw_record_dtype())
    return [(w['left'], w['right']) for w in windows], rec.tobytes(), rd


def oracle_optical(cfg, ins, channels, timings, cutoff):
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, cutoff)
    return orc.results(), orc.pack_records().tobytes()


def full_optical_run(name):
    """the single-batch run of the stored inputs and the oracle's (accumulator rows: every pulse is on the engine's tile list)"""
    if name not in _full:
        d, cfg0, dt, rext, dec = fixture(name)
        cfg = dict(cfg0, seed=71, row_resident=False)
        windows, rec, rd = run_optical(cfg, d['instructions'], d['channels'], d['timings'])
        p = rd.engine.pulses()
        flags = cluster_flags(rd.engine, len(dec))
        o, orec = oracle_optical(cfg, d['instructions'], d['channels'], d['timings'], int(d['cutoff']))
        _full[name] = (cfg, windows, rec, p, flags, o, orec)
    return _full[name]


@pytest.mark.parametrize('name', NAMES)
def test_own_optical_path(name):
    """RawDataOptical.iter_windows on the stored instructions, channels and timings: with spread 0 the photon times are the fixture's, so
    windows and the pulse bounds of every call equal the fixture; the gains are ours, so the records equal the oracle's bytes"""
    d, cfg0, dt, rext, dec = fixture(name)
    cfg, windows, rec, p, flags, o, orec = full_optical_run(name)
    assert windows == list(zip(d['dg_left'].tolist(), d['dg_right'].tolist()))
    order = np.lexsort((p['channel'], p['set']))
    call_of_pulse = np.repeat(np.arange(len(d['call_kind'])), np.diff(d['call_pulse_off']))
    assert np.array_equal(p['set'][order], call_of_pulse) and np.array_equal(p['channel'][order], d['pl_ch'])
    assert np.array_equal(p['left'][order], d['pl_left']) and np.array_equal(p['right'][order], d['pl_right'])
    assert np.array_equal(p['n_photons'][order], d['pl_photons'])
    assert flags.tolist() == [x['flush'] for x in dec]
    assert np.array_equal(o['dg_left'], d['dg_left']) and np.array_equal(o['dg_right'], d['dg_right'])
    assert rec == orec and len(rec) > 0
    # resident rows: the same windows and bytes
    w2, rec2, _ = run_optical(dict(cfg, row_resident=True), d['instructions'], d['channels'], d['timings'])
    assert w2 == windows and rec2 == rec


@pytest.mark.parametrize('quanta', [1, 2, 3, 7, 40])
@pytest.mark.parametrize('name', NAMES)
def test_batch_cuts(name, quanta):
    """the same run cut into batches (max_batch_quanta 1: a batch is one cluster unless its window is still open): windows and record
    bytes are those of the single batch.  With 1, a cut falls directly before and directly behind every section-A decision"""
    d, cfg0, dt, rext, dec = fixture(name)
    cfg, windows, rec, p, flags, o, orec = full_optical_run(name)
    log = []
    w, r, rd = run_optical(cfg, d['instructions'], d['channels'], d['timings'], max_batch_quanta=quanta, log=log)
    assert w == windows and r == rec
    cuts = {a for a, b in log} | {b for a, b in log}
    assert len(log) >= 2                  # (more than one batch)
    if quanta == 1:
        a_dec = np.flatnonzero((d['dec_section'] == WE.SECTIONS.index('A')) & d['dec_has_delta'])
        assert len(a_dec) == 9
        for c in a_dec:
            assert int(d['dec_first'][c]) in cuts and int(d['dec_first'][c] + d['dec_n'][c]) in cuts, c


# ------------------------------------------------------------------------------------------------ the carry, directly
def tail_of(d, k0, cfg):
    """the recorded calls from call k0 on as a batch of their own (what replay_chain_on_engine reads)"""
    from wfsim_amd.scheduler import schedule
    ins = d['instructions'][k0:]
    order, key, cluster = schedule(ins, cfg)
    assert np.array_equal(order, np.arange(len(ins)))
    a = int(d['call_ph_off'][k0])
    return dict(set_cluster=cluster.astype(np.int32), set_tmin=key.astype(np.int64), call_ph_off=d['call_ph_off'][k0:] - a,
                call_has_gains=d['call_has_gains'][k0:], ph_t=d['ph_t'][a:], ph_ch=d['ph_ch'][a:], ph_dpe=d['ph_dpe'][a:], ph_gain=d['ph_gain'][a:])


@pytest.mark.parametrize('name', NAMES)
def test_carry_set_directly(name):
    """the stream from a cluster on, alone through load_photons behind set_window_carry.  With the running maximum of the fixture's first
    part, and with carries that put the first decision at -1, 0 and +1 ns: only at +1 (and with the fixture's own, which is beyond) does the
    first cluster open a new group -- an empty one in front; windows, flags of the later clusters and record bytes are the tail of the
    full run every time.  With has_pulse 0 the first cluster opens no group whatever the time (no pulse yet)"""
    d, cfg0, dt, rext, dec = fixture(name)
    eng, cfg = engine(name, True, False)
    replay_chain_on_engine(eng, d, cfg, debug=False)
    full_rec = eng.records()
    full_groups = eng.groups()
    full_cl_group = eng.cluster_groups(len(dec))
    n_groups_full = eng.counts['n_groups']
    a_plus = [c for c in np.flatnonzero((d['dec_section'] == WE.SECTIONS.index('A')) & d['dec_has_delta'] & (d['dec_delta'] == 1))]
    others = [c for c in range(1, len(dec)) if dec[c]['flush'] and dec[c]['E'] is not None and dec[c]['end'] is not None][::9]
    splits = sorted(set(int(c) for c in a_plus + others))
    assert len(splits) >= 4
    for c in splits:
        x = dec[c]
        assert x['flush']                     # the reference digitised in front of it: no window spans the split
        tail = tail_of(d, x['first'], cfg)
        w0 = int(np.searchsorted(d['dg_first_pulse'], d['call_pulse_off'][x['first']]))
        want_rec = full_rec[full_groups['first_record'][full_cl_group[c]]:].tobytes()
        later = [y['flush'] for y in dec[c + 1:]]
        carries = [(1, x['E'], True)] + [(1, x['tmin'] - rext - delta, delta > 0) for delta in (-1, 0, 1)]
        carries += [(0, x['E'], False), (0, x['tmin'] - rext - 1, False), (0, 0, False)]
        for has, e, opens in carries:
            eng.set_window_carry(has, e)
            replay_chain_on_engine(eng, tail, cfg, debug=False)
            flags = cluster_flags(eng, len(dec) - c)
            assert flags.tolist() == [opens] + later, (c, has, e)
            g, keep = _nonempty_groups(eng)
            assert (g['right'][0] < g['left'][0]) == opens, (c, has, e)
            assert eng.counts['n_groups'] == n_groups_full - full_cl_group[c] + (1 if opens else 0), (c, has, e)
            assert np.array_equal(g['left'][keep], d['dg_left'][w0:]) and np.array_equal(g['right'][keep], d['dg_right'][w0:]), (c, has, e)
            assert eng.records().tobytes() == want_rec, (c, has, e)
    eng.set_window_carry(0, 0)


# ------------------------------------------------------------------------------------------------ more clusters than k_groups has threads
def layouts():
    """(total clusters, name, clusters without pulses in front, runs of them between the first copies) -- the copies of the 78-cluster
    stream fill up the total, the rest are clusters without pulses behind the last copy"""
    out = []
    for total in (1023, 1024, 1025, 2049, 3073):
        per = -(-total // GROUPS_TPB)
        out.append((total, 'plain', 0, ()))
        if total > GROUPS_TPB:
            out += [(total, f'prefix{p}', p, ()) for p in range(1, per)]
            out.append((total, 'runs', 0, (per, 2 * per + 1)))
    return out


def tiled(total, prefix, runs):
    """the nVeto fixture tiled to `total` clusters.  Every copy is shifted by a multiple of 2 x sample_duration and starts more than
    right_raw_extension + the longest pulse behind everything before it, clusters without pulses included, so the reference's verdicts
    inside a copy are those of the fixture (even landing included) and every cluster in front of a copy's first pulse -- its own
    pulse-less opening clusters, the filler clusters -- is more than right_raw_extension behind the last pulse end: a flush once a
    pulse exists, none before.  Returns (stream, shifts, expected flag per cluster)"""
    d, cfg, dt, rext, dec = fixture('nveto')
    n_c = len(dec)
    m = (total - prefix - sum(runs)) // n_c
    trailing = total - m * n_c - prefix - sum(runs)
    assert m >= 3 and trailing >= 0
    t = d['instructions']['time']
    t_first, t_last = int(t[0]), int(max(t[-1], d['pl_right'].max() * dt))
    longest = int((d['pl_right'] - d['pl_left'] + 1).max()) * dt
    gap = -(-(2 * rext + longest + 1000) // (2 * dt)) * (2 * dt)
    cursor, shifts, fillers = gap, [], []

    def fill(n):
        nonlocal cursor
        for _ in range(n):
            fillers.append(cursor)
            cursor += gap
    fill(prefix)
    for j in range(m):
        shift = -(-(cursor - t_first) // (2 * dt)) * (2 * dt)
        shifts.append(shift)
        cursor = shift + t_last + gap
        if j < len(runs):
            fill(runs[j])
    fill(trailing)
    s = WE.tile_stream(d, shifts, fillers, cfg)
    assert int(s['set_cluster'][-1]) + 1 == total
    # expected flags
    first_pulse = next(c for c, x in enumerate(dec) if x['end'] is not None)
    copy_of_cluster = s['copy_of_call'][np.concatenate([[0], np.flatnonzero(np.diff(s['set_cluster'])) + 1])]
    local = np.zeros(total, dtype=np.int64)
    seen = {}
    for k, j in enumerate(copy_of_cluster):
        if j >= 0:
            local[k] = seen.get(int(j), 0)
            seen[int(j)] = local[k] + 1
    expect, has = [], False
    for k, j in enumerate(copy_of_cluster):
        if j >= 0 and local[k] > first_pulse:
            expect.append(dec[local[k]]['flush'])
        else:
            expect.append(has)
        if j >= 0 and dec[local[k]]['end'] is not None:
            has = True
    return s, shifts, np.array(expect), m


@pytest.mark.parametrize('total,kind,prefix,runs', layouts(), ids=[f'{t}-{k}' for t, k, _, _ in layouts()])
def test_more_clusters_than_threads(total, kind, prefix, runs):
    """per = ceil(clusters / 1024) consecutive clusters per thread of k_groups.  The recorded photons through load_photons and the stored
    inputs through RawDataOptical, one batch each: the flag of every cluster is the reference's verdict, the non-empty windows of copy j
    are the fixture's shifted by shifts[j] / dt, the records are the oracle's bytes for the whole stream, and n_groups less the empty
    groups is copies x the fixture's windows"""
    d, cfg0, dt, rext, dec = fixture('nveto')
    s, shifts, expect, m = tiled(total, prefix, runs)
    per = -(-total // GROUPS_TPB)
    assert per == (1 if total <= GROUPS_TPB else {1025: 2, 2049: 3, 3073: 4}[total]) and len(shifts) == m
    want_left = np.concatenate([d['dg_left'] + sh // dt for sh in shifts])
    want_right = np.concatenate([d['dg_right'] + sh // dt for sh in shifts])
    # ---- the recorded photons and gains
    eng, cfg = engine('nveto', True, True)
    counts = replay_chain_on_engine(eng, s, cfg, debug=False)
    flags = cluster_flags(eng, total)
    wrong = np.flatnonzero(flags != expect)
    assert len(wrong) == 0, f'flags differ at clusters {wrong[:10].tolist()} (per {per}: positions {(wrong[:10] % per).tolist()} of a thread\'s range)'
    g, keep = _nonempty_groups(eng)
    assert np.array_equal(g['left'][keep], want_left) and np.array_equal(g['right'][keep], want_right)
    assert counts['n_groups'] - (g['right'] < g['left']).sum() == m * len(d['dg_left'])
    assert counts['n_groups'] == expect.sum() + 1
    orc = make_oracle(cfg)
    r = replay_chain_on_oracle(orc, s)
    assert np.array_equal(r['dg_left'], want_left) and np.array_equal(r['dg_right'], want_right)
    assert eng.records().tobytes() == orc.pack_records().tobytes()
    # ---- our own optical path
    ocfg = dict(cfg, seed=72)
    windows, rec, rd = run_optical(ocfg, s['instructions'], s['channels'], s['timings'])
    assert [w[0] for w in windows] == want_left.tolist() and [w[1] for w in windows] == want_right.tolist()
    assert rd.engine.counts['n_pulse_sets'] == len(s['instructions'])               # one batch
    assert np.array_equal(cluster_flags(rd.engine, total), expect)
    go = rd.engine.groups()
    assert rd.engine.counts['n_groups'] - (go['right'] < go['left']).sum() == m * len(d['dg_left'])
    o, orec = oracle_optical(ocfg, s['instructions'], s['channels'], s['timings'], int(d['cutoff']))
    assert np.array_equal(o['dg_left'], want_left) and np.array_equal(o['dg_right'], want_right)
    assert rec == orec


def test_instructions_that_share_photon_ranges():
    """RawDataOptical.sim_primary takes _first:_last as they come (rawdata.py:477): three shifted copies of the nVeto stream that all name
    the one stretch of the flat photon arrays, so the instructions' ranges add up to three times the arrays' length.  wfs_load_optical
    sized its bucketed photon copies by the arrays' length and k_optical_bucket wrote past them; they are sized by the sum of the ranges
    now.  Windows are the fixture's, shifted; records the oracle's bytes"""
    d, cfg0, dt, rext, dec = fixture('nveto')
    span = int(max(d['instructions']['time'][-1], d['pl_right'].max() * dt)) - int(d['instructions']['time'][0])
    period = -(-(span + 10 * rext) // (2 * dt)) * (2 * dt)
    shifts = [0, period, 2 * period]
    s = WE.tile_stream(d, shifts, [], cfg0, share_photons=True)
    ins = s['instructions']
    assert len(s['channels']) == len(d['channels']) and (ins['_last'] - ins['_first']).sum() == 3 * len(d['channels'])
    cfg = dict(cfg0, seed=73)
    windows, rec, rd = run_optical(cfg, ins, s['channels'], s['timings'])
    o, orec = oracle_optical(cfg, ins, s['channels'], s['timings'], int(d['cutoff']))
    assert [w[0] for w in windows] == np.concatenate([d['dg_left'] + sh // dt for sh in shifts]).tolist()
    assert [w[1] for w in windows] == np.concatenate([d['dg_right'] + sh // dt for sh in shifts]).tolist()
    assert rec == orec and len(rec) > 0
