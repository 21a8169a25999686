"""The bottom-array sum channel on the GPU (config 'emit_sum_signal', wfs_set_sum_signal, k_sum_signal; MI355X only).

The expectation is the numpy restatement of tests/sum_signal.py on the oracle's pulses (test_sum_signal_cpu.py pins it on the
reference's own row 800).  In every case: the unfinished rows S and their ranges (Engine.sum_signal()), the records of channel 800
(finished samples, intervals, fragments) and -- the existing guarantee the feature leans on -- the records of every other channel
byte for byte those of the oracle, in the reference's order with the sum row behind the window's TPC and HE rows.
"""
import numpy as np
import pytest

from tests.helpers import (golden, make_engine, make_oracle, replay_chain_on_engine, replay_chain_on_oracle, with_fma,
                           geometry_chain_config, ap_tables_from_golden)
from tests.sum_signal import SUM_CHANNEL, assert_sum_rows, expected_sum_rows, expected_sum_records, record_tuples
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype
from wfsim_amd.engine import WfsError
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule, run_sets

pytestmark = pytest.mark.gpu
MS = 1_000_000
SUM_CHUNK = 1024        # samples of a sum row per workgroup of k_sum_signal (wfs_kernels.h)


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _he(**kw):
    return with_fma(xenonnt_test_config(high_energy_deamplification_factor=20, **kw), False)


def _records_off_sum(rec):
    return rec[rec['channel'] != SUM_CHANNEL]


def _assert_reference_order(rec, o, dt):
    """(window, channel, interval, fragment): windows in time order, channels ascending inside a window -- the sum row last"""
    w = np.searchsorted(o['dg_left'] * dt, rec['time'], side='right') - 1
    assert np.all(rec['time'] <= o['dg_right'][w] * dt)
    key = w.astype(np.int64) * 4096 + rec['channel']
    assert np.all(np.diff(key) >= 0)


def _assert_all(eng, orc, cfg, ix_rand=None, noise=None):
    o = orc.results()
    p = kernel_params(cfg)
    exp = expected_sum_rows(o, p, orc.tables['thr_zle'], noise=noise, ix_rand=ix_rand)
    rec = assert_sum_rows(eng, exp)
    assert _records_off_sum(rec).tobytes() == orc.pack_records().tobytes()
    _assert_reference_order(rec, o, int(p['dt']))
    c = eng.counts
    assert c['n_records'] == len(rec) and c['n_intervals'] == len(o['zl_ch']) + sum(len(e['intervals']) for e in exp)
    return exp, rec


# ---------------------------------------------------------------------------------------------------- 4: the reference's chain
@pytest.fixture(scope='module')
def chain_he():
    cfg = _he()
    d = golden('chain_he.npz')
    orc = make_oracle(cfg)
    replay_chain_on_oracle(orc, d)
    eng_off = make_engine(cfg)
    replay_chain_on_engine(eng_off, d, cfg)
    return cfg, d, orc, eng_off.records().copy(), dict(eng_off.counts)


def test_chain_he_sum_rows(chain_he):
    cfg, d, orc, rec_off, counts_off = chain_he
    on = dict(cfg, emit_sum_signal=True)
    eng = make_engine(on)
    assert eng.emits_sum_records
    replay_chain_on_engine(eng, d, on)                     # (debug on: finished rows are kept)
    exp, rec = _assert_all(eng, orc, on)
    assert [int(e['S'].min()) for e in exp] == d['dg_sum_min'].tolist()
    assert [int(e['S'].sum()) for e in exp] == d['dg_sum_total'].tolist()
    assert _records_off_sum(rec).tobytes() == rec_off.tobytes()
    assert len(rec) > len(rec_off)
    # finished rows and intervals of channel 800
    g = eng.groups()
    keep = np.where(g['right'] >= g['left'])[0]
    r = eng.rows()
    rows = sorted((int(np.searchsorted(keep, r['group'][k])), int(r['left'][k]), int(r['right'][k]),
                   r['data'][r['data_off'][k]:r['data_off'][k] + r['right'][k] - r['left'][k] + 1].astype(np.int64).tobytes())
                  for k in np.where(r['channel'] == SUM_CHANNEL)[0])
    assert rows == [(e['window'], e['left'] - int(d['dg_left'][e['window']]), e['right'] - int(d['dg_left'][e['window']]), e['finished'].tobytes()) for e in exp]
    z = eng.intervals()
    sel = z['channel'] == SUM_CHANNEL
    assert list(zip(z['left'][sel].tolist(), z['right'][sel].tolist())) == [i for e in exp for i in e['intervals']]
    c = eng.counts
    assert c['n_rows'] == counts_off['n_rows'] + len(exp)
    assert c['n_raw_samples'] == counts_off['n_raw_samples'] + sum(len(e['S']) for e in exp)


def test_switch_off_changes_nothing(chain_he):
    cfg, d, orc, rec_off, counts_off = chain_he
    assert not np.any(rec_off['channel'] == SUM_CHANNEL) and rec_off.tobytes() == orc.pack_records().tobytes()
    o = orc.results()
    # the counts of the parent commit on this chain: rows, samples and intervals of the oracle's masked rows, nothing else
    # (an HE row is its top row's accumulators times the factor: it counts as a row and adds no samples)
    tpc = np.repeat(o['row_ch'] < kernel_params(cfg)['n_tpc'], np.diff(o['row_data_off']))
    assert counts_off['n_rows'] == len(o['row_ch']) and counts_off['n_raw_samples'] == int(tpc.sum())
    assert counts_off['n_intervals'] == len(o['zl_ch']) and counts_off['n_groups'] >= len(o['dg_left'])
    eng = make_engine(dict(cfg, emit_sum_signal=False))
    assert not eng.emits_sum_records
    eng.set_profiling(True)
    replay_chain_on_engine(eng, d, cfg, debug=False)
    assert 'k_sum_signal' not in eng.kernel_times()
    assert len(eng.sum_signal()['group']) == 0 and eng.records().tobytes() == rec_off.tobytes()


def test_record_order_by_time(chain_he):
    cfg, d, orc, rec_off, counts_off = chain_he
    on = dict(cfg, emit_sum_signal=True)
    a, b = make_engine(on), make_engine(on)
    replay_chain_on_engine(a, d, on, debug=False)
    b.set_record_order(True)
    replay_chain_on_engine(b, d, on, debug=False)
    ra, rb = a.records(), b.records()
    assert np.any(rb['channel'] == SUM_CHANNEL)
    assert rb.tobytes() == ra[np.lexsort((ra['channel'], ra['time']))].tobytes()


def test_other_detector_and_invalid_channel(chain_he):
    cfg, d, orc, rec_off, counts_off = chain_he
    # XENON1T: the switch is accepted, no row (rawdata.py:241)
    c1 = dict(cfg, detector='XENON1T', emit_sum_signal=True)
    eng = make_engine(c1)
    assert not eng.emits_sum_records
    replay_chain_on_engine(eng, d, c1, debug=False)
    rec = eng.records()
    assert len(rec) and not np.any(rec['channel'] == SUM_CHANNEL) and len(eng.sum_signal()['group']) == 0
    # sum_signal inside the TPC range / the HE range: refused when the switch goes on, fine with it off
    for ch in (100, 600):
        cm = dict(cfg['channel_map'], sum_signal=ch)
        make_engine(dict(cfg, channel_map=cm))
        with pytest.raises(WfsError, match='sum_channel'):
            make_engine(dict(cfg, channel_map=cm, emit_sum_signal=True))


# ---------------------------------------------------------------------------------------------------- 5: designed photon lists
def _run_designed(cfg, windows, noise=None):
    """windows: list of lists of (channel, [photon times ns], gain factor); one pulse set per (window, entry), one cluster per window,
    10 ms apart.  Explicit gains.  Returns (engine, oracle, ix_rand)"""
    cfg = dict(cfg, emit_sum_signal=True)
    gains = np.asarray(cfg['gains'], dtype=np.float64)
    orc, eng = make_oracle(cfg), make_engine(cfg)
    set_cluster, set_tmin, off, t, ch, gain = [], [], [0], [], [], []
    ix = [(7 + 1001 * w) % 2500 for w in range(len(windows))]
    if noise is not None:
        orc.set_noise_override(ix)
    for w, entries in enumerate(windows):
        base = 10 * MS * (w + 1)
        for c, times, f in sorted(entries, key=lambda e: min(e[1])):
            tt = base + np.sort(np.asarray(times, dtype=np.int64))
            orc.pulse_call(1, len(set_cluster), tt, np.full(len(tt), c, np.int16), np.zeros(len(tt), np.uint8), np.full(len(tt), gains[c] * f), True)
            set_cluster.append(w); set_tmin.append(int(tt.min()))
            t += tt.tolist(); ch += [c] * len(tt); gain += [gains[c] * f] * len(tt); off.append(len(t))
        orc.digitize_and_zle(0)
    eng.set_debug(False)
    for attempt in range(2 if noise is not None else 1):
        eng.load_photons(set_cluster, set_tmin, off, t, ch, gain, np.zeros(len(t), np.uint8))
        eng.run()
        if noise is not None and attempt == 0:       # the noise start of every window, as test_gpu_parity.py injects the reference's
            g = eng.groups()
            v = np.full(len(g['left']), -1, dtype=np.int64)
            v[g['right'] >= g['left']] = ix
            eng.set_noise_offsets(v)
    return eng, orc, ix


def _designed_windows(p):
    n_top, last = int(p['n_top']), int(p['last_bottom'])
    dt = int(p['dt'])
    per = int(p['store_before'] + p['samples_before'] + p['store_after'] + p['samples_after']) + 1 + 2 * int(p['trigger_window'])
    far = (2 * int(p['trigger_window']) + 1 + per + 40) * dt            # pulses further apart than the ZLE hold-off
    # the row's first sample is start bin - store_before - samples_before - trigger_window: odd (the windows start 10 ms apart, on even samples)
    odd = dt * (1000 + (int(p['store_before'] + p['samples_before'] + p['trigger_window']) + 1) % 2)
    return [
        [(3, [500, 520], 1.0), (n_top - 1, [900], 1.0)],                                               # 0 top channels only: no row
        [(n_top + 5, [700], 1.0)],                                                                     # 1 one bottom pulse
        [(n_top + 1, [400, 430], 1.0), (last - 3, [400 + far], 1.0)],                                   # 2 two disjoint pulses: two intervals
        [(n_top - 1, [300], 1.0), (n_top, [350], 1.0), (last, [390, 2000], 1.0)],                       # 3 the edges of the bottom range
        [(n_top + 2, [100], 1.0), (n_top + 9, [100 + dt * (SUM_CHUNK + 1 - per)], 1.0)],                # 4 one chunk plus one sample
        [(n_top + 7, [100, 100 + dt * 2500], 1.0), (n_top + 8, [100 + dt * 1300], 1.0), (2, [50], 1.0)],      # 5 three chunks
        [(n_top + 4, [odd], 1.0), (5, [odd - 3000], 1.0)],                                              # 6 the row starts on an odd sample
        [(n_top + 3, [600 + k for k in range(40)], 60.0), (n_top + 6, [640], 1.0)],                     # 7 clamps to 0
    ]


@pytest.fixture(scope='module', params=['bundled', 'geometry'])
def designed(request):
    cfg = _he() if request.param == 'bundled' else with_fma(dict(geometry_chain_config(), high_energy_deamplification_factor=20), False)
    p = kernel_params(cfg)
    windows = _designed_windows(p)
    eng, orc, _ = _run_designed(cfg, windows)
    return cfg, p, windows, eng, orc


def test_designed_rows(designed):
    cfg, p, windows, eng, orc = designed
    exp, rec = _assert_all(eng, orc, dict(cfg, emit_sum_signal=True))
    tw, dt = int(p['trigger_window']), int(p['dt'])
    by_w = {e['window']: e for e in exp}
    assert sorted(by_w) == [1, 2, 3, 4, 5, 6, 7]                                   # window 0 holds top pulses only
    o = orc.results()
    assert len(by_w[2]['intervals']) == 2 and len(by_w[1]['intervals']) == 1
    # window 3: only the pulses on n_top and last_bottom count
    e = by_w[3]
    first = int(o['dg_first_pulse'][3])
    lefts = {int(o['pl_ch'][first + k]): int(o['pl_left'][first + k]) for k in range(int(o['dg_n_pulses'][3]))}
    assert e['left'] == min(lefts[int(p['n_top'])], lefts[int(p['last_bottom'])]) - tw and lefts[int(p['n_top']) - 1] - tw < e['left']
    assert len(by_w[4]['S']) == SUM_CHUNK + 1 and len(by_w[5]['S']) > 2 * SUM_CHUNK
    assert (by_w[6]['left'] - int(o['dg_left'][6])) % 2 == 1
    assert np.sum(by_w[7]['finished'] == 0) > 5 and all(np.all(by_w[w]['finished'] > 0) for w in (1, 2, 3, 4, 5, 6))


def test_designed_special_threshold():
    base = _he()
    p = kernel_params(base)
    n_top = int(p['n_top'])
    windows = [[(n_top + 1, [400], 1.0), (n_top + 30, [400 + 4000], 12.0)]]
    eng0, orc0, _ = _run_designed(base, windows)
    cfg = dict(base, special_thresholds={str(SUM_CHANNEL): 4000})
    eng1, orc1, _ = _run_designed(cfg, windows)
    e0, _ = _assert_all(eng0, orc0, dict(base, emit_sum_signal=True))
    e1, _ = _assert_all(eng1, orc1, dict(cfg, emit_sum_signal=True))
    assert len(e0[0]['intervals']) == 2 and len(e1[0]['intervals']) == 1      # the small pulse stays above the special threshold


@pytest.mark.parametrize('columns', [801, 494])
def test_designed_noise(columns):
    rng = np.random.default_rng(columns)
    noise = rng.integers(-12, 13, size=(3000, columns)).astype(np.int16)
    cfg = _he(enable_noise=True, noise_data=noise)
    p = kernel_params(cfg)
    eng, orc, ix = _run_designed(cfg, _designed_windows(p)[1:4], noise=noise)
    exp, rec = _assert_all(eng, orc, dict(cfg, emit_sum_signal=True), ix_rand=ix, noise=noise)
    quiet = [e for e in expected_sum_rows(orc.results(), p, orc.tables['thr_zle'])]
    same = all(np.array_equal(a['finished'], b['finished']) for a, b in zip(exp, quiet))
    assert same == (columns <= SUM_CHANNEL)                  # column 800 is used when the array has it, nothing otherwise


# ---------------------------------------------------------------------------------------------------- 6, 7: generated photons
def _run_generated(cfg, ins, ap=None, profiling=False):
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    orc = make_oracle(cfg, ap)
    orc.simulate(s_ins, gid, ip)
    eng = make_engine(cfg)
    if profiling:
        eng.set_profiling(True)
    rs = None if cfg.get('save_full_truth', True) else run_sets(s_ins, key, cluster, cfg)[0]
    eng.load_instructions(s_ins, gid, cluster, key, ip, run_set=rs)
    eng.run()
    return eng, orc


def _instructions(rows):
    ins = np.zeros(len(rows), dtype=instruction_dtype)
    for k, r in enumerate(rows):
        for f, v in r.items():
            ins[k][f] = v
    ins['recoil'], ins['event_number'] = 7, np.arange(len(rows))
    return ins


EVERY_SOURCE = [dict(type=2, time=MS, x=2, y=1, z=-8, amp=2500),            # bright enough for single-tile rows of k_s2_tile
                dict(type=2, time=MS + 2000, x=2, y=1, z=-8, amp=15),       # overlaps it on about half of the channels: shared rows (k_tile_add)
                dict(type=1, time=4 * MS, x=0, y=0, z=-30, amp=60)]         # a small S1: rows that would be resident


# (factor 0: no HE rows, so that resident rows exist next to the sum row -- S is then all zeros, its range still the union)
@pytest.mark.parametrize('resident,bright,he_factor', [(r, b, 20) for r in (0, 1, 'auto') for b in (True, False)] + [(1, True, 0), (1, False, 0)])
def test_every_row_source_feeds_the_sum(resident, bright, he_factor):
    cfg = with_fma(xenonnt_test_config(high_energy_deamplification_factor=he_factor, emit_sum_signal=True, seed=31, row_resident=resident,
                                       tile_local_bright=bright, tile_local_min_photons=0), False)
    eng, orc = _run_generated(cfg, _instructions(EVERY_SOURCE), profiling=True)
    exp, rec = _assert_all(eng, orc, cfg)
    kt = eng.kernel_times()
    assert kt['k_sum_signal'][1] == 1 and 'k_tile_add' in kt and 'k_s2_tile' in kt, sorted(kt)
    assert ('k_row_pulse' in kt) == (he_factor == 0), sorted(kt)
    assert len(exp) == 2


def _random_case(seed):
    """a random mix as tests/test_gpu_random_mixes.py builds them, with HE rows and the sum row on"""
    rng = np.random.default_rng(seed)
    kw = dict(s2_secondary_sc_gain=float(rng.choice([1.5, 4.0, 21.3, 100.0])), seed=int(rng.integers(1, 10 ** 6)),
              high_energy_deamplification_factor=20, emit_sum_signal=True)
    kw['tile_local_min_photons'] = int(rng.choice([0, 0, 64]))
    if rng.random() < 0.4:
        kw['save_full_truth'] = False
    ap = ap_tables_from_golden() if rng.random() < 0.35 else None
    if ap is not None:
        kw.update(enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    noise = None
    if rng.random() < 0.5:
        noise = golden('noise.npz')['noise']
        if rng.random() < 0.5:          # with a column for the sum channel
            noise = np.concatenate([noise, rng.integers(-9, 10, size=(len(noise), 801 - noise.shape[1])).astype(np.int16)], axis=1)
        kw.update(enable_noise=True, noise_data=noise)
    u = rng.random()
    if u < 0.5:
        kw['row_resident'] = u < 0.25
    cfg = with_fma(xenonnt_test_config(**kw), False)
    n = int(rng.integers(3, 40))
    ins = np.zeros(n, dtype=instruction_dtype)
    ins['type'] = rng.choice([1, 2], n)
    ins['time'] = np.cumsum(rng.choice([200, 3_000, 40_000, 500_000, 3_000_000], n)).astype(np.int64) + 1_000_000
    ins['x'], ins['y'], ins['z'] = rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), -rng.uniform(0.5, 95, n)
    ins['amp'] = np.where(ins['type'] == 1, rng.choice([0, 1, 40, 700, 5000, 30000], n), rng.choice([0, 1, 7, 60, 400, 2500], n, p=[.1, .15, .2, .25, .2, .1]))
    ins['recoil'], ins['event_number'] = 7, np.arange(n)
    return cfg, ins, ap, noise


@pytest.mark.parametrize('seed', range(10))
def test_random_mix(seed):
    cfg, ins, ap, noise = _random_case(41000 + seed)
    eng, orc = _run_generated(cfg, ins, ap)
    _assert_all(eng, orc, cfg, noise=noise)


# ---------------------------------------------------------------------------------------------------- 9: through the plugin
def test_plugin_fills_raw_records_aqmon():
    import wfsim_amd
    from wfsim_amd import ministrax
    rows = []
    for i in range(2):
        rows += [dict(type=1, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=800), dict(type=2, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=120)]
    ins = _instructions(rows)
    ins['event_number'] = np.arange(len(ins)) // 2
    out = {}
    for on in (False, True):
        cfg = xenonnt_test_config(seed=5, chunk_size=0.5, high_energy_deamplification_factor=20, emit_sum_signal=on, instructions=ins.copy())
        chunks = ministrax.run_plugin(wfsim_amd.RawRecordsFromFaxNT(cfg))
        out[on] = {k: np.concatenate([c.data for c in chunks[k]]) for k in ('raw_records', 'raw_records_he', 'raw_records_aqmon')}
    aq = out[True]['raw_records_aqmon']
    assert len(aq) > 0 and np.all(aq['channel'] == SUM_CHANNEL) and np.all(np.diff(aq['time']) >= 0)
    assert len(out[False]['raw_records_aqmon']) == 0
    for k in ('raw_records', 'raw_records_he'):
        assert len(out[True][k]) > 0 and out[True][k].tobytes() == out[False][k].tobytes(), k
        assert not np.any(out[True][k]['channel'] == SUM_CHANNEL)
