"""Digitiser noise drawn per sample on the device (config 'noise_model', wfs_set_noise_model, noise kind 3 of the row kernels; MI355X only).

The definition is restated in numpy in tests/noise_model.py (test_noise_model_cpu.py checks the restatement on the CPU).  The device is
pinned against it twice: sample by sample through Engine.noise_samples, and end to end through the EXISTING table-noise path -- the
model's values for the rows of a run are written into an int16 table with one stretch per digitise window (materialise), and the oracle
and the engine replay that table from the stretch's start.  Records are compared byte for byte.
"""
import gc

import numpy as np
import pytest

from tests import noise_model as NM
from tests.helpers import ap_tables_from_golden, make_engine, make_oracle, with_fma
from tests.sum_signal import SUM_CHANNEL, assert_sum_rows, expected_sum_rows
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype, raw_record_dtype
from wfsim_amd.engine import WfsError, device_allocations
from wfsim_amd.noise_model import gaussian_pmf, noise_pmf
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule, run_sets

pytestmark = pytest.mark.gpu
MS = 1_000_000
T34 = 2 ** 34           # the sample index at which the quad index t >> 2 leaves 32 bits: 171.8 s of run time


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _sigmas(n, seed=3, quiet=(3,)):
    """per channel between 0 and half the ZLE threshold of 15 ADC counts, exact zeros on the channels of ``quiet``"""
    s = np.random.default_rng(seed).uniform(0.0, 7.5, n)
    s[list(quiet)] = 0.0
    return s


def _as_records(blob):
    return np.frombuffer(np.asarray(blob).tobytes(), dtype=raw_record_dtype())


def _bounds(rec):
    return sorted(zip(rec['channel'].tolist(), rec['time'].tolist(), rec['pulse_length'].tolist(), rec['record_i'].tolist()))


def _model_of(cfg):
    pmf, vmin = noise_pmf(cfg, 801)
    return pmf, vmin, int(kernel_params(cfg)['seed'])


def _table_config(cfg, table):
    c = {k: v for k, v in cfg.items() if k != 'noise_model'}
    return dict(c, enable_noise=True, noise_data=table)


def _off_config(cfg):
    return dict({k: v for k, v in cfg.items() if k not in ('noise_model', 'noise_data')}, enable_noise=False)


def _rows_with_sum(o, cfg, orc):
    """(window, channel, first absolute sample, length) of a noise-free oracle run, the sum rows included"""
    rows = NM.oracle_rows(o)
    if cfg.get('emit_sum_signal'):
        rows += [(e['window'], SUM_CHANNEL, e['left'], len(e['S'])) for e in expected_sum_rows(o, kernel_params(cfg), orc.tables['thr_zle'])]
    return rows


# ---------------------------------------------------------------------------------------------------- 1, 2: cells and samples
@pytest.fixture(scope='module')
def probe():
    sigma = np.full(801, 2.2)
    sigma[NM.STAT_CHANNELS[1]] = 0.7
    sigma[[7, 503]] = [0.0, 5.1]
    cfg = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20, enable_noise=True, noise_model={'sigma': sigma}, seed=NM.STAT_SEED), False)
    eng = make_engine(cfg)
    pmf, vmin = gaussian_pmf(sigma)
    return eng, cfg, pmf, vmin


@pytest.mark.parametrize('ch', [0, 250, 800])
def test_cells_encode_the_pmf(probe, ch):
    eng, cfg, pmf, vmin = probe
    c = eng.noise_model_cells(ch)
    K = len(c['thr'])
    assert K == 64 and c['shift'] == 26 and c['vmin'] == vmin == -31          # 63 values: half = ceil(6 * 5.1)
    mass = NM.cells_pmf(c['thr'], c['alias'], pmf.shape[1])
    assert np.all(np.abs(mass[:pmf.shape[1]] - pmf[ch]) <= K * 2.0 ** -32) and np.all(mass[pmf.shape[1]:] <= K * 2.0 ** -32)
    thr, alias, shift = NM.build_alias(pmf[ch])         # the transcription of the host's construction arrives at the same cells
    assert np.array_equal(thr, c['thr']) and np.array_equal(alias, c['alias']) and shift == c['shift']


@pytest.mark.parametrize('t0', [0, 1, 2, 3, -6, T34 - 5])
def test_probe_is_the_restatement(probe, t0):
    eng, cfg, pmf, vmin = probe
    p = kernel_params(cfg)
    n = 4099
    for ch in (0, 7, int(p['n_tpc']) - 1, int(p['he_first']) + 3, 800):
        c = eng.noise_model_cells(ch)
        exp = NM.noise_values((c['thr'], c['alias']), c['shift'], c['vmin'], NM.STAT_SEED, ch, t0 + np.arange(n, dtype=np.int64))
        got = eng.noise_samples(ch, t0, n)
        assert got.dtype == np.int16 and np.array_equal(got.astype(np.int64), exp), (ch, t0)
        if ch == 7:
            assert not got.any()                         # sigma 0
    assert len(eng.noise_samples(0, t0, 0)) == 0
    assert np.array_equal(eng.noise_samples(0, t0, 3), eng.noise_samples(0, t0, 4099)[:3])


def test_probe_statistics(probe):
    eng, cfg, pmf, vmin = probe
    a, b = NM.STAT_CHANNELS
    sa, sb = eng.noise_samples(a, NM.STAT_T0, NM.STAT_N), eng.noise_samples(b, NM.STAT_T0, NM.STAT_N)
    NM.assert_white(sa.astype(np.int64), sb.astype(np.int64), pmf[a], pmf[b], vmin)


# ---------------------------------------------------------------------------------------------------- 3: designed rows
def _photon_sets(windows, gains):
    """windows: list of (base time ns, [(channel, [photon times relative to the base], gain factor)]); one pulse set per entry, one
    cluster per window.  Returns the arguments of Engine.load_photons and the oracle's calls per window"""
    set_cluster, set_tmin, off, t, ch, gain, calls = [], [], [0], [], [], [], []
    for w, (base, entries) in enumerate(windows):
        calls.append([])
        for c, times, f in sorted(entries, key=lambda e: min(e[1])):
            tt = int(base) + np.sort(np.asarray(times, dtype=np.int64))
            calls[-1].append((len(set_cluster), tt, c, gains[c] * f))
            set_cluster.append(w); set_tmin.append(int(tt.min()))
            t += tt.tolist(); ch += [c] * len(tt); gain += [gains[c] * f] * len(tt); off.append(len(t))
    return (set_cluster, set_tmin, off, t, ch, gain, np.zeros(len(t), np.uint8)), calls


def _oracle_photons(cfg, calls, ix=None):
    orc = make_oracle(cfg)
    if ix is not None:
        orc.set_noise_override(ix)
    for window in calls:
        for k, tt, c, g in window:
            orc.pulse_call(1, k, tt, np.full(len(tt), c, np.int16), np.zeros(len(tt), np.uint8), np.full(len(tt), g), True)
        orc.digitize_and_zle(0)
    return orc


def _engine_photons(cfg, sets, ix=None, profiling=False):
    eng = make_engine(cfg)
    eng.set_debug(False)
    if profiling:
        eng.set_profiling(True)
    for attempt in range(2 if ix is not None else 1):
        eng.load_photons(*sets)
        eng.run()
        if ix is not None and attempt == 0:              # the noise start of every window, as tests/test_gpu_sum_signal.py injects them
            g = eng.groups()
            v = np.full(len(g['left']), -1, dtype=np.int64)
            v[g['right'] >= g['left']] = ix
            eng.set_noise_offsets(v)
    return eng


def _designed_windows(p):
    n_top, last, dt, tw = int(p['n_top']), int(p['last_bottom']), int(p['dt']), int(p['trigger_window'])
    per = int(p['store_before'] + p['samples_before'] + p['store_after'] + p['samples_after']) + 1 + 2 * tw      # row of one photon
    far = (2 * tw + 1 + per + 40) * dt
    assert per < 257
    w = []
    for k in range(4):          # the row's first sample takes every residue mod 4; lengths per + k: at most one a multiple of four
        w.append((10 * MS * (k + 1) + dt * k, [(3, [500, 500 + dt * k], 1.0), (n_top + 5 + k, [700 + dt * ((k + 1) % 4)], 1.0), (7 + k, [900, 900 + dt * (k + 2)], 2.0)]))
    w.append((50 * MS, [(n_top + 1, [400, 400 + dt * (257 - per)], 1.0), (11, [430], 1.0)]))                       # 4: 256 + 1 samples
    w.append((60 * MS + dt, [(n_top + 7, [100, 100 + dt * 1100, 100 + dt * 2300], 1.0), (12, [100 + dt * 3, 100 + dt * 2150], 1.0)]))      # 5: beyond 2 x 1024
    w.append((70 * MS, [(n_top + 2, [400, 400 + far, 400 + 2 * far], 1.0), (last, [400, 400 + far], 1.0), (13, [350], 30.0)]))      # 6: several intervals; a large pulse
    w.append((dt * (T34 - 60), [(14, [0, 1900], 1.0), (n_top + 9, [300], 1.0)]))                                   # 7: rows across t = 2^34
    w.append((dt * (T34 + 2_000_001), [(15, [0], 1.0), (n_top + 3, [dt, 3 * dt], 1.0), (3, [40], 1.0)]))           # 8: beyond it, a window of its own 20 ms on
    return w


@pytest.mark.parametrize('sum_signal', [False, True])
@pytest.mark.parametrize('channels', [494, 801])
@pytest.mark.parametrize('tw', [50, 20])
@pytest.mark.parametrize('resident', [0, 1])
def test_designed_rows(resident, tw, channels, sum_signal):
    # 494 channels: no HE rows (factor 0), so that rows can be resident; 801 with factor 20: HE rows and the sum row get noise
    base = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20 if channels == 801 else 0, trigger_window=tw, row_resident=resident,
                                       emit_sum_signal=sum_signal, seed=1234 + channels), False)
    cfg = dict(base, enable_noise=True, noise_model={'sigma': _sigmas(channels)})
    p = kernel_params(cfg)
    sets, calls = _photon_sets(_designed_windows(p), np.asarray(cfg['gains'], dtype=np.float64))
    off = _oracle_photons(_off_config(cfg), calls)
    o_off = off.results()
    rows = _rows_with_sum(o_off, cfg, off)
    first, length = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    assert set((first % 4).tolist()) == {0, 1, 2, 3} and len(set((length % 4).tolist())) == 4
    assert 257 in length and length.max() > 2048 and first.max() > T34 and np.any((first < T34) & (first + length > T34))
    assert channels != 801 or any(int(p['he_first']) <= r[1] < SUM_CHANNEL for r in rows)
    pmf, vmin, seed = _model_of(cfg)
    table, ix = NM.materialise(rows, len(o_off['dg_left']), pmf, vmin, seed)
    tab_cfg = _table_config(cfg, table)
    orc = _oracle_photons(tab_cfg, calls, ix)
    o = orc.results()
    eng = _engine_photons(cfg, sets, profiling=True)
    assert np.all(eng.groups()['ix_rand'][eng.groups()['right'] >= eng.groups()['left']] == 0)
    rec = eng.records()
    if sum_signal:
        exp = expected_sum_rows(o, kernel_params(tab_cfg), orc.tables['thr_zle'], noise=table, ix_rand=ix)
        assert len(exp) == len(calls)
        assert_sum_rows(eng, exp)
        assert (channels == 801) == any(not np.array_equal(e['finished'], np.maximum(e['S'] + int(p['baseline']), 0)) for e in exp)
    assert np.any(rec['channel'] == SUM_CHANNEL) == (sum_signal and channels == 801)        # (factor 0 and no noise column: a flat sum row)
    plain = rec[rec['channel'] != SUM_CHANNEL]
    assert plain.tobytes() == orc.pack_records().tobytes()
    kt = eng.kernel_times()
    res = resident == 1 and channels == 494 and tw == 50         # (HE rows and a hold-off below a chunk keep every row on the accumulators)
    assert ('k_row_pulse' in kt) == res and ('k_pack_res' in kt) == res, sorted(kt)
    # with the sum row on, bottom rows stay on the accumulators; without it every row of these windows is resident
    assert ('k_zle' in kt) == (not res or sum_signal) and ('k_pack' in kt) == (not res or sum_signal), sorted(kt)
    # more than one interval in a row, and the noise reaches the ZLE: some interval bound or count differs from the noise-free run
    assert max(np.bincount(o['zl_ch'][o['zl_digit'] == 6])) > 1
    quiet = _as_records(off.pack_records())
    assert _bounds(plain) != _bounds(quiet)
    ch3 = lambda r: r[r['channel'] == 3]
    assert ch3(plain).tobytes() == ch3(quiet).tobytes() and len(ch3(plain)) > 0        # the sigma = 0 channel
    # the engine on the materialised table, through the kernels of the int16 table
    eng_t = _engine_photons(tab_cfg, sets, ix)
    assert eng_t.records().tobytes() == rec.tobytes()


# ---------------------------------------------------------------------------------------------------- 4, 5: generated photons
def _instructions(rows):
    ins = np.zeros(len(rows), dtype=instruction_dtype)
    for k, r in enumerate(rows):
        for f, v in r.items():
            ins[k][f] = v
    ins['recoil'], ins['event_number'] = 7, np.arange(len(rows))
    return ins


def _generated(cfg, ins, ap=None):
    """engine with the model of cfg, oracle with the materialised table (geometry from a noise-free oracle run)"""
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    off_cfg = _off_config(cfg)
    off = make_oracle(off_cfg, ap)
    off.simulate(s_ins, gid, ip)
    o_off = off.results()
    pmf, vmin, seed = _model_of(cfg)
    table, ix = NM.materialise(_rows_with_sum(o_off, cfg, off), len(o_off['dg_left']), pmf, vmin, seed)
    orc = make_oracle(_table_config(cfg, table), ap)
    orc.set_noise_override(ix)
    orc.simulate(s_ins, gid, ip)
    eng = make_engine(cfg)
    eng.set_profiling(True)
    rs = None if cfg.get('save_full_truth', True) else run_sets(s_ins, key, cluster, cfg)[0]
    eng.load_instructions(s_ins, gid, cluster, key, ip, run_set=rs)
    eng.run()
    return eng, orc, off


EVERY_SOURCE = [dict(type=2, time=MS, x=2, y=1, z=-8, amp=2500),            # bright enough for single-tile rows of k_s2_tile
                dict(type=2, time=MS + 2000, x=2, y=1, z=-8, amp=15),       # overlaps it on about half of the channels: shared rows (k_tile_add)
                dict(type=1, time=4 * MS, x=0, y=0, z=-30, amp=60)]         # a small S1: rows that would be resident


@pytest.mark.parametrize('resident', [0, 1, 'auto'])
def test_every_row_source(resident):
    cfg = with_fma(xenonnt_test_config(seed=31, row_resident=resident, tile_local_min_photons=0, enable_noise=True,
                                       noise_model={'sigma': _sigmas(494, seed=8)}), False)
    eng, orc, off = _generated(cfg, _instructions(EVERY_SOURCE))
    rec = eng.records()
    assert len(rec) > 0 and rec.tobytes() == orc.pack_records().tobytes()
    assert _bounds(rec) != _bounds(_as_records(off.pack_records()))
    kt = eng.kernel_times()
    assert 'k_s2_tile' in kt and 'k_tile_add' in kt, sorted(kt)
    if resident != 'auto':
        assert ('k_row_pulse' in kt) == (resident == 1), sorted(kt)


def _random_case(seed):
    """a random mix as tests/test_gpu_sum_signal.py builds them, without HE rows and without the sum row, the model in place of noise_data"""
    rng = np.random.default_rng(seed)
    kw = dict(s2_secondary_sc_gain=float(rng.choice([1.5, 4.0, 21.3, 100.0])), seed=int(rng.integers(1, 10 ** 6)))
    kw['tile_local_min_photons'] = int(rng.choice([0, 0, 64]))
    if rng.random() < 0.4:
        kw['save_full_truth'] = False
    ap = ap_tables_from_golden() if rng.random() < 0.35 else None
    if ap is not None:
        kw.update(enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    kw.update(enable_noise=True, noise_model={'sigma': _sigmas(494, seed=seed, quiet=(int(rng.integers(0, 494)),))})
    u = rng.random()
    if u < 0.6:
        kw['row_resident'] = u < 0.3
    cfg = with_fma(xenonnt_test_config(**kw), False)
    n = int(rng.integers(3, 40))
    ins = np.zeros(n, dtype=instruction_dtype)
    ins['type'] = rng.choice([1, 2], n)
    ins['time'] = np.cumsum(rng.choice([200, 3_000, 40_000, 500_000, 3_000_000], n)).astype(np.int64) + 1_000_000
    ins['x'], ins['y'], ins['z'] = rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), -rng.uniform(0.5, 95, n)
    ins['amp'] = np.where(ins['type'] == 1, rng.choice([0, 1, 40, 700, 5000, 30000], n), rng.choice([0, 1, 7, 60, 400, 2500], n, p=[.1, .15, .2, .25, .2, .1]))
    ins['recoil'], ins['event_number'] = 7, np.arange(n)
    return cfg, ins, ap


@pytest.mark.parametrize('seed', range(10))
def test_random_mix(seed):
    cfg, ins, ap = _random_case(52000 + seed)
    eng, orc, off = _generated(cfg, ins, ap)
    assert eng.records().tobytes() == orc.pack_records().tobytes()


# ---------------------------------------------------------------------------------------------------- 6: switches
@pytest.fixture(scope='module')
def small():
    """three windows of supplied photons, the table they were run with before the feature existed, and a model"""
    base = with_fma(xenonnt_test_config(seed=99), False)
    p = kernel_params(base)
    sets, calls = _photon_sets(_designed_windows(p)[:3], np.asarray(base['gains'], dtype=np.float64))
    noise = np.random.default_rng(5).integers(-9, 10, size=(3000, 494)).astype(np.int16)
    model = {'sigma': _sigmas(494, seed=12)}
    return base, sets, calls, noise, model


def _profiled(cfg, sets):
    gc.collect()
    before = device_allocations()
    eng = make_engine(cfg)
    eng.set_debug(False)
    eng.set_profiling(True)
    eng.load_photons(*sets)
    eng.run()
    return eng, eng.records().tobytes(), sorted(eng.kernel_times()), device_allocations()[0] - before[0]


def test_without_a_model_nothing_changes(small):
    base, sets, calls, noise, model = small
    for cfg in (dict(base, enable_noise=False), dict(base, enable_noise=True, noise_data=noise)):
        absent, none = _profiled(cfg, sets), _profiled(dict(cfg, noise_model=None), sets)
        assert absent[0].noise_model is None and absent[1:] == none[1:]
        assert 'k_noise_model_samples' not in absent[2]
        with pytest.raises(WfsError, match='no noise model'):
            absent[0].noise_samples(0, 0, 4)
        with pytest.raises(WfsError, match='no noise model'):
            absent[0].noise_model_cells(0)
        if not cfg['enable_noise']:
            assert absent[1] == _oracle_photons(cfg, calls).pack_records().tobytes()
            with_model = _profiled(dict(cfg, enable_noise=True, noise_model=model), sets)
            assert with_model[3] == absent[3] + 1 and with_model[2] == absent[2]      # the cells: one buffer; the same kernels, of another kind
            assert with_model[1] != absent[1]


def test_enable_noise_off_and_precedence(small):
    base, sets, calls, noise, model = small
    quiet = _profiled(dict(base, enable_noise=False), sets)[1]
    assert _profiled(dict(base, enable_noise=False, noise_model=model), sets)[1] == quiet
    alone = _profiled(dict(base, enable_noise=True, noise_model=model), sets)
    both = _profiled(dict(base, enable_noise=True, noise_model=model, noise_data=noise), sets)
    assert both[1:] == alone[1:] and alone[1] != quiet
    assert both[0].tables['noise'] is None                  # not uploaded


def test_clearing_the_model_restores_the_table(small):
    base, sets, calls, noise, model = small
    cfg = dict(base, enable_noise=True, noise_data=noise)
    eng, table_rec = _profiled(cfg, sets)[:2]
    ix_table = eng.groups()['ix_rand'].copy()
    assert ix_table.max() > 0
    pmf, vmin = noise_pmf(dict(base, noise_model=model), 801)
    eng.set_noise_model(pmf, vmin)
    eng.load_photons(*sets); eng.run()
    model_rec = eng.records().tobytes()
    assert model_rec == _profiled(dict(base, enable_noise=True, noise_model=model), sets)[1] and model_rec != table_rec
    g = eng.groups()
    assert np.all(g['ix_rand'][g['right'] >= g['left']] == 0)
    eng.set_noise_offsets(np.full(len(g['left']), 17))      # accepted, without effect
    eng.load_photons(*sets); eng.run()
    assert eng.records().tobytes() == model_rec
    eng.set_noise_offsets([])
    eng.set_noise_model(None)
    eng.load_photons(*sets); eng.run()
    assert eng.records().tobytes() == table_rec and np.array_equal(eng.groups()['ix_rand'], ix_table)
    with pytest.raises(WfsError, match='no noise model'):
        eng.noise_samples(0, 0, 4)


@pytest.mark.parametrize('pmf,vmin,match', [
    (np.full((802, 2), 0.5), 0, 'n_channels'),
    (np.full((1, 4097), 1 / 4097), 0, 'n_values'),
    (np.zeros((1, 0)), 0, 'n_values'),
    ([[0.5, 0.5]], 32767, 'int16'),
    ([[0.5, 0.5]], -32769, 'int16'),
    ([[0.5, 0.6, -0.1]], 0, 'negative'),
    ([[0.5, 0.5], [0.5, 0.5 + 1e-8]], 0, 'does not sum to 1'),
])
def test_invalid_model_is_refused(small, pmf, vmin, match):
    eng = make_engine(small[0])
    with pytest.raises(WfsError, match=match):
        eng.set_noise_model(np.asarray(pmf, dtype=np.float64), vmin)
    with pytest.raises(WfsError, match='no noise model'):
        eng.noise_samples(0, 0, 1)
    eng.set_noise_model([[0.5, 0.5 + 1e-10]], -1)
    assert set(eng.noise_samples(0, 0, 64).tolist()) == {-1, 0}
    with pytest.raises(WfsError, match='channel'):
        eng.noise_samples(1, 0, 1)


# ---------------------------------------------------------------------------------------------------- 7: independence of the cut
def test_one_batch_or_two_and_the_seed(small):
    base, sets, calls, noise, model = small
    cfg = dict(base, enable_noise=True, noise_model=model)
    p = kernel_params(cfg)
    gains = np.asarray(cfg['gains'], dtype=np.float64)
    windows = _designed_windows(p)
    whole = _engine_photons(cfg, _photon_sets(windows, gains)[0]).records()
    eng = make_engine(cfg)
    eng.set_debug(False)
    parts = []
    for part in (windows[:4], windows[4:]):
        eng.load_photons(*_photon_sets(part, gains)[0])
        eng.run()
        parts.append(eng.records())
    assert len(parts[0]) and len(parts[1]) and np.concatenate(parts).tobytes() == whole.tobytes()
    other = _engine_photons(dict(cfg, seed=100), _photon_sets(windows, gains)[0]).records()
    assert other.tobytes() != whole.tobytes()


# ---------------------------------------------------------------------------------------------------- 8: lifetime
def test_close_returns_the_model(small):
    base, sets, calls, noise, model = small
    gc.collect()
    start = device_allocations()
    for cycle in range(2):
        eng = make_engine(dict(base, enable_noise=True, noise_model=model))
        eng.load_photons(*sets)
        assert eng.run()['n_records'] > 0 and len(eng.noise_samples(0, 0, 100)) == 100
        live = device_allocations()
        assert live[0] > start[0] and live[1] > start[1]
        eng.close()
        assert device_allocations() == start, cycle
    eng = make_engine(base)                                 # set, replaced, cleared by hand
    before = device_allocations()
    eng.set_noise_model(*gaussian_pmf([1.0, 2.0]))
    assert device_allocations()[0] == before[0] + 1
    eng.set_noise_model(*gaussian_pmf(np.full(801, 30.0)))
    assert device_allocations()[0] == before[0] + 1
    eng.set_noise_model(None)
    assert device_allocations() == before
    eng.close()
    assert device_allocations() == start


# ---------------------------------------------------------------------------------------------------- 9: through the plugin
def test_plugin_with_a_model_and_no_noise_data():
    import wfsim_amd
    from wfsim_amd import ministrax
    rows = []
    for i in range(2):
        rows += [dict(type=1, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=800), dict(type=2, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=120)]
    ins = _instructions(rows)
    ins['event_number'] = np.arange(len(ins)) // 2
    out = []
    for model in ({'sigma': 2.2}, {'sigma': 2.2}, None):
        cfg = xenonnt_test_config(seed=5, chunk_size=0.5, instructions=ins.copy(), enable_noise=model is not None, noise_model=model)
        assert 'noise_data' not in cfg
        chunks = ministrax.run_plugin(wfsim_amd.RawRecordsFromFaxNT(cfg))
        out.append(np.concatenate([c.data for c in chunks['raw_records']]))
    assert len(out[0]) > 0 and np.all(np.diff(out[0]['time']) >= 0)
    assert out[0].tobytes() == out[1].tobytes()             # reproducible under the seed
    assert out[0].tobytes() != out[2].tobytes()             # and not the noise-free records
