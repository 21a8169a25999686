"""PMT dark counts drawn on the device (config 'dark_count_rate', wfs_set_dark_counts; MI355X only).

The definition is restated in numpy in tests/dark_counts.py (tests/test_dark_counts_cpu.py checks the restatement's statistics).  The
device is pinned against it twice: sample by sample and photon by photon through Engine.dark_count_samples / dark_count_photons on
designed seams, and end to end through the UNCHANGED oracle -- the row terms of a run are written into a noise table with one stretch
per digitise window, on top of whatever noise the case has (tests/dark_counts.materialise), and the oracle replays that table from
forced ix_rand.  Records are compared byte for byte.  The designed cells below were found by scanning the restatement on the CPU at
the mu limit (seed 20261020, channel 5); every test asserts what it relies on with the restatement before it looks at the device.
"""
import numpy as np
import pytest

from tests import dark_counts as DK
from tests import full_readout as FR
from tests import noise_model as NM
from tests import noise_slow as NS
from tests import spe_channels as SC
from tests.helpers import make_engine, make_oracle, with_fma
from tests.sum_signal import SUM_CHANNEL
from tests.test_gpu_noise_slow import _model_of as _slow_model_of, _slow
from tests.test_gpu_noise_model import (MS, _as_records, _designed_windows, _engine_photons, _instructions, _model_of, _off_config,
                                        _oracle_photons, _photon_sets, _table_config)
from wfsim_amd import dark_counts as DC
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.engine import WfsError
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu
SEED = 20261020
CH = 5                          # the channel of the designed cells
NEAR_LIMIT = 0.96               # of the largest rate: mu = 0.12 photons per cell
# cells of channel CH at the mu limit under SEED, by their photon count; LAST_NS: a photon in the last ns of the cell
CELLS = {2: (315, 343, -1048454, 268435580), 3: (1465, 5483, -1046634, 268444343), 4: (1354, 170208, -971789, 268508629)}
LAST_NS = (15389, 17859, -1046337)


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _limit(dt=10):
    return DC.max_rate(dt)


# ---------------------------------------------------------------------------------------------------- 1: the two read-backs
@pytest.fixture(scope='module')
def probe():
    """per-channel SPE rows (the 'shaped' family of spe_channels.npz), non-uniform gains, DEAD_CH turned off; every channel at the mu
    limit but 6, which has rate 0 between two with a rate, and the channels from 300 on, which are beyond the given count"""
    cfg = with_fma(SC.config('shaped', seed=SEED), False)
    rates = np.full(300, _limit())
    rates[6] = 0.0
    eng = make_engine(dict(cfg, dark_count_rate=rates))
    assert eng.tables['spe'].shape[0] == 494
    return eng, DK.Dark.of_engine(eng)


def test_thresholds_on_the_device(probe):
    eng, dark = probe
    mine = DC.thresholds(eng.dark_count_rate, 494, 10)
    for ch in (0, 5, 6, 299):
        got = eng.dark_count_thresholds(ch)
        assert got.dtype == np.uint32 and np.all(np.abs(got.astype(np.int64) - mine[ch].astype(np.int64)) <= 1), (ch, got, mine[ch])
    assert not eng.dark_count_thresholds(6).any() and eng.dark_count_thresholds(5)[0] > eng.dark_count_thresholds(5)[3] > 0
    with pytest.raises(WfsError, match='channel outside the given rates'):
        eng.dark_count_thresholds(300)


def _assert_range(eng, dark, ch, t0, n):
    exp = dark.samples(ch, t0, n)
    got = eng.dark_count_samples(ch, t0, n)
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), exp), (ch, t0, n, np.flatnonzero(got != exp)[:8])
    et, eg = dark.photons_in(ch, t0, n)
    gt, gg = eng.dark_count_photons(ch, t0, n)
    assert np.array_equal(gt, et) and np.array_equal(gg, eg), (ch, t0, n)
    return exp, et


def test_designed_cells(probe):
    """cells with 2, 3 and 4 photons at positive, negative and large m, overlapping photons, seams at 64 m - 1 and 64 m; ranges that
    are and are not multiples of 256, at odd starts: the block form, its tail through the sample form, the sample form alone"""
    eng, dark = probe
    overlapping = 0
    for n_ph, cells in CELLS.items():
        for m in cells:
            assert dark.counts(CH, [m])[0] == n_ph, (m, n_ph)
            p = dark.photons(CH, m, m)
            overlapping += int(np.any(np.diff(np.sort(p['idx'])) < dark.tlen))
            for t0, n in ((64 * m - 301, 777), (64 * m - 256, 512), (64 * m - 1, 2), (64 * m, 1), (64 * m + 63, 3), (64 * m - 7, 259)):
                exp, et = _assert_range(eng, dark, CH, t0, n)
            assert len(dark.photons_in(CH, 64 * m, 64)[0]) == n_ph and np.any(dark.samples(CH, 64 * m - 2, 64 + dark.tlen) != 0)
    assert overlapping >= 6


def test_pulse_into_the_next_cell(probe):
    eng, dark = probe
    for m in LAST_NS:
        p = dark.photons(CH, m, m)
        k = int(np.argmax(p['t_ns']))
        assert p['t_ns'][k] == 64 * 10 * m + 639 and p['idx'][k] == 64 * m + 63 and p['r'][k] == 9
        exp, _ = _assert_range(eng, dark, CH, 64 * (m + 1), 64)           # the next cell alone: the tail of the pulse
        assert np.any(exp[:dark.tlen - dark.before - 1] != 0)
        _assert_range(eng, dark, CH, 64 * m + 61, 5)
        _assert_range(eng, dark, CH, 64 * m + 1, 255)


@pytest.mark.parametrize('t0', [0, -64 * 3000 - 1, 2 ** 40 + 77, -2 ** 40 - 13])
def test_long_ranges(probe, t0):
    """64 * 2000 samples and more: every remainder r < dt, the per-channel SPE rows, the high counter word, negative t"""
    eng, dark = probe
    n = 64 * 2000 + 3
    for ch in (CH, 8, 252, 253, 299, SC.ZERO_CH):
        exp, et = _assert_range(eng, dark, ch, t0, n)
        if ch != SC.ZERO_CH:
            assert set((et % 10).tolist()) == set(range(10)) and np.any(exp != 0)
        else:
            assert len(et) > 100 and not exp.any()          # an SPE row of zeros: photons of gain 0
    g = dark.photons_in(CH, t0, n)[1]                        # the gains name the channel's own SPE row, not a neighbour's
    assert np.all(np.isin(g, dark.gains[CH] * dark.spe_row(CH)[1:])) and not np.all(np.isin(g, dark.gains[CH] * dark.spe_row(8)[1:]))


def test_nothing_where_nothing_is_due(probe):
    eng, dark = probe
    for ch in (6, SC.DEAD_CH):                              # rate 0 between two channels with a rate; gain 0
        assert not eng.dark_count_samples(ch, -1000, 70000).any() and len(eng.dark_count_photons(ch, -1000, 70000)[0]) == 0
    assert eng.dark_count_samples(5, 64 * 315 - 3, 300).any() and eng.dark_count_samples(8, 0, 70000).any()
    assert len(eng.dark_count_samples(CH, 17, 0)) == 0 and len(eng.dark_count_photons(CH, 17, 0)[0]) == 0
    with pytest.raises(WfsError, match='channel outside the given rates'):
        eng.dark_count_samples(300, 0, 10)


def test_setter_errors_and_off(probe):
    eng = make_engine(with_fma(xenonnt_test_config(seed=3), False))
    with pytest.raises(WfsError, match='no dark-count rates are set'):
        eng.dark_count_samples(0, 0, 10)
    with pytest.raises(WfsError, match='no dark-count rates are set'):
        eng.dark_count_photons(0, 0, 10)
    with pytest.raises(WfsError, match='no dark-count rates are set'):
        eng.dark_count_thresholds(0)
    with pytest.raises(WfsError, match='wfs_set_dark_counts: n_channels outside 0 .. n_tpc'):
        eng.set_dark_counts(np.full(495, 100.0))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(WfsError, match='wfs_set_dark_counts: rate_hz of channel 2 is negative or not finite'):
            eng.set_dark_counts([100.0, 100.0, bad])
    with pytest.raises(WfsError, match='wfs_set_dark_counts: rate_hz of channel 1: more than 1/8 dark photons per cell'):
        eng.set_dark_counts([100.0, _limit() * 1.001])
    eng.set_dark_counts(np.full(494, _limit()))             # the limit itself is taken
    assert eng.dark_count_thresholds(493)[0] == DC.thresholds_of_mu(0.125)[0]
    eng.set_dark_counts(np.zeros(494))                      # all zero: off
    with pytest.raises(WfsError, match='no dark-count rates are set'):
        eng.dark_count_thresholds(0)
    eng.set_dark_counts(100.0)
    assert eng.dark_count_thresholds(493)[0] == DC.thresholds_of_mu(100.0 * 640e-9)[0]
    eng.set_dark_counts(None)
    assert eng.dark_count_rate is None
    with pytest.raises(ValueError, match='dark_count_rate'):
        make_engine(with_fma(xenonnt_test_config(seed=3, dark_count_rate=_limit() * 2), False))


# ---------------------------------------------------------------------------------------------------- 2: records against the oracle
TABLE_LEN = 3000


def _noise_of(kind, channels):
    """config keys of the noise of a case"""
    if kind == 0:
        return dict(enable_noise=False)
    if kind in (1, 2):
        noise = np.random.default_rng(5).integers(-9, 10, size=(TABLE_LEN, channels)).astype(np.float64 if kind == 2 else np.int16)
        if kind == 2:           # multiples of 1/8: table + D is exact in float64, the truncated sum is the device's
            noise = noise + np.random.default_rng(6).integers(-3, 4, size=noise.shape) / 8.0
        return dict(enable_noise=True, noise_data=noise)
    m = {'sigma': np.random.default_rng(3).uniform(0.0, 4.0, channels)}
    if kind == 5:
        m['slow'] = _slow(channels, (5, 9))
    return dict(enable_noise=True, noise_model=m)


def _quiet_intervals(off):
    """{channel: [(first absolute sample, length)]} of the records of a run without dark counts and without noise"""
    rec = _as_records(off.pack_records())
    out = {}
    for r in rec[rec['record_i'] == 0]:
        out.setdefault(int(r['channel']), []).append((int(r['time']) // int(r['dt']), int(r['pulse_length'])))
    return out


def _expected(cfg, rates, calls, dark_seed_engine, kind, starts=None):
    """(expected records, ix_rand of the oracle's table, rows, rows with a dark hit) of supplied-photon calls under cfg + rates"""
    p = kernel_params(cfg)
    off = _oracle_photons(_off_config(cfg), calls)
    o_off = off.results()
    rows, n_win = NM.oracle_rows(o_off), len(o_off['dg_left'])
    dark = DK.Dark.of_engine(dark_seed_engine)
    if kind == 0:
        base = None
    elif kind in (1, 2):
        base = DK.stretches_of_table(rows, n_win, np.asarray(cfg['noise_data']), starts)
    elif kind == 3:
        pmf, vmin, seed = _model_of(cfg)
        base = NM.materialise(rows, n_win, pmf, vmin, seed)[0]
    else:
        model, seed = _slow_model_of(cfg)
        base = NS.materialise_slow(rows, n_win, model, seed)[0]
    n_columns = max(801 if p['he_factor'] else p['n_tpc'], 0 if base is None else base.shape[1])
    table, ix = DK.materialise(rows, n_win, dark, p, n_columns, base)
    orc = _oracle_photons(_table_config(cfg, table), calls, ix)
    # (a threshold that stores whole rows: "where no instruction pulse is" is asked of the run at the ordinary threshold)
    quiet_run = off if cfg['zle_threshold'] == FR.ZLE_ADC else _oracle_photons(_off_config(dict(cfg, zle_threshold=FR.ZLE_ADC)), calls)
    hits = DK.dark_hits(dark, p, rows, FR.ZLE_ADC, _quiet_intervals(quiet_run))
    return orc.pack_records().tobytes(), rows, hits, _as_records(off.pack_records())


def _rates(n=494):
    r = np.full(n, NEAR_LIMIT * _limit())
    r[6] = 0.0
    return r


def _photon_case(kind, resident, channels=494, tw=50, full=False, n_windows=None, **kw):
    cfg = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20 if channels == 801 else 0, trigger_window=tw, row_resident=resident,
                                       seed=SEED, **kw), False)
    cfg = dict(cfg, **_noise_of(kind, channels))
    p = kernel_params(cfg)
    windows = (FR.windows_of(p) if full else _designed_windows(p))[:n_windows]
    if full:
        sets, calls, run_calls = FR.photon_input(cfg, p, windows)
    else:
        sets, calls = _photon_sets(windows, np.asarray(cfg['gains'], dtype=np.float64))
        run_calls = calls
    starts = np.random.default_rng(7).integers(0, TABLE_LEN, len(windows)) if kind in (1, 2) else None
    if starts is not None:
        starts[-1] = TABLE_LEN - 10                          # every row of the last window wraps
    on = dict(cfg, dark_count_rate=_rates(), full_readout=full)
    eng = _engine_photons(on, sets, starts, profiling=True)
    exp, rows, hits, quiet = _expected(cfg, _rates(), run_calls, eng, kind, starts)
    return dict(cfg=cfg, on=on, eng=eng, rec=eng.records(), exp=exp, rows=rows, hits=hits, quiet=quiet, sets=sets, starts=starts, p=p,
                windows=windows, calls=calls)


@pytest.mark.parametrize('kind', [0, 1, 2, 3, 5])
@pytest.mark.parametrize('resident', [0, 1])
def test_designed_rows_every_noise_kind(kind, resident):
    """accumulator rows (row_resident 0: k_zle / k_pack) and resident rows (1: k_row_pulse / k_pack_res) give the oracle's bytes, hence
    the same bytes, under every noise kind"""
    c = _photon_case(kind, resident)
    assert len(c['hits']) >= 3, len(c['hits'])
    assert c['rec'].tobytes() == c['exp'] and c['rec'].tobytes() != c['quiet'].tobytes()
    kt = c['eng'].kernel_times()
    assert ('k_row_pulse' in kt) == (resident == 1) and ('k_zle' in kt) == (resident == 0) and ('k_pack_res' in kt) == (resident == 1), sorted(kt)
    if kind == 0:           # a hit where no instruction made one: the channel's records are no longer those of the quiet run
        for w, ch, first, length in c['hits']:
            assert c['rec'][c['rec']['channel'] == ch].tobytes() != c['quiet'][c['quiet']['channel'] == ch].tobytes(), ch


def test_he_rows():
    """an HE slot gets its top channel's D times int(he_factor); HE rows keep every row on the accumulators"""
    c = _photon_case(3, 1, channels=801)
    he_hits = [r for r in c['hits'] if r[1] >= 500]
    assert len(he_hits) >= 3 and any(r[1] < 494 for r in c['hits'])
    assert c['rec'].tobytes() == c['exp']
    assert np.any(c['rec']['channel'] >= 500)


def test_short_hold_off_general_path():
    """trigger_window 20: a hold-off below a chunk, the general path of k_zle (load_sample per sample)"""
    c = _photon_case(1, 0, tw=20)
    assert len(c['hits']) >= 3 and c['rec'].tobytes() == c['exp']


@pytest.mark.parametrize('resident,channels,kind', [(1, 494, 3), (0, 801, 0), (1, 494, 1)])
def test_full_readout_rows_without_a_pulse(resident, channels, kind):
    c = _photon_case(kind, resident, channels=channels, full=True, n_windows=6)
    have = {(r[0], r[1]) for r in NM.oracle_rows(_oracle_photons(_off_config(c['cfg']), c['calls']).results())}
    empty_hits = [r for r in c['hits'] if (r[0], r[1]) not in have]
    assert len(empty_hits) >= 3 and 'k_row_empty' in c['eng'].kernel_times()
    assert c['rec'].tobytes() == c['exp']


def test_record_order_by_time():
    c = _photon_case(3, 1)
    eng = make_engine(c['on'])
    eng.set_record_order(True)
    eng.load_photons(*c['sets'])
    eng.run()
    rec = eng.records()
    exp = _as_records(np.frombuffer(c['exp'], dtype=np.uint8))
    assert len(c['hits']) >= 3 and len(rec) == len(exp)
    assert np.all(np.diff(rec['time']) >= 0)
    key = lambda r: np.lexsort((r['record_i'], r['channel'], r['time']))
    assert rec[key(rec)].tobytes() == exp[key(exp)].tobytes()


def test_whole_rows_are_compared():
    """zle_threshold below -2^15: every row is one interval, stored whole -- every sample of every row against the oracle"""
    c = _photon_case(3, 1, zle_threshold=-40000)
    # (the oracle makes HE rows whatever the HE factor, flat ones here, which this threshold stores; the engine has HE rows only when
    # they can differ from a flat baseline: the TPC rows are the comparison)
    exp = _as_records(np.frombuffer(c['exp'], dtype=np.uint8))
    assert len(c['hits']) >= 3 and c['rec'].tobytes() == exp[exp['channel'] < 494].tobytes()
    n_samples = int(c['rec']['length'][c['rec']['channel'] < 494].sum())
    assert n_samples == sum((r[3] - 1) // 2 * 2 + 1 for r in c['rows'] if r[1] < 494)          # every row whole, right down to an even sample


def test_batches_small_and_one():
    """the windows of one run, one per batch: the same records"""
    c = _photon_case(3, 1, n_windows=7)
    assert c['rec'].tobytes() == c['exp']
    gains = np.asarray(c['cfg']['gains'], dtype=np.float64)
    eng = make_engine(c['on'])
    parts = []
    for w in c['windows']:
        eng.load_photons(*_photon_sets([w], gains)[0])
        eng.run()
        parts.append(eng.records().tobytes())
    assert b''.join(parts) == c['rec'].tobytes()


# ---------------------------------------------------------------------------------------------------- 3: generated photons, tile rows
TILE_ROWS = [dict(type=2, time=MS, x=2, y=1, z=-8, amp=2500)]                       # rows of k_s2_tile's buffers (kind 1)
BRIGHT_ROWS = [dict(type=2, time=MS, x=0, y=0, z=-8, amp=20000)]                    # with s2_secondary_sc_gain 100 every tile is beyond 2048 photons: k_s2_bright (kind 3)


def _generated_case(rows_of_ins, resident='auto', sum_signal=False, rates=None, **kw):
    cfg = with_fma(xenonnt_test_config(seed=SEED + 1, row_resident=resident, tile_local_min_photons=0, enable_noise=False, emit_sum_signal=sum_signal, **kw), False)
    ins = _instructions(rows_of_ins)
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    eng = make_engine(dict(cfg, dark_count_rate=_rates() if rates is None else rates))
    eng.set_debug(False)
    eng.set_profiling(True)
    eng.load_instructions(s_ins, gid, cluster, key, ip)
    eng.run()
    return cfg, eng, (s_ins, gid, ip, cluster, key)


@pytest.mark.parametrize('source,tile_kind,kernel,gain', [(TILE_ROWS, 1, 'k_s2_tile', 21.3), (BRIGHT_ROWS, 3, 'k_s2_bright', 100.0)])
def test_tile_buffer_rows(source, tile_kind, kernel, gain):
    """one instruction in its window: every row is made by one tile and read from that tile's buffer in place"""
    cfg, eng, (s_ins, gid, ip, cluster, key) = _generated_case(source, s2_secondary_sc_gain=gain)
    p = kernel_params(cfg)
    off = make_oracle(_off_config(cfg))
    off.simulate(s_ins, gid, ip)
    o_off = off.results()
    rows, n_win = NM.oracle_rows(o_off), len(o_off['dg_left'])
    dark = DK.Dark.of_engine(eng)
    table, ix = DK.materialise(rows, n_win, dark, p, p['n_tpc'])
    orc = make_oracle(_table_config(cfg, table))
    orc.set_noise_override(ix)
    orc.simulate(s_ins, gid, ip)
    kinds = eng.tile_kernels()[0]
    assert kernel in eng.kernel_times(), sorted(eng.kernel_times())
    hits = [r for r in DK.dark_hits(dark, p, rows, FR.ZLE_ADC, _quiet_intervals(off)) if kinds[r[1]] == tile_kind]
    assert len(hits) >= 3, (len(hits), np.bincount(kinds.astype(np.int64)))
    assert eng.records().tobytes() == orc.pack_records().tobytes()


# ---------------------------------------------------------------------------------------------------- 4: what does not move
def test_sum_row_truth_and_groups_do_not_move():
    """the sum row, the truth, the windows (left, right, ix_rand of wfs_copy_groups) and the counts of rows, photons and samples are
    those of the run without dark counts.  wfs_copy_groups also hands out the index of a window's first RECORD, which counts the
    records in front of it: that one moves with the records dark pulses add, and must still cut the records window by window"""
    src = TILE_ROWS + [dict(type=1, time=4 * MS, x=0, y=0, z=-30, amp=60), dict(type=2, time=4 * MS + 30000, x=5, y=-3, z=-30, amp=40)]
    out = []
    for rates in (_rates(), np.zeros(494)):
        cfg, eng, _ = _generated_case(src, sum_signal=True, rates=rates, high_energy_deamplification_factor=20)      # (a factor of 0 makes the sum row flat)
        rec = eng.records()
        g = eng.groups()
        s = eng.sum_signal()
        first = g['first_record']
        assert first[0] == 0 and np.all(np.diff(first) > 0) and first[-1] < len(rec)
        cuts = np.append(first, len(rec))
        spans = [(int(rec['time'][a:b].min()), int(rec['time'][a:b].max())) for a, b in zip(cuts[:-1], cuts[1:])]
        assert all(x[1] < y[0] for x, y in zip(spans[:-1], spans[1:]))          # the records of a window, then those of the next
        out.append(dict(rec=rec, sum_rec=rec[rec['channel'] == SUM_CHANNEL].tobytes(), truth=b''.join(np.asarray(x).tobytes() for x in eng.truth()),
                        windows={k: np.asarray(g[k]).tobytes() for k in ('left', 'right', 'ix_rand')}, first=first,
                        sum={k: np.asarray(v).tobytes() for k, v in s.items()},
                        counts={k: eng.counts[k] for k in ('n_groups', 'n_rows', 'n_photons', 'n_raw_samples')}))
    on, off = out
    assert on['rec'].tobytes() != off['rec'].tobytes() and len(on['sum_rec']) > 0
    for k in ('sum_rec', 'truth', 'windows', 'sum', 'counts'):
        assert on[k] == off[k], k
    assert len(on['first']) == len(off['first']) and np.all(on['first'] >= off['first']) and len(on['rec']) > len(off['rec'])


def test_row_ranges_do_not_move():
    """the rows before zero suppression (debug copy): the same rows over the same ranges with and without dark counts, and what the
    finished samples differ by is the row term of the restatement"""
    cfg = with_fma(xenonnt_test_config(seed=SEED, enable_noise=False, emit_sum_signal=True), False)
    p = kernel_params(cfg)
    sets, calls = _photon_sets(_designed_windows(p)[:7], np.asarray(cfg['gains'], dtype=np.float64))
    got = []
    for rates in (_rates(), None):
        eng = make_engine(cfg if rates is None else dict(cfg, dark_count_rate=rates))
        eng.set_debug(True)                                 # (finished rows are kept)
        eng.load_photons(*sets)
        eng.run()
        got.append((eng, eng.rows(), eng.groups()))
    (eng, on, g_on), (_, off, g_off) = got

    def by_row(r):
        """{(window, channel): (left, right, finished samples)}: the library lists the rows in the order its row list was filled in,
        which is not the same from run to run"""
        out = {}
        for k in range(len(r['channel'])):
            n, a = int(r['right'][k] - r['left'][k] + 1), int(r['data_off'][k])
            out[(int(r['group'][k]), int(r['channel'][k]))] = (int(r['left'][k]), int(r['right'][k]), r['data'][a:a + n].astype(np.int64))
        assert len(out) == len(r['channel'])
        return out

    on, off = by_row(on), by_row(off)
    assert sorted(on) == sorted(off) and len(on) > 20 and any(ch == SUM_CHANNEL for _, ch in on)
    assert all(on[k][:2] == off[k][:2] for k in on)        # the same rows over the same ranges
    assert all(np.array_equal(g_on[k], g_off[k]) for k in ('left', 'right', 'ix_rand'))
    dark = DK.Dark.of_engine(eng)
    moved = 0
    for (group, ch), (left, right, data) in on.items():
        diff = data - off[(group, ch)][2]
        first = int(g_on['left'][group]) + left                                   # (row ranges are relative to their window)
        assert np.array_equal(diff, DK.row_term(dark, p, ch, first, right - left + 1)), (group, ch)
        moved += int(diff.any())
    assert moved >= 3


def test_off_in_three_spellings():
    """rates all zero, no rates (n_channels 0) and never calling the setter: the same bytes from the same kernels"""
    cfg = with_fma(xenonnt_test_config(seed=SEED, enable_noise=True, noise_model={'sigma': 2.0}), False)
    p = kernel_params(cfg)
    sets, calls = _photon_sets(_designed_windows(p)[:4], np.asarray(cfg['gains'], dtype=np.float64))
    expected = _engine_photons(cfg, sets, profiling=True)
    ref, kernels = expected.records().tobytes(), sorted(expected.kernel_times())
    for spelling in ('zeros', 'none', 'set then cleared'):
        eng = make_engine(dict(cfg, dark_count_rate=np.zeros(494)) if spelling == 'zeros' else cfg)
        if spelling == 'none':
            eng.set_dark_counts(None)
        if spelling == 'set then cleared':
            eng.set_dark_counts(_rates())
            eng.set_dark_counts(np.zeros(3))
        eng.set_profiling(True)
        eng.load_photons(*sets)
        eng.run()
        assert eng.records().tobytes() == ref and sorted(eng.kernel_times()) == kernels, spelling
        assert eng.dark_count_rate is None
