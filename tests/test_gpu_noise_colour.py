"""Coloured and common-mode digitiser noise drawn on the device (config 'noise_model' with 'taps' / 'common', wfs_set_noise_colour, noise
kind 4 of the row kernels; MI355X only).

The definition is restated in numpy in tests/noise_colour.py (test_noise_colour_cpu.py holds its statistics on the CPU).  The device is
pinned against it as the white model is: sample by sample through Engine.noise_samples / noise_white_samples -- exact integers, so
``==`` -- and end to end through the table-noise path: the model's values for the rows of a run are written into an int16 table with
one stretch per digitise window, and oracle and engine replay that table.  Records are compared byte for byte.
"""
import gc

import numpy as np
import pytest

from tests import noise_colour as NC
from tests import noise_model as NM
from tests.helpers import make_engine, make_oracle, with_fma
from tests.sum_signal import SUM_CHANNEL, assert_sum_rows, expected_sum_rows
from tests.test_gpu_noise_model import (EVERY_SOURCE, MS, T34, _as_records, _bounds, _designed_windows, _engine_photons, _instructions,
                                        _off_config, _oracle_photons, _photon_sets, _profiled, _random_case, _rows_with_sum, _sigmas,
                                        _table_config)
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.engine import WfsError, device_allocations
from wfsim_amd.noise_model import gaussian_pmf, noise_colour, noise_pmf
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule, run_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _model_of(cfg):
    pmf, vmin = noise_pmf(cfg, 801)
    return NC.colour_model(pmf, vmin, noise_colour(cfg, 801)), int(kernel_params(cfg)['seed'])


def _boards(n, quiet=(3,)):
    """two groups: boards of eight channels alternate; the quiet channels and every 37th have none"""
    g = (np.arange(n) // 8) % 2
    g[::37] = -1
    g[list(quiet)] = -1
    if n > SUM_CHANNEL:
        g[SUM_CHANNEL] = 0
    return g


def _colour(n, L, seed=1, quiet=(3,)):
    """the 'taps' and 'common' keys of a model of n channels: L taps per channel, all different; two groups with 3-tap rows of their own"""
    rng = np.random.default_rng(seed)
    gain = np.where(np.arange(n) % 2 == 0, 0.5, -0.75)
    return dict(taps=rng.uniform(-0.6, 0.6, (n, L)), common=dict(groups=_boards(n, quiet), gain=gain, sigma=[1.5, 2.5], taps=[[0.5, 0.7, 0.5], [0.9, -0.3, 0.1]]))


# ---------------------------------------------------------------------------------------------------- probes
PROBE_SIGMA = np.full(801, 2.2)
PROBE_SIGMA[[7, 250, 503]] = [0.0, 0.7, 5.1]
PROBE_T0 = [0, 1, 2, 3, -6, T34 - 5, 4001]          # 4001: the first white of lane 0 lies in the quad in front of t0's for every L > 2 (L = 2: t0 = 0)
PROBE_N = 2 * 256 + 7                               # two block seams, the halo lanes, the n & 3 tail


@pytest.fixture(scope='module')
def probe():
    cfg = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20, enable_noise=True, noise_model={'sigma': PROBE_SIGMA}, seed=NM.STAT_SEED), False)
    return make_engine(cfg), cfg


def _probe_model(eng, cfg, L, common):
    p = kernel_params(cfg)
    m = {'sigma': PROBE_SIGMA, 'taps': np.random.default_rng(10 + L).uniform(-1.0, 1.0, (801, L))}
    if common is not None:
        groups = np.arange(801) % 2
        groups[7] = -1
        m['common'] = dict(groups=groups, gain=common, sigma=[1.5, 3.0], taps=[[0.5, 0.7, 0.5], [1.0, -0.25, 0.125]])
    c = dict(cfg, noise_model=m)
    pmf, vmin = noise_pmf(c, 801)
    colour = noise_colour(c, 801)
    eng.set_noise_model(pmf, vmin)
    eng.set_noise_colour(**colour)
    assert colour['taps_q'].shape == (801 + (2 if common is not None else 0), max(L, 3) if common is not None else L)
    channels = (0, 7, int(p['n_tpc']) - 1, int(p['he_first']) + 3, 800)
    return NC.colour_model(pmf, vmin, colour), channels


@pytest.mark.parametrize('common', [None, 0.5, -1.0])
@pytest.mark.parametrize('L', [1, 2, 5, 16])
def test_probe_is_the_restatement(probe, L, common):
    eng, cfg = probe
    model, channels = _probe_model(eng, cfg, L, common)
    assert any((t0 - L + 1) >> 2 != t0 >> 2 for t0 in PROBE_T0) or L == 1
    for t0 in PROBE_T0:
        t = t0 + np.arange(PROBE_N, dtype=np.int64)
        for ch in channels:
            got = eng.noise_samples(ch, t0, PROBE_N)
            exp = NC.colour_values(model, NM.STAT_SEED, ch, t)
            assert got.dtype == np.int16 and np.array_equal(got.astype(np.int64), exp), (L, common, ch, t0, np.flatnonzero(got != exp)[:8])
        assert len(eng.noise_samples(0, t0, 0)) == 0
        assert np.array_equal(eng.noise_samples(0, t0, 3), eng.noise_samples(0, t0, PROBE_N)[:3])          # the single-sample form alone
    # the streams do something: the values differ from the whites, and a channel with a group from the same channel without
    white = NC.white_values(model, NM.STAT_SEED, 0, np.arange(PROBE_N, dtype=np.int64))
    assert L == 1 or not np.array_equal(eng.noise_samples(0, 0, PROBE_N), white)


def test_whites_probe_is_the_restatement(probe):
    eng, cfg = probe
    model, channels = _probe_model(eng, cfg, 5, 0.5)
    for t0 in PROBE_T0:
        t = t0 + np.arange(PROBE_N, dtype=np.int64)
        for row in (503, 801, 802):
            got = eng.noise_white_samples(row, t0, PROBE_N)
            assert np.array_equal(got.astype(np.int64), NC.white_values(model, NM.STAT_SEED, row, t)), (row, t0)
    assert not np.array_equal(eng.noise_white_samples(801, 0, 64), eng.noise_white_samples(802, 0, 64))
    assert not np.array_equal(eng.noise_white_samples(801, 0, 64), eng.noise_white_samples(0, 0, 64))       # common stream 0 is not channel 0
    with pytest.raises(WfsError, match='row outside'):
        eng.noise_white_samples(803, 0, 4)
    eng.set_noise_colour(None)
    with pytest.raises(WfsError, match='row outside'):
        eng.noise_white_samples(801, 0, 4)
    assert np.array_equal(eng.noise_white_samples(503, 5, 77), eng.noise_samples(503, 5, 77))                # white again


def test_long_run_is_the_restatement(probe):
    """2^20 samples, L = 16, common on: device == restatement, whose statistics tests/test_noise_colour_cpu.py holds"""
    eng, cfg = probe
    model, channels = _probe_model(eng, cfg, 16, 0.5)
    n = 1 << 20
    got = eng.noise_samples(250, NC.STAT_T0, n)
    assert np.array_equal(got.astype(np.int64), NC.colour_values(model, NM.STAT_SEED, 250, NC.STAT_T0 + np.arange(n, dtype=np.int64)))


# ---------------------------------------------------------------------------------------------------- identity: kind 4 == kind 3
@pytest.fixture(scope='module')
def small():
    base = with_fma(xenonnt_test_config(seed=99), False)
    p = kernel_params(base)
    sets, calls = _photon_sets(_designed_windows(p)[:3], np.asarray(base['gains'], dtype=np.float64))
    return base, sets, calls, {'sigma': _sigmas(494, seed=12)}


def test_unit_tap_is_the_white_model(small):
    base, sets, calls, model = small
    white = _profiled(dict(base, enable_noise=True, noise_model=model), sets)
    unit = _profiled(dict(base, enable_noise=True, noise_model=dict(model, taps=[1.0])), sets)
    assert white[0].noise_colour is None and unit[0].noise_colour is not None
    assert unit[1] == white[1] and unit[2] == white[2]          # the same records from the same kernels, of kind 4
    assert unit[3] == white[3] + 1                              # one more buffer: taps, groups and gains
    assert np.array_equal(unit[0].noise_samples(5, -3, 1000), white[0].noise_samples(5, -3, 1000))
    assert 'k_noise_colour_samples' in unit[0].kernel_times() and 'k_noise_colour_samples' not in white[0].kernel_times()


# ---------------------------------------------------------------------------------------------------- designed rows
@pytest.mark.parametrize('L', [5, 16])
@pytest.mark.parametrize('sum_signal', [False, True])
@pytest.mark.parametrize('channels', [494, 801])
@pytest.mark.parametrize('tw', [50, 20])
@pytest.mark.parametrize('resident', [0, 1])
def test_designed_rows(resident, tw, channels, sum_signal, L):
    base = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20 if channels == 801 else 0, trigger_window=tw, row_resident=resident,
                                       emit_sum_signal=sum_signal, seed=1234 + channels), False)
    cfg = dict(base, enable_noise=True, noise_model=dict({'sigma': _sigmas(channels)}, **_colour(channels, L)))
    p = kernel_params(cfg)
    sets, calls = _photon_sets(_designed_windows(p), np.asarray(cfg['gains'], dtype=np.float64))
    off = _oracle_photons(_off_config(cfg), calls)
    o_off = off.results()
    rows = _rows_with_sum(o_off, cfg, off)
    first, length = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    assert set((first % 4).tolist()) == {0, 1, 2, 3} and len(set((length % 4).tolist())) == 4
    assert 257 in length and length.max() > 2048 and first.max() > T34 and np.any((first < T34) & (first + length > T34))
    model, seed = _model_of(cfg)
    assert model['n_groups'] == 2 and (channels != 801 or model['group'][SUM_CHANNEL] == 0)
    table, ix = NC.materialise_colour(rows, len(o_off['dg_left']), model, seed)
    tab_cfg = _table_config(cfg, table)
    orc = _oracle_photons(tab_cfg, calls, ix)
    o = orc.results()
    eng = _engine_photons(cfg, sets, profiling=True)
    rec = eng.records()
    if sum_signal:
        exp = expected_sum_rows(o, kernel_params(tab_cfg), orc.tables['thr_zle'], noise=table, ix_rand=ix)
        assert len(exp) == len(calls)
        assert_sum_rows(eng, exp)
    assert np.any(rec['channel'] == SUM_CHANNEL) == (sum_signal and channels == 801)
    plain = rec[rec['channel'] != SUM_CHANNEL]
    assert plain.tobytes() == orc.pack_records().tobytes()
    kt = eng.kernel_times()
    res = resident == 1 and channels == 494 and tw == 50         # (as the white model: HE rows and a short hold-off keep rows on the accumulators)
    assert ('k_row_pulse' in kt) == res and ('k_pack_res' in kt) == res, sorted(kt)
    assert ('k_zle' in kt) == (not res or sum_signal) and ('k_pack' in kt) == (not res or sum_signal), sorted(kt)
    quiet = _as_records(off.pack_records())
    assert _bounds(plain) != _bounds(quiet)
    ch3 = lambda r: r[r['channel'] == 3]
    assert ch3(plain).tobytes() == ch3(quiet).tobytes() and len(ch3(plain)) > 0        # sigma 0 and no group
    white = _engine_photons(dict(cfg, noise_model={'sigma': _sigmas(channels)}), sets).records()
    assert white.tobytes() != rec.tobytes()
    eng_t = _engine_photons(tab_cfg, sets, ix)                  # the engine on the materialised table, through the kernels of the int16 table
    assert eng_t.records().tobytes() == rec.tobytes()


# ---------------------------------------------------------------------------------------------------- generated photons
def _generated(cfg, ins, ap=None):
    """engine with the coloured model of cfg, oracle with the materialised table (geometry from a noise-free oracle run)"""
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    off = make_oracle(_off_config(cfg), ap)
    off.simulate(s_ins, gid, ip)
    o_off = off.results()
    model, seed = _model_of(cfg)
    table, ix = NC.materialise_colour(_rows_with_sum(o_off, cfg, off), len(o_off['dg_left']), model, seed)
    orc = make_oracle(_table_config(cfg, table), ap)
    orc.set_noise_override(ix)
    orc.simulate(s_ins, gid, ip)
    eng = make_engine(cfg)
    eng.set_profiling(True)
    rs = None if cfg.get('save_full_truth', True) else run_sets(s_ins, key, cluster, cfg)[0]
    eng.load_instructions(s_ins, gid, cluster, key, ip, run_set=rs)
    eng.run()
    return eng, orc, off


@pytest.mark.parametrize('resident', [0, 1, 'auto'])
def test_every_row_source(resident):
    cfg = with_fma(xenonnt_test_config(seed=31, row_resident=resident, tile_local_min_photons=0, enable_noise=True,
                                       noise_model=dict({'sigma': _sigmas(494, seed=8)}, **_colour(494, 7, seed=2))), False)
    eng, orc, off = _generated(cfg, _instructions(EVERY_SOURCE))
    rec = eng.records()
    assert len(rec) > 0 and rec.tobytes() == orc.pack_records().tobytes()
    assert _bounds(rec) != _bounds(_as_records(off.pack_records()))
    kt = eng.kernel_times()
    assert 'k_s2_tile' in kt and 'k_tile_add' in kt, sorted(kt)
    if resident != 'auto':
        assert ('k_row_pulse' in kt) == (resident == 1), sorted(kt)


@pytest.mark.parametrize('seed', range(3))
def test_random_mix(seed):
    cfg, ins, ap = _random_case(53000 + seed)
    quiet = int(np.flatnonzero(np.asarray(cfg['noise_model']['sigma']) == 0)[0])
    cfg = dict(cfg, noise_model=dict(cfg['noise_model'], **_colour(494, [4, 16, 9][seed], seed=seed, quiet=(quiet,))))
    eng, orc, off = _generated(cfg, ins, ap)
    assert eng.records().tobytes() == orc.pack_records().tobytes()


def test_one_batch_or_two(small):
    base, sets, calls, model = small
    cfg = dict(base, enable_noise=True, noise_model=dict(model, **_colour(494, 16)))
    gains = np.asarray(cfg['gains'], dtype=np.float64)
    windows = _designed_windows(kernel_params(cfg))
    whole = _engine_photons(cfg, _photon_sets(windows, gains)[0]).records()
    eng = make_engine(cfg)
    eng.set_debug(False)
    parts = []
    for part in (windows[:4], windows[4:]):
        eng.load_photons(*_photon_sets(part, gains)[0])
        eng.run()
        parts.append(eng.records())
    assert len(parts[0]) and len(parts[1]) and np.concatenate(parts).tobytes() == whole.tobytes()


# ---------------------------------------------------------------------------------------------------- switches and clean-up
def test_clearing_and_resetting(small):
    base, sets, calls, model = small
    white_cfg = dict(base, enable_noise=True, noise_model=model)
    cfg = dict(base, enable_noise=True, noise_model=dict(model, **_colour(494, 5)))
    white_rec = _profiled(white_cfg, sets)[1]
    gc.collect()
    before = device_allocations()
    eng = make_engine(cfg)
    eng.set_debug(False)

    def run():
        eng.load_photons(*sets)
        eng.run()
        return eng.records().tobytes()
    coloured = run()
    assert coloured != white_rec
    count = lambda: device_allocations()[0]                 # (a run may allocate: the counts are compared around each switch alone)
    n = count()
    eng.set_noise_colour(None)                              # clearing the colour restores the white records
    assert count() == n - 1 and run() == white_rec
    n = count()
    eng.set_noise_colour(**eng.noise_colour)
    assert count() == n + 1 and run() == coloured
    n = count()
    eng.set_noise_model(*eng.noise_model)                   # setting the white model again clears the colour
    assert count() == n - 1 and run() == white_rec
    eng.set_noise_colour(**eng.noise_colour)
    n = count()
    eng.set_noise_model(None)
    assert count() == n - 2
    with pytest.raises(WfsError, match='no noise model'):   # colour without a model
        eng.set_noise_colour(**eng.noise_colour)
    import ctypes as C
    assert eng.lib.wfs_set_noise_colour(eng._h, C.c_int32(0), C.c_void_p(0), C.c_int32(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)) == -4      # WFS_E_STATE
    eng.close()
    assert device_allocations() == before


def _refusals():
    pmf, vmin = gaussian_pmf([1.0, 2.0, 0.5])               # three channels, values -12 .. 12
    unit = np.full((5, 1), 65536)
    grp, mix, cp = np.array([0, 1, -1]), np.array([100, -65536, 0]), pmf[:2]
    at = (2 ** 29 - 1) // 12                                # sum |taps| * 12 <= 2^29 - 1 < 2^29
    return pmf, vmin, unit, grp, mix, cp, at


@pytest.mark.parametrize('case,match', [
    ('taps17', 'n_taps'), ('overflow', 'taps_q of row 4'), ('group_high', 'group of channel 1'), ('group_low', 'group of channel 2'),
    ('mix', 'mix_q of channel 0'), ('negative', 'negative'), ('sum', 'common_pmf of group 1 does not sum to 1'), ('null', 'null')])
def test_invalid_colour_is_refused(small, case, match):
    pmf, vmin, unit, grp, mix, cp, at = _refusals()
    eng = make_engine(small[0])
    eng.set_noise_model(pmf, vmin)
    args = dict(taps_q=unit.copy(), group=grp.copy(), mix_q=mix.copy(), common_pmf=cp.copy())
    if case == 'taps17':
        args['taps_q'] = np.ones((5, 17), dtype=np.int32)
    elif case == 'overflow':
        args['taps_q'][4, 0] = -(at + 1)
    elif case == 'group_high':
        args['group'][1] = 2
    elif case == 'group_low':
        args['group'][2] = -2
    elif case == 'mix':
        args['mix_q'][0] = 65537
    elif case == 'negative':
        args['common_pmf'][0, :2] = [-1e-3, args['common_pmf'][0, 1] + args['common_pmf'][0, 0] + 1e-3]
    elif case == 'sum':
        args['common_pmf'][1, 12] += 1e-8
    white = eng.noise_samples(1, 0, 64)
    if case == 'null':
        import ctypes as C
        rc = eng.lib.wfs_set_noise_colour(eng._h, C.c_int32(1), C.c_void_p(0), C.c_int32(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
        assert rc != 0 and match in eng.lib.wfs_last_error(eng._h).decode()
    else:
        with pytest.raises(WfsError, match=match):
            eng.set_noise_colour(**args)
    assert np.array_equal(eng.noise_samples(1, 0, 64), white)          # a refused colour changes nothing
    args = dict(taps_q=unit.copy(), group=grp, mix_q=mix, common_pmf=cp)
    args['taps_q'][4, 0] = -at                              # the edge of the bound is accepted
    eng.set_noise_colour(**args)
    model = NC.colour_model(pmf, vmin, args)
    assert np.array_equal(eng.noise_samples(1, -9, 300).astype(np.int64), NC.colour_values(model, int(kernel_params(small[0])['seed']), 1, -9 + np.arange(300, dtype=np.int64)))


def test_close_returns_the_colour(small):
    base, sets, calls, model = small
    gc.collect()
    start = device_allocations()
    for cycle in range(2):
        eng = make_engine(dict(base, enable_noise=True, noise_model=dict(model, **_colour(494, 5))))
        eng.load_photons(*sets)
        assert eng.run()['n_records'] > 0 and len(eng.noise_samples(0, 0, 100)) == 100
        assert device_allocations()[0] > start[0]
        eng.close()
        assert device_allocations() == start, cycle


def test_plugin_equals_rawdata():
    import wfsim_amd
    from wfsim_amd import ministrax
    rows = []
    for i in range(2):
        rows += [dict(type=1, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=800), dict(type=2, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=120)]
    ins = _instructions(rows)
    ins['event_number'] = np.arange(len(ins)) // 2
    n = len(xenonnt_test_config()['gains'])
    model = {'sigma': 2.2, 'taps': [0.25, 0.5, 0.75, 0.5, 0.25], 'common': {'groups': (np.arange(n) // 8) % 3 - 1, 'gain': 0.6, 'sigma': 1.8, 'taps': [0.7, 0.7]}}
    out = []
    for m in (model, {'sigma': 2.2}):
        cfg = xenonnt_test_config(seed=5, chunk_size=0.5, instructions=ins.copy(), enable_noise=True, noise_model=m)
        assert 'noise_data' not in cfg
        chunks = ministrax.run_plugin(wfsim_amd.RawRecordsFromFaxNT(cfg))
        out.append(np.concatenate([c.data for c in chunks['raw_records']]))
    assert len(out[0]) > 0 and np.all(np.diff(out[0]['time']) >= 0)
    assert out[0].tobytes() != out[1].tobytes()             # not the white records
    cfg = xenonnt_test_config(seed=5, chunk_size=0.5, enable_noise=True, noise_model=model)
    direct = np.concatenate([w['records'] for w in wfsim_amd.RawData(cfg).iter_windows(ins.copy())])
    assert np.sort(direct, order=['time', 'channel']).tobytes() == np.sort(out[0], order=['time', 'channel']).tobytes()
