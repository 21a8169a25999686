"""Slow baseline motion in the noise model drawn on the device (config 'noise_model' with 'slow', wfs_set_noise_slow, noise kind 5 of the
row kernels; MI355X only).

The definition is restated in numpy in tests/noise_slow.py (test_noise_slow_cpu.py holds its statistics on the CPU).  The device is pinned
against it as the coloured model is: sample by sample through Engine.noise_samples / noise_slow_samples -- exact integers, so ``==`` --
and end to end through the table-noise path: the model's values for the rows of a run are written into an int16 table with one stretch
per digitise window, and oracle and engine replay that table.  Records are compared byte for byte.
"""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import noise_colour as NC
from tests import noise_model as NM
from tests import noise_slow as NS
from tests.helpers import make_engine, make_oracle, with_fma
from tests.sum_signal import SUM_CHANNEL, assert_sum_rows, expected_sum_rows
from tests.test_gpu_noise_colour import _colour
from tests.test_gpu_noise_model import (EVERY_SOURCE, MS, T34, _as_records, _bounds, _designed_windows, _engine_photons, _instructions,
                                        _off_config, _oracle_photons, _photon_sets, _profiled, _random_case, _rows_with_sum, _sigmas,
                                        _table_config)
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.engine import WfsError, device_allocations
from wfsim_amd.noise_model import gaussian_pmf, noise_colour, noise_pmf, noise_slow
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule, run_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _model_of(cfg):
    pmf, vmin = noise_pmf(cfg, 801)
    return NS.slow_model(pmf, vmin, noise_colour(cfg, 801), noise_slow(cfg, 801)), int(kernel_params(cfg)['seed'])


def _slow(n, shifts, seed=1):
    """the 'slow' key of a model of n channels: amplitudes per channel and level, all different, some zero"""
    amp = np.random.default_rng(100 + seed).uniform(-0.8, 0.8, (n, len(shifts)))
    amp[5::11, 0] = 0.0
    return dict(shifts=list(shifts), amplitude=amp)


def _coloured_slow(n, L, shifts, seed=1, quiet=(3,)):
    """'taps', 'common' and 'slow' of a model of n channels; the two common streams have slow levels of their own (one level off in the second)"""
    m = _colour(n, L, seed=seed, quiet=quiet)
    m['slow'] = _slow(n, shifts, seed)
    m['slow']['amplitude'][list(quiet)] = 0.0           # the quiet channels stay quiet: sigma 0 would do it too (every knot is 0), this makes it plain
    camp = np.random.default_rng(200 + seed).uniform(-0.9, 0.9, (2, len(shifts)))
    camp[1, -1] = 0.0
    m['common'] = dict(m['common'], slow=camp)
    return m


# ---------------------------------------------------------------------------------------------------- probes
PROBE_SIGMA = np.full(801, 2.2)
PROBE_SIGMA[[7, 250, 503]] = [0.0, 0.7, 5.1]
# block starts on, before and behind knots of every level; negative t (the high counter words are 0xFFFFFFFF); the segment seam of 1024;
# 2^34 - 5: the quad index t >> 2 of the whites leaves 32 bits; 2^30 - 3: a knot of the level with shift 30 inside the run
PROBE_T0 = [0, 1, 2, 3, -6, -2 ** 8 - 3, 2 ** 8 - 5, 2 ** 10 - 2, T34 - 5, 2 ** 30 - 3]
PROBE_N = 2 * 256 + 7                               # two block seams, 33 knots of a level with shift 4, the n & 3 tail
PROBE_LEVELS = {'4': (4,), '8': (8,), '4_6_10': (4, 6, 10), '4_to_11': tuple(range(4, 12)), '30': (30,)}
PROBE_COLOURS = ['white', 'L5', 'L16_common']
# for S alone, on top: the quad index (t >> 4) >> 2 of the knots of the fastest level leaves 32 bits at t = 2^38 (the high counter word
# of a level turns positive), and that of the level with shift 8 at 2^42
SLOW_T0 = PROBE_T0 + [2 ** 38 - 5, 2 ** 42 - 259]


@pytest.fixture(scope='module')
def probe():
    cfg = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20, enable_noise=True, noise_model={'sigma': PROBE_SIGMA}, seed=NM.STAT_SEED), False)
    return make_engine(cfg), cfg


def _probe_model(eng, cfg, shifts, colour_kind):
    p = kernel_params(cfg)
    m = {'sigma': PROBE_SIGMA, 'slow': _slow(801, shifts, seed=len(shifts))}
    if colour_kind != 'white':
        L = 5 if colour_kind == 'L5' else 16
        m['taps'] = np.random.default_rng(10 + L).uniform(-1.0, 1.0, (801, L))
    if colour_kind == 'L16_common':
        groups = np.arange(801) % 2
        groups[7] = -1
        camp = np.zeros((2, len(shifts)))
        camp[0, 0], camp[1, -1] = 0.75, -1.25           # each common stream has a slow level of its own
        m['common'] = dict(groups=groups, gain=-1.0, sigma=[1.5, 3.0], taps=[[0.5, 0.7, 0.5], [1.0, -0.25, 0.125]], slow=camp)
    c = dict(cfg, noise_model=m)
    pmf, vmin = noise_pmf(c, 801)
    colour, slow = noise_colour(c, 801), noise_slow(c, 801)
    eng.set_noise_model(pmf, vmin)
    if colour is not None:
        eng.set_noise_colour(**colour)
    eng.set_noise_slow(**slow)
    assert (colour is None) == (colour_kind == 'white') and slow['slow_q'].shape == (801 + (2 if colour_kind == 'L16_common' else 0), len(shifts))
    channels = (0, 7, int(p['n_tpc']) - 1, int(p['he_first']) + 3, 800)
    return NS.slow_model(pmf, vmin, colour, slow), channels


@pytest.mark.parametrize('colour_kind', PROBE_COLOURS)
@pytest.mark.parametrize('levels', list(PROBE_LEVELS))
def test_probe_is_the_restatement(probe, levels, colour_kind):
    eng, cfg = probe
    shifts = PROBE_LEVELS[levels]
    model, channels = _probe_model(eng, cfg, shifts, colour_kind)
    for t0 in PROBE_T0:
        t = t0 + np.arange(PROBE_N, dtype=np.int64)
        for ch in channels:
            got = eng.noise_samples(ch, t0, PROBE_N)
            exp = NS.slow_noise_values(model, NM.STAT_SEED, ch, t)
            assert got.dtype == np.int16 and np.array_equal(got.astype(np.int64), exp), (levels, colour_kind, ch, t0, np.flatnonzero(got != exp)[:8])
        assert len(eng.noise_samples(0, t0, 0)) == 0
        assert np.array_equal(eng.noise_samples(0, t0, 3), eng.noise_samples(0, t0, PROBE_N)[:3])          # the single-sample form alone
    # the levels do something: channel 0 differs from the same model without them
    with_levels = eng.noise_samples(0, 0, PROBE_N)
    eng.set_noise_slow(None)
    assert not np.array_equal(eng.noise_samples(0, 0, PROBE_N), with_levels)


@pytest.mark.parametrize('colour_kind', ['white', 'L16_common'])
def test_slow_probe_is_the_restatement(probe, colour_kind):
    eng, cfg = probe
    model, channels = _probe_model(eng, cfg, tuple(range(4, 12)), colour_kind)
    rows = channels + ((801, 802) if colour_kind == 'L16_common' else ())
    for t0 in SLOW_T0:
        t = t0 + np.arange(PROBE_N, dtype=np.int64)
        for row in rows:
            got = eng.noise_slow_samples(row, t0, PROBE_N)
            assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), NS.slow_values(model, NM.STAT_SEED, row, t)), (row, t0)
        assert np.array_equal(eng.noise_slow_samples(0, t0, 3), eng.noise_slow_samples(0, t0, PROBE_N)[:3])
    assert np.any(eng.noise_slow_samples(0, 0, 64)) and not np.any(eng.noise_slow_samples(7, 0, 64))          # sigma 0: every knot is 0
    with pytest.raises(WfsError, match='row outside'):
        eng.noise_slow_samples(len(model['slow_q']), 0, 4)
    eng.set_noise_slow(None)
    with pytest.raises(WfsError, match='no noise model with slow levels'):
        eng.noise_slow_samples(0, 0, 4)


def test_full_value_beyond_the_knot_quad_wrap(probe):
    """the full value through both forms where the high counter word of the knots is positive"""
    eng, cfg = probe
    model, channels = _probe_model(eng, cfg, (4, 6, 10), 'L16_common')
    for t0 in SLOW_T0[-2:]:
        t = t0 + np.arange(PROBE_N, dtype=np.int64)
        for ch in channels:
            assert np.array_equal(eng.noise_samples(ch, t0, PROBE_N).astype(np.int64), NS.slow_noise_values(model, NM.STAT_SEED, ch, t)), (ch, t0)


def test_sample_probe_and_engine_refusals(probe):
    eng, cfg = probe
    model, channels = _probe_model(eng, cfg, (4, 9), 'L16_common')
    out = np.zeros(8, dtype=np.int32)
    p = out.ctypes.data_as(C.c_void_p)

    def refused(row, t0, n, buf, match):
        rc = eng.lib.wfs_noise_slow_samples(eng._h, C.c_int32(row), C.c_int64(t0), C.c_int64(n), buf)
        assert rc == -1 and match in eng.lib.wfs_last_error(eng._h).decode(), (row, t0, n, eng.lib.wfs_last_error(eng._h).decode())      # WFS_E_INVALID
    refused(-1, 0, 4, p, 'row outside')
    refused(803, 0, 4, p, 'row outside')
    refused(0, 0, -1, p, 'n outside 0 .. 2^30 or null buffer')
    refused(0, 0, 2 ** 30 + 1, p, 'n outside 0 .. 2^30 or null buffer')
    refused(0, 0, 4, C.c_void_p(0), 'n outside 0 .. 2^30 or null buffer')
    refused(0, 2 ** 63 - 4, 5, p, 't0 + n overflows')
    assert not np.any(out)                                     # nothing was written
    assert eng.lib.wfs_noise_slow_samples(eng._h, C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_void_p(0)) == 0       # n = 0 needs no buffer
    assert np.array_equal(eng.noise_slow_samples(802, 2 ** 63 - 9, 8).astype(np.int64),
                          NS.slow_values(model, NM.STAT_SEED, 802, 2 ** 63 - 9 + np.arange(8, dtype=np.int64)))        # the last t0 that is accepted
    # the Engine's own checks: shapes, and the rows of the model and colour it last set (the C entry points take no row count)
    q = np.zeros((803, 2), dtype=np.int32)
    for shifts, slow_q in (([[4, 9]], q), ([4, 9], q[:, 0]), ([4, 9, 12], q), (4, q)):
        with pytest.raises(ValueError, match=r'set_noise_slow: shifts must be \[n_levels\], slow_q \[n_channels \+ n_groups\]\[n_levels\]'):
            eng.set_noise_slow(shifts, slow_q)
    with pytest.raises(ValueError, match='set_noise_slow: the model has 801 channels and 2 common streams: slow_q must have 803 rows, not 801'):
        eng.set_noise_slow([4, 9], q[:801])
    before = eng.noise_samples(0, 0, 64)
    eng.set_noise_colour(None)                                 # the rows of a colour that is gone: too many, and too few of them the other way round
    with pytest.raises(ValueError, match='set_noise_slow: the model has 801 channels and 0 common streams: slow_q must have 801 rows, not 803'):
        eng.set_noise_slow([4, 9], q)
    with pytest.raises(ValueError, match='set_noise_colour: the model has 801 channels: taps_q must have 801 rows'):
        eng.set_noise_colour(np.full((803, 1), 65536))
    with pytest.raises(ValueError, match='set_noise_colour: the model has 801 channels: taps_q must have 803 rows'):
        eng.set_noise_colour(np.full((801, 1), 65536), np.zeros(801), np.zeros(801), np.full((2, 3), 1 / 3))
    assert not np.array_equal(eng.noise_samples(0, 0, 64), before)         # (white now: the colour and its levels are gone)
    eng.set_noise_slow([4, 9], q[:801])


def test_long_run_is_the_restatement(probe):
    """2^20 samples, eight levels, L = 16, common on: device == restatement, whose statistics tests/test_noise_slow_cpu.py holds"""
    eng, cfg = probe
    model, channels = _probe_model(eng, cfg, tuple(range(4, 12)), 'L16_common')
    n = 1 << 20
    got = eng.noise_samples(250, NC.STAT_T0, n)
    assert np.array_equal(got.astype(np.int64), NS.slow_noise_values(model, NM.STAT_SEED, 250, NC.STAT_T0 + np.arange(n, dtype=np.int64)))


# ---------------------------------------------------------------------------------------------------- identity: kind 5 == kinds 4 and 3
@pytest.fixture(scope='module')
def small():
    base = with_fma(xenonnt_test_config(seed=99), False)
    p = kernel_params(base)
    sets, calls = _photon_sets(_designed_windows(p)[:3], np.asarray(base['gains'], dtype=np.float64))
    return base, sets, calls, {'sigma': _sigmas(494, seed=12)}


def test_zero_amplitudes_are_the_model_without_levels(small):
    base, sets, calls, model = small
    zero = dict(shifts=[4, 7, 12], amplitude=[0.0, 0.0, 0.0])
    col = _colour(494, 5)
    white = _profiled(dict(base, enable_noise=True, noise_model=model), sets)
    white5 = _profiled(dict(base, enable_noise=True, noise_model=dict(model, slow=zero)), sets)
    assert white[0].noise_slow is None and white5[0].noise_slow is not None and white5[0].noise_colour is None
    assert white5[1] == white[1] and white5[2] == white[2]      # the same records from the same kernels, of kind 5
    assert white5[3] == white[3] + 1                            # one more buffer: shifts, amplitudes and the unit taps
    assert np.array_equal(white5[0].noise_samples(5, -3, 1000), white[0].noise_samples(5, -3, 1000))
    coloured = _profiled(dict(base, enable_noise=True, noise_model=dict(model, **col)), sets)
    coloured5 = _profiled(dict(base, enable_noise=True, noise_model=dict(model, slow=zero, **dict(col, common=dict(col['common'], slow=[0.0, 0.0, 0.0])))), sets)
    assert coloured5[1] == coloured[1] and coloured5[1] != white[1] and coloured5[3] == coloured[3] + 1
    assert np.array_equal(coloured5[0].noise_samples(5, -3, 1000), coloured[0].noise_samples(5, -3, 1000))
    assert not np.any(coloured5[0].noise_slow_samples(494, -3, 1000))


# ---------------------------------------------------------------------------------------------------- designed rows
@pytest.mark.parametrize('sum_signal', [False, True])
@pytest.mark.parametrize('channels', [494, 801])
@pytest.mark.parametrize('tw', [50, 20])
@pytest.mark.parametrize('resident', [0, 1])
def test_designed_rows(monkeypatch, resident, tw, channels, sum_signal):
    monkeypatch.setenv('WFS_RES_MAX_LEN', '256')        # resident rows in segments of 256 samples: every longer row has seams
    base = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20 if channels == 801 else 0, trigger_window=tw, row_resident=resident,
                                       emit_sum_signal=sum_signal, seed=1234 + channels), False)
    cfg = dict(base, enable_noise=True, noise_model=dict({'sigma': _sigmas(channels)}, **_coloured_slow(channels, 5, (4, 6, 10))))
    p = kernel_params(cfg)
    sets, calls = _photon_sets(_designed_windows(p), np.asarray(cfg['gains'], dtype=np.float64))
    off = _oracle_photons(_off_config(cfg), calls)
    o_off = off.results()
    rows = _rows_with_sum(o_off, cfg, off)
    first, length = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    assert set((first % 4).tolist()) == {0, 1, 2, 3} and len(set((length % 4).tolist())) == 4
    assert 257 in length and length.max() > 2048 and first.max() > T34 and np.any((first < T34) & (first + length > T34))
    model, seed = _model_of(cfg)
    assert model['n_groups'] == 2 and (channels != 801 or model['group'][SUM_CHANNEL] == 0) and np.any(model['slow_q'][model['n_channels']:])
    table, ix = NS.materialise_slow(rows, len(o_off['dg_left']), model, seed)
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
    no_levels = dict(cfg['noise_model'], common=dict(cfg['noise_model']['common']))
    del no_levels['slow'], no_levels['common']['slow']
    assert _engine_photons(dict(cfg, noise_model=no_levels), sets).records().tobytes() != rec.tobytes()
    eng_t = _engine_photons(tab_cfg, sets, ix)                  # the engine on the materialised table, through the kernels of the int16 table
    assert eng_t.records().tobytes() == rec.tobytes()


# ---------------------------------------------------------------------------------------------------- generated photons
def _generated(cfg, ins, ap=None):
    """engine with the model of cfg, oracle with the materialised table (geometry from a noise-free oracle run)"""
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    off = make_oracle(_off_config(cfg), ap)
    off.simulate(s_ins, gid, ip)
    o_off = off.results()
    model, seed = _model_of(cfg)
    table, ix = NS.materialise_slow(_rows_with_sum(o_off, cfg, off), len(o_off['dg_left']), model, seed)
    orc = make_oracle(_table_config(cfg, table), ap)
    orc.set_noise_override(ix)
    orc.simulate(s_ins, gid, ip)
    eng = make_engine(cfg)
    eng.set_profiling(True)
    rs = None if cfg.get('save_full_truth', True) else run_sets(s_ins, key, cluster, cfg)[0]
    eng.load_instructions(s_ins, gid, cluster, key, ip, run_set=rs)
    eng.run()
    return eng, orc, off


@pytest.mark.parametrize('colour_kind', ['white', 'coloured'])
@pytest.mark.parametrize('resident', [0, 1, 'auto'])
def test_every_row_source(monkeypatch, resident, colour_kind):
    monkeypatch.setenv('WFS_RES_MAX_LEN', '256')
    m = _coloured_slow(494, 7, (4, 5, 9, 13), seed=2) if colour_kind == 'coloured' else dict(slow=_slow(494, (4, 5, 9, 13), seed=2))
    cfg = with_fma(xenonnt_test_config(seed=31, row_resident=resident, tile_local_min_photons=0, enable_noise=True,
                                       noise_model=dict({'sigma': _sigmas(494, seed=8)}, **m)), False)
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
    cfg, ins, ap = _random_case(54000 + seed)
    quiet = int(np.flatnonzero(np.asarray(cfg['noise_model']['sigma']) == 0)[0])
    shifts = [(4, 8), tuple(range(4, 12)), (6, 17, 30)][seed]
    cfg = dict(cfg, noise_model=dict(cfg['noise_model'], **_coloured_slow(494, [4, 16, 9][seed], shifts, seed=seed, quiet=(quiet,))))
    eng, orc, off = _generated(cfg, ins, ap)
    assert eng.records().tobytes() == orc.pack_records().tobytes()


def test_one_batch_or_two(small):
    base, sets, calls, model = small
    cfg = dict(base, enable_noise=True, noise_model=dict(model, **_coloured_slow(494, 16, (4, 6, 10))))
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
    col = _colour(494, 5)
    coloured_rec = _profiled(dict(base, enable_noise=True, noise_model=dict(model, **col)), sets)[1]
    white_rec = _profiled(dict(base, enable_noise=True, noise_model=model), sets)[1]
    cfg = dict(base, enable_noise=True, noise_model=dict(model, **_coloured_slow(494, 5, (4, 6, 10))))
    gc.collect()
    before = device_allocations()
    eng = make_engine(cfg)
    eng.set_debug(False)

    def run():
        eng.load_photons(*sets)
        eng.run()
        return eng.records().tobytes()
    slow = run()
    assert slow != coloured_rec and slow != white_rec
    count = lambda: device_allocations()[0]                 # (a run may allocate: the counts are compared around each switch alone)
    n = count()
    eng.set_noise_slow(None)                                # clearing the levels restores the coloured records
    assert count() == n - 1 and run() == coloured_rec
    n = count()
    eng.set_noise_slow(**eng.noise_slow)
    assert count() == n + 1 and run() == slow
    n = count()
    eng.set_noise_colour(**eng.noise_colour)                # setting the colour again clears the levels
    assert count() == n - 1 and run() == coloured_rec
    eng.set_noise_slow(**eng.noise_slow)
    n = count()
    eng.set_noise_colour(None)                              # clearing the colour clears them too
    assert count() == n - 2 and run() == white_rec
    eng.set_noise_slow(eng.noise_slow['shifts'], eng.noise_slow['slow_q'][:494])      # (without a colour the rows are the channels alone)
    assert run() not in (white_rec, coloured_rec, slow)
    n = count()
    eng.set_noise_model(*eng.noise_model)                   # setting the white model again clears the levels
    assert count() == n - 1 and run() == white_rec
    eng.set_noise_slow(eng.noise_slow['shifts'], eng.noise_slow['slow_q'][:494])
    n = count()
    eng.set_noise_model(None)
    assert count() == n - 2
    with pytest.raises(WfsError, match='no noise model'):   # levels without a model
        eng.set_noise_slow(**eng.noise_slow)
    assert eng.lib.wfs_set_noise_slow(eng._h, C.c_int32(0), C.c_void_p(0), C.c_void_p(0)) == -4      # WFS_E_STATE
    eng.close()
    assert device_allocations() == before


def _refusals():
    pmf, vmin = gaussian_pmf([1.0, 2.0, 0.5])               # three channels, values -12 .. 12
    at = (2 ** 29 - 1) // 12                                # (sum |taps| + sum |slow|) * 12 <= 2^29 - 1 < 2^29
    return pmf, vmin, at


@pytest.mark.parametrize('colour', [False, True])
@pytest.mark.parametrize('case,match', [
    ('levels9', 'n_levels outside 0 .. 8'), ('negative', 'n_levels outside 0 .. 8'), ('shift3', r'shifts\[0\] outside 4 .. 30'),
    ('shift31', r'shifts\[1\] outside 4 .. 30'), ('equal', 'not strictly ascending at level 1'), ('descending', 'not strictly ascending at level 1'),
    ('overflow', r'slow_q of row 2: \(sum \|taps\| \+ sum \|slow\|\) \* max \|value\| reaches 2\^29'), ('null', 'null shifts or slow_q')])
def test_invalid_levels_are_refused(small, case, match, colour):
    pmf, vmin, at = _refusals()
    eng = make_engine(small[0])
    eng.set_noise_model(pmf, vmin)
    taps = np.array([[30000, -20000], [65536, 0], [-1000, 99000], [65536, 65536]])
    if colour:
        eng.set_noise_colour(taps, [0, -1, 0], [32768, 0, -65536], pmf[:1])
    rows = 4 if colour else 3
    tapsum = int(np.abs(taps[2]).sum()) if colour else 65536
    shifts, q = np.array([4, 9]), np.full((rows, 2), 1000, dtype=np.int64)
    if case == 'levels9':
        shifts, q = np.arange(4, 13), np.zeros((rows, 9), dtype=np.int64)
    elif case == 'shift3':
        shifts = np.array([3, 9])
    elif case == 'shift31':
        shifts = np.array([4, 31])
    elif case == 'equal':
        shifts = np.array([9, 9])
    elif case == 'descending':
        shifts = np.array([9, 8])
    elif case == 'overflow':
        q[2] = [-(at - tapsum - 5), 6]                      # together at + 1
    before = eng.noise_samples(1, 0, 64)
    if case in ('null', 'negative'):
        rc = eng.lib.wfs_set_noise_slow(eng._h, C.c_int32(1 if case == 'null' else -1), C.c_void_p(0), C.c_void_p(0))
        assert rc == -1 and match in eng.lib.wfs_last_error(eng._h).decode()      # WFS_E_INVALID
    else:
        with pytest.raises(WfsError, match=match):
            eng.set_noise_slow(shifts, q)
    assert np.array_equal(eng.noise_samples(1, 0, 64), before)          # refused levels change nothing
    with pytest.raises(WfsError, match='no noise model with slow levels'):
        eng.noise_slow_samples(0, 0, 4)
    q = np.full((rows, 2), 1000, dtype=np.int64)
    q[2] = [-(at - tapsum - 5), 5]                          # the edge of the bound is accepted: (sum |taps| + sum |slow|) * 12 <= 2^29 - 1
    eng.set_noise_slow([4, 9], q)
    args = dict(taps_q=taps, group=np.array([0, -1, 0]), mix_q=np.array([32768, 0, -65536]), common_pmf=pmf[:1]) if colour else None
    model = NS.slow_model(pmf, vmin, args, dict(shifts=[4, 9], slow_q=q))
    seed = int(kernel_params(small[0])['seed'])
    for ch in range(3):
        assert np.array_equal(eng.noise_samples(ch, -9, 300).astype(np.int64), NS.slow_noise_values(model, seed, ch, -9 + np.arange(300, dtype=np.int64))), ch


def test_close_returns_the_levels(small):
    base, sets, calls, model = small
    gc.collect()
    start = device_allocations()
    for cycle in range(2):
        eng = make_engine(dict(base, enable_noise=True, noise_model=dict(model, **_coloured_slow(494, 5, (4, 6, 10)))))
        eng.load_photons(*sets)
        assert eng.run()['n_records'] > 0 and len(eng.noise_samples(0, 0, 100)) == 100 and len(eng.noise_slow_samples(495, 0, 100)) == 100
        assert device_allocations()[0] > start[0]
        eng.close()
        assert device_allocations() == start, cycle


def test_plugin_equals_rawdata():
    import wfsim_amd
    from wfsim_amd import ministrax
    from wfsim_amd.noise_model import slow_levels
    rows = []
    for i in range(2):
        rows += [dict(type=1, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=800), dict(type=2, time=MS * (i + 1), x=1, y=1, z=-20.0, amp=120)]
    ins = _instructions(rows)
    ins['event_number'] = np.arange(len(ins)) // 2
    n = len(xenonnt_test_config()['gains'])
    coloured = {'sigma': 2.2, 'taps': [0.25, 0.5, 0.75, 0.5, 0.25], 'common': {'groups': (np.arange(n) // 8) % 3 - 1, 'gain': 0.6, 'sigma': 1.8, 'taps': [0.7, 0.7]}}
    sl = slow_levels(2e5, 4e6, 1.5, 2.2)
    model = dict(coloured, slow=sl, common=dict(coloured['common'], slow=[0.5] * len(sl['shifts'])))
    out = []
    for m in (model, coloured):
        cfg = xenonnt_test_config(seed=5, chunk_size=0.5, instructions=ins.copy(), enable_noise=True, noise_model=m)
        assert 'noise_data' not in cfg
        chunks = ministrax.run_plugin(wfsim_amd.RawRecordsFromFaxNT(cfg))
        out.append(np.concatenate([c.data for c in chunks['raw_records']]))
    assert len(out[0]) > 0 and np.all(np.diff(out[0]['time']) >= 0)
    assert out[0].tobytes() != out[1].tobytes()             # not the records without the levels
    cfg = xenonnt_test_config(seed=5, chunk_size=0.5, enable_noise=True, noise_model=model)
    direct = np.concatenate([w['records'] for w in wfsim_amd.RawData(cfg).iter_windows(ins.copy())])
    assert np.sort(direct, order=['time', 'channel']).tobytes() == np.sort(out[0], order=['time', 'channel']).tobytes()
