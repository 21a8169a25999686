"""Full readout (config 'full_readout', wfs_set_full_readout; MI355X only): every channel of a digitise window.

The pin is the unchanged oracle on anchored input (tests/full_readout.py, checked on the CPU by tests/test_full_readout_cpu.py): two
photons of gain 0 on every TPC channel at the window's earliest and latest photon give the oracle a row of the union range in every
row slot, and its records for that input are the engine's in full-readout mode on the original input, byte for byte.  The model kinds
of noise go through the materialised-table route of tests/noise_slow.py over the FULL rows.
"""
import gc

import numpy as np
import pytest

from tests import full_readout as FR
from tests import noise_slow as NS
from tests.helpers import ap_tables_from_golden, make_engine, make_oracle, with_fma
from tests.noise_model import oracle_rows
from tests.sum_signal import SUM_CHANNEL
from tests.test_gpu_noise_model import EVERY_SOURCE, _engine_photons, _instructions, _off_config, _oracle_photons, _photon_sets, _table_config
from tests.test_gpu_noise_slow import _coloured_slow, _model_of
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.engine import WfsError, device_allocations
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot
    monkeypatch.setenv('WFS_RES_MAX_LEN', '256')        # resident rows in segments of 256 samples


def _base(channels, tw, **kw):
    return with_fma(xenonnt_test_config(high_energy_deamplification_factor=20 if channels == 801 else 0, trigger_window=tw, seed=1234 + channels, **kw), False)


def _noise_config(base, channels, kind):
    if kind == 'off':
        return dict(base, enable_noise=False)
    if kind in ('int16', 'float', 'int16_short'):        # (a table shorter than 512 samples wraps inside a block of 256: the sample-by-sample path)
        noise = np.random.default_rng(5).integers(-24, 25, size=(TABLE_LEN[kind], channels)).astype(np.float64 if kind == 'float' else np.int16)
        if kind == 'float':
            noise = noise + np.random.default_rng(6).uniform(-0.5, 0.5, noise.shape)
        return dict(base, enable_noise=True, noise_data=noise)
    m = {'sigma': FR.sigmas(channels)}
    if kind == 'coloured':
        m.update(_coloured_slow(channels, 5, (4, 6, 10), quiet=(FR.QUIET,)))
        del m['slow'], m['common']['slow']
    elif kind == 'slow':
        m.update(_coloured_slow(channels, 5, (4, 6, 10), quiet=(FR.QUIET,)))
    return dict(base, enable_noise=True, noise_model=m)


TABLE_LEN = {'int16': 3000, 'float': 3000, 'int16_short': 300}
_EXPECTED = {}


def _expected(channels, tw, kind='white', n_windows=None):
    """records of the anchored and of the plain oracle for one configuration, computed once for the tests that share it"""
    key = (channels, tw, kind, n_windows)
    if key not in _EXPECTED:
        cfg = _noise_config(_base(channels, tw), channels, kind)
        p = kernel_params(cfg)
        windows = FR.windows_of(p)[:n_windows]
        sets, calls, anchored = FR.photon_input(cfg, p, windows)
        out = dict(cfg=cfg, p=p, windows=windows, sets=sets, ix=None, ix_plain=None)
        if kind == 'off':
            out['full'], out['plain'] = _oracle_photons(cfg, anchored).pack_records().tobytes(), _oracle_photons(cfg, calls).pack_records().tobytes()
        elif kind in TABLE_LEN:
            # injected start indices: the last ones so close to the end of the table that every row of their windows wraps
            ix = np.random.default_rng(7).integers(0, TABLE_LEN[kind], len(windows))
            ix[-2:] = [TABLE_LEN[kind] - 10, TABLE_LEN[kind] - 1]
            out['ix'] = out['ix_plain'] = ix
            out['full'], out['plain'] = _oracle_photons(cfg, anchored, ix).pack_records().tobytes(), _oracle_photons(cfg, calls, ix).pack_records().tobytes()
        else:
            model, seed = _model_of(cfg)
            orc, tab_cfg, ix, rows = FR.model_expectation(cfg, model, seed, calls, anchored)
            out['full'], out['rows'] = orc.pack_records().tobytes(), rows
            o_off = _oracle_photons(_off_config(cfg), calls).results()
            table, ixp = NS.materialise_slow(oracle_rows(o_off), len(o_off['dg_left']), model, seed)
            out['plain'] = _oracle_photons(_table_config(cfg, table), calls, ixp).pack_records().tobytes()
            out['plain_rows'] = oracle_rows(o_off)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def _run(cfg, sets, ix=None):
    eng = _engine_photons(cfg, sets, ix, profiling=True)
    return eng, eng.records()


def _plain(rec):
    return rec[rec['channel'] != SUM_CHANNEL]


# ---------------------------------------------------------------------------------------------------- 1: designed windows
@pytest.mark.parametrize('sum_signal', [False, True])
@pytest.mark.parametrize('channels', [494, 801])
@pytest.mark.parametrize('tw', [50, 20])
@pytest.mark.parametrize('resident', [0, 1])
def test_designed_windows(resident, tw, channels, sum_signal):
    e = _expected(channels, tw)
    cfg = dict(e['cfg'], row_resident=resident, emit_sum_signal=sum_signal)
    eng, rec = _run(dict(cfg, full_readout=True), e['sets'])
    assert eng.full_readout and _plain(rec).tobytes() == e['full']
    kt = eng.kernel_times()
    assert 'k_row_empty' in kt and 'k_rows_widen' in kt and 'k_pack_res' in kt, sorted(kt)
    res = resident == 1 and channels == 494 and tw == 50
    assert ('k_row_pulse' in kt) == res, sorted(kt)
    c = eng.counts
    n_win = len(e['windows'])
    slots = 494 + (253 if channels == 801 else 0)
    assert c['n_groups'] >= n_win and c['n_rows'] == n_win * (slots + (1 if sum_signal else 0))      # (every window has a bottom pulse, hence a sum row)
    assert np.any(rec['channel'] == SUM_CHANNEL) == (sum_signal and channels == 801)        # (factor 0 and no noise column: a flat sum row)


@pytest.mark.parametrize('resident,tw,channels,sum_signal', [(1, 50, 494, False), (0, 20, 801, True), (1, 50, 801, True)])
def test_switch_off_is_the_parent(resident, tw, channels, sum_signal):
    """the same cases without the key, and with it False: the parent's bytes from the parent's kernels; the sum row of the run with
    the switch keeps the range and the value it has without"""
    e = _expected(channels, tw)
    cfg = dict(e['cfg'], row_resident=resident, emit_sum_signal=sum_signal)
    off_eng, off_rec = _run(cfg, e['sets'])
    assert not off_eng.full_readout and _plain(off_rec).tobytes() == e['plain'] and e['plain'] != e['full']
    assert not {'k_row_empty', 'k_rows_widen'} & set(off_eng.kernel_times())
    assert _run(dict(cfg, full_readout=False), e['sets'])[1].tobytes() == off_rec.tobytes()
    if sum_signal:
        rec = _run(dict(cfg, full_readout=True), e['sets'])[1]
        assert np.any(rec['channel'] == SUM_CHANNEL) and rec[rec['channel'] == SUM_CHANNEL].tobytes() == off_rec[off_rec['channel'] == SUM_CHANNEL].tobytes()


@pytest.mark.parametrize('kind', ['off', 'int16', 'int16_short', 'float', 'coloured', 'slow'])
@pytest.mark.parametrize('resident,tw,channels', [(1, 50, 494), (0, 20, 801)])
def test_each_noise_source(kind, resident, tw, channels):
    e = _expected(channels, tw, kind, n_windows=None if kind == 'off' or kind in TABLE_LEN else 6)
    cfg = dict(e['cfg'], row_resident=resident, full_readout=True)
    eng, rec = _run(cfg, e['sets'], e['ix'])
    assert rec.tobytes() == e['full'] and (kind == 'off' or e['full'] != e['plain'])      # (without noise a row without a pulse is flat: no record)
    assert _run(dict(cfg, full_readout=False), e['sets'], e['ix_plain'])[1].tobytes() == e['plain']


# ---------------------------------------------------------------------------------------------------- 2: store everything
N_MODEL = 740
BEYOND = 745                    # the HE channel of top channel 245, which no designed window has a pulse on


@pytest.fixture(scope='module')
def whole_rows():
    """zle_threshold -40000: no sample can reach it, every row is stored whole; channel 12 keeps the ordinary threshold"""
    channels, tw = 801, 50
    sigma = FR.sigmas(channels)[:N_MODEL]                   # (the HE channels from 740 on lie beyond the model)
    base = _base(channels, tw, zle_threshold=-40000, special_thresholds={'12': FR.ZLE_ADC})
    cfg = dict(base, enable_noise=True, noise_model={'sigma': sigma}, row_resident=1)
    p = kernel_params(cfg)
    windows = FR.windows_of(p)[:6]
    sets, calls, anchored = FR.photon_input(cfg, p, windows)
    model, seed = _model_of(cfg)
    orc, tab_cfg, ix, rows = FR.model_expectation(cfg, model, seed, calls, anchored)
    plain_rows = oracle_rows(_oracle_photons(_off_config(cfg), calls).results())
    eng, rec = _run(dict(cfg, full_readout=True), sets)
    return dict(cfg=cfg, p=p, eng=eng, rec=rec, rows=rows, plain_rows=plain_rows, expected=orc.pack_records().tobytes(), n_windows=len(windows))


def test_store_everything_threshold(whole_rows):
    w = whole_rows
    rec, p = w['rec'], w['p']
    assert rec.tobytes() == w['expected']
    have = {(r[0], r[1]) for r in w['plain_rows']}
    baseline = int(p['baseline'])
    checked = 0
    per_channel = {}
    for win, ch, first, n in w['rows']:
        if ch == 12:
            continue                                        # the ordinary threshold
        per_channel.setdefault(ch, FR.reassemble(rec, ch))
        data = per_channel[ch][first]                       # (a row starts on its first sample: the even landing is relative to the row)
        last = (n - 1) // 2 * 2
        assert len(data) == last + 1, (win, ch)             # ONE interval: the whole row, right down to an even sample
        if (win, ch) not in have and ch < N_MODEL and ch % 19 == 0:
            noise = w['eng'].noise_samples(ch, first, n).astype(np.int64)
            assert np.array_equal(data, np.maximum(baseline + noise, 0)[:last + 1]), (win, ch)
            checked += 1
    assert checked >= 100
    assert sum(len(v) for v in per_channel.values()) == len([r for r in w['rows'] if r[1] != 12])
    own = [(r[2], r[2] + r[3]) for r in w['plain_rows'] if r[1] == 12]
    at12 = FR.reassemble(rec, 12)
    assert at12 and all(any(a <= first < b for a, b in own) for first in at12)      # the ordinary threshold: its own pulses alone
    assert w['eng'].counts['n_intervals'] >= len(w['rows']) - w['n_windows']


# ---------------------------------------------------------------------------------------------------- 3: special channels
def test_special_channels(whole_rows):
    """beyond the noise source's channels and sigma 0: flat baseline -- whole-row records when everything is stored, none at the
    ordinary threshold; a channel of gain 0 has its row (the oracle turns it off: pulse.py:89, so its records are looked at directly)"""
    w = whole_rows
    p, rec = w['p'], w['rec']
    have = {(r[0], r[1]) for r in w['plain_rows']}
    baseline = int(p['baseline'])
    flat = 0
    for ch in (FR.QUIET, BEYOND):                           # sigma 0; beyond the noise source's channels
        for first, data in FR.reassemble(rec, ch).items():
            win = [r[0] for r in w['rows'] if r[1] == ch and r[2] == first][0]
            if (win, ch) not in have:
                assert np.all(data == baseline)
                flat += 1
    assert flat == sum(w['n_windows'] - len([r for r in w['plain_rows'] if r[1] == ch]) for ch in (FR.QUIET, BEYOND)) >= w['n_windows']
    # the ordinary threshold and a dead PMT
    gains = np.asarray(w['cfg']['gains'], dtype=np.float64).copy()
    gains[40] = 0.0
    cfg = dict(w['cfg'], zle_threshold=FR.ZLE_ADC, special_thresholds={'40': -40000}, gains=gains)
    windows = FR.windows_of(p)[:6]
    sets, calls, anchored = FR.photon_input(cfg, p, windows)
    model, seed = _model_of(cfg)
    orc, tab_cfg, ix, rows = FR.model_expectation(cfg, model, seed, calls, anchored)
    assert 40 not in {r[1] for r in rows}
    eng, rec = _run(dict(cfg, full_readout=True), sets)
    assert rec[rec['channel'] != 40].tobytes() == orc.pack_records().tobytes()
    for ch in (FR.QUIET, BEYOND):
        own = {r[2] for r in w['plain_rows'] if r[1] == ch}
        assert all(any(f <= first < f + 4000 for f in own) for first in FR.reassemble(rec, ch))      # records in its own pulses' windows alone
    dead = FR.reassemble(rec, 40)
    assert len(dead) == len(windows)                        # its row in every window, stored whole: noise on the baseline
    by_window = {r[0]: r for r in rows if r[1] == 41}
    for win, (_, _, first, n) in by_window.items():
        noise = eng.noise_samples(40, first, n).astype(np.int64)
        assert np.array_equal(dead[first], np.maximum(baseline + noise, 0)[:(n - 1) // 2 * 2 + 1])


# ---------------------------------------------------------------------------------------------------- 4: generated photons
@pytest.mark.parametrize('resident', [0, 1, 'auto'])
@pytest.mark.parametrize('bright', [True, False])
def test_generated_photons(resident, bright):
    ap = ap_tables_from_golden()
    cfg = with_fma(xenonnt_test_config(seed=31, row_resident=resident, tile_local_min_photons=0, tile_local_bright=bright, enable_noise=True,
                                       enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap, noise_model={'sigma': FR.sigmas(494)}), False)
    ins = _instructions(EVERY_SOURCE)
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    off = make_oracle(_off_config(cfg), ap)
    off.simulate(s_ins, gid, ip)
    o = off.results()
    assert 3 in o['call_kind']                              # PMT afterpulses
    n_tpc = int(kernel_params(cfg)['n_tpc'])
    o_full = FR.replay(make_oracle(_off_config(cfg)), o, n_tpc).results()
    assert np.array_equal(o_full['dg_left'], o['dg_left']) and np.array_equal(o_full['dg_right'], o['dg_right'])
    model, seed = _model_of(cfg)
    table, ix = NS.materialise_slow(oracle_rows(o_full), len(o['dg_left']), model, seed)
    orc = make_oracle(_table_config(cfg, table))
    orc.set_noise_override(ix)
    FR.replay(orc, o, n_tpc)
    eng = make_engine(dict(cfg, full_readout=True))
    eng.set_profiling(True)
    out = {}
    for on in (True, False):
        eng.set_full_readout(on)
        eng.load_instructions(s_ins, gid, cluster, key, ip)
        counts = eng.run()
        out[on] = dict(rec=eng.records().tobytes(), kinds=eng.tile_kernels().copy(), truth=[a.copy() for a in eng.truth()], kt=set(eng.kernel_times()), counts=counts)
        if on:      # the device's own photons are the oracle's, set by set
            ph = eng.photons()
            assert counts['n_photons'] == len(o['ph_t']) and np.array_equal(np.sort(ph['t']), np.sort(o['ph_t'])) and np.array_equal(np.sort(ph['gain']), np.sort(o['ph_gain']))
    assert out[True]['rec'] == orc.pack_records().tobytes() and out[True]['rec'] != out[False]['rec']
    assert np.array_equal(out[True]['kinds'], out[False]['kinds']) and out[True]['kinds'].max() >= 1
    for a, b in zip(out[True]['truth'], out[False]['truth']):
        assert np.array_equal(a, b, equal_nan=True)
    assert {'k_s2_tile', 'k_tile_add', 'k_row_empty'} <= out[True]['kt'] and 'k_row_empty' not in out[False]['kt']
    assert out[True]['counts']['n_rows'] == 494 * len(o['dg_left'])


# ---------------------------------------------------------------------------------------------------- 5: one batch or two
@pytest.mark.parametrize('resident', [0, 1])
def test_one_batch_or_two(resident):
    e = _expected(494, 50)
    cfg = dict(e['cfg'], row_resident=resident, full_readout=True)
    gains = np.asarray(cfg['gains'], dtype=np.float64)
    eng = make_engine(cfg)
    eng.set_debug(False)
    parts = []
    for part in (e['windows'][:4], e['windows'][4:]):
        eng.load_photons(*_photon_sets(part, gains)[0])
        eng.run()
        parts.append(eng.records())
    assert len(parts[0]) and len(parts[1]) and np.concatenate(parts).tobytes() == e['full']


# ---------------------------------------------------------------------------------------------------- 6: optical input
def test_optical_nveto():
    from wfsim_amd.workloads import nveto_config, optical_instructions
    noise = np.random.default_rng(9).integers(-9, 10, size=(4000, 120)).astype(np.int16)
    noise[:, 10:16] = np.random.default_rng(10).integers(-40, 41, size=(4000, 6))
    cfg = nveto_config(seed=31, enable_noise=True, noise_data=noise)
    ins, channels, timings = optical_instructions(3, 5000.0, 3)
    ins['time'] = [1_000_000, 1_009_000, 1_020_000]
    order, key, cluster = schedule(ins, cfg)
    gid = order.astype(np.uint32)
    plain = make_oracle(_off_config(cfg))
    plain.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, int(1e6))
    o = plain.results()
    assert len(o['dg_left']) == 3
    ix = np.array([17, 1234, 3990])
    orc = make_oracle(cfg)
    orc.set_noise_override(ix)
    FR.replay(orc, o, 120, gains=cfg['gains'])
    rows = {(r[0], r[1]) for r in oracle_rows(orc.results())}
    assert len(rows) == 3 * 119                             # every channel of the array but the dead PMT, which the oracle turns off
    eng = make_engine(dict(cfg, full_readout=True))
    recs = {}
    for on in (True, False):
        eng.set_full_readout(on)
        eng.set_noise_offsets([])
        for attempt in range(2):
            eng.load_optical(ins[order], gid, cluster, key, channels, timings, int(1e6))
            counts = eng.run()
            g = eng.groups()
            v = np.full(len(g['left']), -1, dtype=np.int64)
            v[g['right'] >= g['left']] = ix
            eng.set_noise_offsets(v)
        recs[on] = eng.records()
        if on:
            ph = eng.photons()
            live = np.asarray(cfg['gains']) > 0
            assert np.array_equal(np.sort(ph['t'][live[ph['ch']]]), np.sort(o['ph_t'][live[o['ph_ch']]])) and counts['n_rows'] == 3 * 120
    # the dead PMT's rows: noise below the threshold, no record; every other row as the anchored oracle has it
    assert 7 not in recs[True]['channel'] and recs[True].tobytes() == orc.pack_records().tobytes()
    assert recs[True].tobytes() != recs[False].tobytes() and len(recs[True]) > len(recs[False])


# ---------------------------------------------------------------------------------------------------- 7: switch and clean-up
def test_toggle_close_and_capacity(monkeypatch):
    e = _expected(494, 50)
    gc.collect()
    before = device_allocations()
    eng = make_engine(dict(e['cfg'], full_readout=True))
    eng.set_debug(False)
    for on in (True, False, True):
        eng.set_full_readout(on)
        eng.load_photons(*e['sets'])
        eng.run()
        assert eng.records().tobytes() == (e['full'] if on else e['plain']), on
    eng.close()
    assert device_allocations() == before
    # the debug copy of the unfinished rows lists the rows WITH pulses, each over its window's range; the records are the same bytes
    eng = make_engine(dict(e['cfg'], full_readout=True))
    eng.set_debug(True)
    eng.load_photons(*e['sets'])
    eng.run()
    r = eng.rows()
    have = {(w, ch) for w, ch, _, _ in e['plain_rows']}
    assert sorted(zip(r['channel'].tolist(), (r['right'] - r['left'] + 1).tolist())) == sorted((ch, n) for w, ch, _, n in e['rows'] if (w, ch) in have and ch < 494)      # (factor 0: the engine has no HE rows)
    assert len(r['data']) == int((r['right'] - r['left'] + 1).sum()) and eng.records().tobytes() == e['full']
    eng.close()
    # a batch beyond the cap ends in WFS_E_CAPACITY with a message that names full readout, before any buffer is sized from it
    monkeypatch.setenv('WFS_FULL_READOUT_MAX_SAMPLES', '100000')
    eng = make_engine(dict(e['cfg'], full_readout=True))
    eng.load_photons(*e['sets'])
    with pytest.raises(WfsError, match=r'error -3: full readout: \d+ rows without a pulse need \d+ finished samples'):
        eng.run()
    eng.set_full_readout(False)                             # the engine is still good for a batch that fits
    eng.load_photons(*e['sets'])
    eng.run()
    assert eng.records().tobytes() == e['plain']
    eng.close()
    assert device_allocations() == before


# ---------------------------------------------------------------------------------------------------- 8: through the plugin
def test_plugin():
    import wfsim_amd
    from wfsim_amd import ministrax
    rows = []
    for i in range(2):
        rows += [dict(type=1, time=FR.MS * (i + 1), x=1, y=1, z=-20.0, amp=800), dict(type=2, time=FR.MS * (i + 1), x=1, y=1, z=-20.0, amp=120)]
    ins = _instructions(rows)
    ins['event_number'] = np.arange(len(ins)) // 2
    model = {'sigma': FR.sigmas(494)}
    out = {}
    for on in (True, False):
        cfg = xenonnt_test_config(seed=5, chunk_size=0.5, instructions=ins.copy(), enable_noise=True, noise_model=model, full_readout=on)
        chunks = ministrax.run_plugin(wfsim_amd.RawRecordsFromFaxNT(cfg))
        out[on] = np.concatenate([c.data for c in chunks['raw_records']])
    assert np.all(np.diff(out[True]['time']) >= 0) and len(out[True]) > len(out[False]) > 0
    cfg = xenonnt_test_config(seed=5, chunk_size=0.5, enable_noise=True, noise_model=model, full_readout=True)
    direct = np.concatenate([w['records'] for w in wfsim_amd.RawData(cfg).iter_windows(ins.copy())])
    by_time = lambda r: np.sort(r, order=['time', 'channel'])
    assert by_time(direct).tobytes() == by_time(out[True]).tobytes() and by_time(direct).tobytes() != by_time(out[False]).tobytes()
    loud = np.isin(out[True]['channel'], FR.LOUD)
    assert loud.sum() > np.isin(out[False]['channel'], FR.LOUD).sum()
