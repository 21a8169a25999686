"""The digitise-window rule on runs of the reference over designed instruction spacings (tests/golden/window_edges.npz: the nVeto
configuration; window_edges_tpc.npz: the bundled TPC one; tests/window_edges.py holds the case table, make_golden.py window_edges ran
the reference's RawDataOptical on it with pmt_transit_time_spread 0).  CPU only:
  * the designed differences are in the fixtures -- recomputed from the fixtures' own instruction times, pl_right and the reference's
    flush record, not from the case table
  * the oracle (its optical scheduler on the stored inputs; the injected-photon replay) equals the fixtures bit for bit
  * the host scheduler's clusters are the ones the reference's verdicts imply
The device: tests/test_gpu_window_edges.py.
"""
import numpy as np
import pytest

from tests import window_edges as WE
from tests.helpers import golden, make_oracle, photons_by_call_and_channel, replay_chain_on_oracle, window_edges_config, with_fma

NAMES = ['nveto', 'tpc']
_cache = {}


def fixture(name):
    """(fixture, config, sample duration, right_raw_extension, decisions recomputed from the fixture) -- loaded once"""
    if name not in _cache:
        d = golden(WE.FIXTURES[name])
        cfg = window_edges_config(name)
        dt, rext = int(cfg['sample_duration']), int(cfg['right_raw_extension'])
        _cache[name] = (d, cfg, dt, rext, WE.fixture_decisions(d, rext, dt))
    return _cache[name]


def labels(d):
    sec = [WE.SECTIONS[i] for i in d['dec_section']]
    return sec, [str(v) for v in d['dec_variant']], [str(t) for t in d['dec_tag']]


def delta_histogram(name):
    """{diff: number of decisions} for the decisions within 1 ns of the threshold, from the fixture's own numbers"""
    dec = fixture(name)[4]
    return {k: sum(1 for x in dec if x['diff'] == k) for k in (-1, 0, 1)}


def window_of_pulse(d, j):
    return int(np.searchsorted(d['dg_first_pulse'], j, side='right') - 1)


@pytest.mark.parametrize('name', NAMES)
def test_every_decision_is_the_designed_one(name):
    """per cluster of the stored instructions: its difference from the threshold, from instruction times and recorded pulse ends, is the
    designed one; the reference digitised the cache exactly where the difference is positive and a pulse existed; the case table
    rebuilds the stored inputs"""
    d, cfg, dt, rext, dec = fixture(name)
    s = WE.CASES[name](cfg)
    ins, channels, timings = s.inputs()
    assert np.array_equal(ins, d['instructions']) and np.array_equal(channels, d['channels']) and np.array_equal(timings, d['timings'])
    assert int(cfg['pmt_transit_time_spread']) == 0 and len(d['call_kind']) == len(ins)
    assert [x['first'] for x in dec] == d['dec_first'].tolist() and [x['n'] for x in dec] == d['dec_n'].tolist()
    assert [x['tmin'] for x in dec] == d['dec_tmin'].tolist()
    for c, x in enumerate(dec):
        assert (x['diff'] is not None) == bool(d['dec_has_diff'][c]), c
        if x['diff'] is not None:
            assert x['diff'] == d['dec_diff'][c], c
        if d['dec_has_delta'][c]:
            assert x['diff'] == d['dec_delta'][c], c
        assert x['flush'] == bool(d['dec_expect'][c]) == (x['diff'] is not None and x['diff'] > 0), (c, x)
    # every entry of digitize_pulse_cache is in front of a cluster (or the last one, behind everything); every non-empty cache is a window
    fl = d['flush_at_call']
    assert fl[-1] == len(ins) and set(fl[:-1].tolist()) <= set(d['dec_first'].tolist()) and len(set(fl.tolist())) == len(fl)
    pulses_before = d['call_pulse_off'][fl]
    pulses_before = np.unique(pulses_before)
    assert np.array_equal(pulses_before[pulses_before > 0], d['dg_first_pulse'] + d['dg_n_pulses'])
    h = delta_histogram(name)
    print(f'\n{name}: {len(dec)} decisions, {int(d["dec_has_delta"].sum())} designed; at -1 / 0 / +1 ns from the threshold: {h[-1]} / {h[0]} / {h[1]}')
    assert all(h[k] == int((d['dec_has_delta'] & (d['dec_delta'] == k)).sum()) >= 3 for k in (-1, 0, 1))         # (none by accident)


@pytest.mark.parametrize('name', NAMES)
def test_section_a_threshold(name):
    """all three differences in each way E is set, a flush only at +1; how E was set is read off the recorded pulse ends"""
    d, cfg, dt, rext, dec = fixture(name)
    sec, var, tag = labels(d)
    for v in WE.A_VARIANTS:
        got = {}
        for c in range(len(dec)):
            if sec[c] == 'A' and var[c] == v and d['dec_has_delta'][c]:
                x = dec[c]
                got[x['diff']] = x['flush']
                ends = [dec[k]['end'] if k >= 0 else None for k in range(c - 3, c)]
                if v == 'previous':
                    assert ends[2] == x['E'] and (dec[c - 1]['E'] is None or dec[c - 1]['E'] < x['E'])       # the previous cluster raised the maximum
                elif v == 'three_back':
                    assert ends[0] == x['E'] and ends[1] < x['E'] and ends[2] < x['E'] and ends[1] < ends[2]        # held from three clusters back
                    assert not dec[c - 1]['flush'] and not dec[c - 2]['flush']
                else:
                    assert ends[1] == ends[2] == x['E'] and dec[c - 2]['E'] < x['E']     # reached by two clusters
        assert got == {-1: False, 0: False, 1: True}, (v, got)


def test_section_b_whose_time_counts():
    d, cfg, dt, rext, dec = fixture('nveto')
    sec, var, tag = labels(d)
    npl = np.diff(d['call_pulse_off'])
    nin = np.diff(d['call_in_off'])
    nraw = d['instructions']['_last'] - d['instructions']['_first']
    t = d['instructions']['time']
    for v, raw in (('first_equals_last', False), ('all_cut', True)):
        got = {}
        for c in range(len(dec)):
            if sec[c] == 'B' and var[c] == v and d['dec_has_delta'][c]:
                x = dec[c]
                k = x['first']
                assert t[k] == x['tmin'] and npl[k] == 0 and (nraw[k] > 0) == raw and x['n'] == 2 and npl[k + 1] > 0 and t[k + 1] > t[k]
                if raw:         # negative, at / behind the cutoff, on the dead PMT (the last enters the call and makes no pulse)
                    a, b = int(d['instructions']['_first'][k]), int(d['instructions']['_last'][k])
                    tm, ch = d['timings'][a:b], d['channels'][a:b]
                    assert (tm < 0).any() and (tm >= int(d['cutoff'])).any() and nin[k] == 1 and cfg['gains'][ch[(tm >= 0) & (tm < int(d['cutoff']))]].max() == 0
                # at -1 the pulse-making instruction alone would have been behind the threshold
                assert t[k + 1] - x['E'] - rext > 0
                got[x['diff']] = x['flush']
        assert got == {-1: False, 1: True}, (v, got)
    n_empty_flush = 0
    for c in range(len(dec)):
        if sec[c] == 'B' and tag[c] == 'pulseless':
            x = dec[c]
            assert x['end'] is None and dec[c + 1]['E'] == x['E']                           # E unchanged
            if var[c].startswith('pulseless_beyond'):
                assert x['diff'] == 1 and x['flush'] and dec[c + 1]['flush'] and dec[c + 1]['end'] is not None
                # two entries of digitize_pulse_cache, one window: the second found the cache empty
                assert d['call_pulse_off'][dec[c]['first']] == d['call_pulse_off'][dec[c + 1]['first']]
                n_empty_flush += 1
            else:
                assert var[c] == 'pulseless_within' and x['diff'] < 0 and not x['flush'] and dec[c + 1]['diff'] in (-1, 1)
                assert dec[c + 1]['flush'] == (dec[c + 1]['diff'] > 0)
    assert n_empty_flush == 2
    assert sorted(dec[c + 1]['diff'] for c in range(len(dec)) if var[c] == 'pulseless_within' and tag[c] == 'pulseless') == [-1, 1]


def test_section_c_before_any_pulse():
    d, cfg, dt, rext, dec = fixture('nveto')
    sec, var, tag = labels(d)
    assert sec[:5] == ['C'] * 5
    for c in range(3):
        assert dec[c]['end'] is None and dec[c]['E'] is None and not dec[c]['flush']
        assert dec[c + 1]['tmin'] - dec[c]['tmin'] > rext
    assert dec[3]['E'] is None and dec[3]['end'] is not None and not dec[3]['flush'] and d['call_pulse_off'][dec[3]['first']] == 0
    assert dec[4]['diff'] == 1 and dec[4]['flush']
    assert d['dg_first_pulse'][0] == 0 and d['dg_n_pulses'][0] == np.diff(d['call_pulse_off'])[dec[3]['first']]


def test_section_d_even_landing():
    d, cfg, dt, rext, dec = fixture('nveto')
    sec, var, tag = labels(d)
    tw = int(cfg['trigger_window'])
    seen = set()
    for c in range(len(dec)):
        if sec[c] == 'D' and d['dec_parity'][c] >= 0:
            j = int(d['call_pulse_off'][dec[c]['first']])
            w = window_of_pulse(d, j)
            assert d['dg_first_pulse'][w] == j
            pl = np.arange(j, j + d['dg_n_pulses'][w])
            raw = int(d['pl_left'][pl].min()) - tw
            assert raw % 2 == d['dec_parity'][c] and d['dg_left'][w] == raw - raw % 2 and d['dg_right'][w] == d['pl_right'][pl].max() + tw
            n_clusters = sum(1 for k in range(len(dec)) if j <= d['call_pulse_off'][dec[k]['first']] < j + len(pl) and dec[k]['end'] is not None)
            assert n_clusters == (1 if var[c] == 'single' else 2)
            seen.add((var[c], int(d['dec_parity'][c])))
    assert seen == {('single', 0), ('single', 1), ('merged', 0), ('merged', 1)}


@pytest.mark.parametrize('name', NAMES)
def test_section_e_rows(name):
    d, cfg, dt, rext, dec = fixture(name)
    sec, var, tag = labels(d)
    cl = [c for c in range(len(dec)) if sec[c] == 'E']
    assert len(cl) == 4 and dec[cl[0]]['flush'] and not any(dec[c]['flush'] for c in cl[1:]) and dec[cl[-1] + 1]['flush']
    j0 = int(d['call_pulse_off'][dec[cl[0]]['first']])
    w = window_of_pulse(d, j0)
    j1 = j0 + int(d['dg_n_pulses'][w])
    assert d['dg_first_pulse'][w] == j0 and j1 == d['call_pulse_off'][dec[cl[-1] + 1]['first']]           # one window, all four clusters
    cluster_of_pulse = np.array([max(c for c in cl if d['call_pulse_off'][dec[c]['first']] <= j) for j in range(j0, j1)])
    ch, left, right = d['pl_ch'][j0:j1], d['pl_left'][j0:j1], d['pl_right'][j0:j1]
    by_ch = {int(c): sorted(set(cluster_of_pulse[ch == c].tolist())) for c in np.unique(ch)}
    x = [c for c, v in by_ch.items() if len(v) == 3]
    y = [c for c, v in by_ch.items() if v == [cl[-1]]]
    assert x == [63] and 64 in by_ch and len(cfg['gains']) - 1 in y
    rows = slice(int(d['dg_row_off'][w]), int(d['dg_row_off'][w + 1]))
    rch = d['row_ch'][rows].tolist()
    r = rch.index(63)
    # the row spans the union of its three pulses (relative to the window; rawdata.py:258-259), with idle stretches between them
    assert d['row_left'][rows][r] == left[ch == 63].min() - d['dg_left'][w] - int(cfg['trigger_window'])
    assert d['row_right'][rows][r] == right[ch == 63].max() - d['dg_left'][w] + int(cfg['trigger_window'])
    lx, rx = np.sort(left[ch == 63]), np.sort(right[ch == 63])
    assert np.all(lx[1:] - rx[:-1] > 2 * int(cfg['trigger_window']) + 1)
    assert ((d['zle_digit'] == w) & (d['zle_ch'] == 63)).sum() >= 3
    # the pulses that start and end the window sit on two other channels
    p, q = int(ch[np.argmin(left)]), int(ch[np.argmax(right)])
    assert len({p, q, 63, 64} | set(y)) >= 5 and (left == left.min()).sum() == 1 and (right == right.max()).sum() == 1
    assert by_ch[p] == [cl[0]] and by_ch[q] == [cl[-1]]
    if name == 'tpc':
        assert p < cfg['n_top_pmts'] <= q and 493 in y and 500 + p in rch           # a top channel (with its high-energy row), a bottom one


def test_section_f_gaps_and_equal_times():
    d, cfg, dt, rext, dec = fixture('nveto')
    sec, var, tag = labels(d)
    t = d['instructions']['time']
    npl = np.diff(d['call_pulse_off'])
    f = [c for c in range(len(dec)) if sec[c] == 'F']
    by = {v: [c for c in f if var[c] == v] for v in set(var[c] for c in f)}
    # a gap of exactly rext: one cluster, whose minimum (an instruction without photons, exactly at the threshold) decides -- no flush;
    # were the second instruction a cluster of its own, it would be rext behind the threshold
    c = by['gap_rext'][1]
    k = dec[c]['first']
    assert dec[c]['n'] == 2 and t[k + 1] - t[k] == rext and npl[k] == 0 and npl[k + 1] > 0 and dec[c]['diff'] == 0 and not dec[c]['flush']
    assert t[k + 1] - dec[c]['E'] - rext == rext
    # a gap of rext + 1: two clusters, the second rext + 1 behind the threshold
    c = by['gap_rext_plus_1'][1]
    k = dec[c]['first']
    assert dec[c]['n'] == 1 and dec[c + 1]['n'] == 1 and t[k + 1] - t[k] == rext + 1 and npl[k] == 0 and npl[k + 1] > 0
    assert dec[c]['diff'] == 0 and not dec[c]['flush'] and dec[c + 1]['diff'] == rext + 1 and dec[c + 1]['flush']
    c = by['gap_rext_pulses'][0]
    k = dec[c]['first']
    assert dec[c]['n'] == 2 and t[k + 1] - t[k] == rext and t[k + 2] - t[k + 1] == rext + 1 and dec[c + 1]['first'] == k + 2 and not dec[c + 1]['flush']
    # equal instruction times: one cluster, processed in input order
    eq = by['equal_times']
    assert [dec[c]['n'] for c in eq] == [2, 2, 3] and all(np.all(t[dec[c]['first']:dec[c]['first'] + dec[c]['n']] == dec[c]['tmin']) for c in eq)
    assert [dec[c]['diff'] for c in eq[1:]] == [1, 0] and [dec[c]['flush'] for c in eq[1:]] == [True, False]
    assert np.array_equal(d['truth']['event_number'], d['instructions']['event_number'])


@pytest.mark.parametrize('name', NAMES)
def test_oracle_optical_scheduler_equals_the_fixture(name):
    """orc.simulate_optical on the stored inputs: calls, the photon lists on entry and behind the (constant) transit time, pulses and
    windows EQUAL the reference's"""
    d, cfg, dt, rext, dec = fixture(name)
    ins = d['instructions']
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), d['channels'], d['timings'], int(d['cutoff']))
    r = orc.results()
    assert len(r['call_kind']) == len(d['call_kind']) == len(ins)
    assert np.array_equal(r['call_ph_off'], d['call_in_off']) and np.array_equal(r['call_ph_off'], d['call_ph_off'])
    assert photons_by_call_and_channel(r['call_ph_off'], r['opt_in_t'], r['opt_in_ch']) == photons_by_call_and_channel(d['call_in_off'], d['in_t'], d['in_ch'])
    assert photons_by_call_and_channel(r['call_ph_off'], r['ph_t'], r['ph_ch']) == photons_by_call_and_channel(d['call_ph_off'], d['ph_t'], d['ph_ch'])
    assert np.array_equal(d['ph_t'], d['in_t'] + int(cfg['pmt_transit_time_mean']))
    live = np.asarray(cfg['gains'])[r['pl_ch']] > 0 if len(r['pl_ch']) else np.zeros(0, bool)
    assert live.all()
    for a, b in [('pl_ch', 'pl_ch'), ('pl_left', 'pl_left'), ('pl_right', 'pl_right'), ('pl_nph', 'pl_photons'), ('dg_left', 'dg_left'),
                 ('dg_right', 'dg_right'), ('dg_first_pulse', 'dg_first_pulse'), ('dg_n_pulses', 'dg_n_pulses')]:
        assert np.array_equal(r[a], d[b]), a


@pytest.mark.parametrize('name', NAMES)
def test_oracle_replay_bit_exact(name):
    """the reference's photons and gains injected call by call: pulses, windows, rows and ZLE tuples bit for bit, in both arithmetic forms"""
    d, cfg, dt, rext, dec = fixture(name)
    for fma in (True, False):
        r = replay_chain_on_oracle(make_oracle(with_fma(cfg, fma)), d)
        for a, b in [('pl_ch', 'pl_ch'), ('pl_left', 'pl_left'), ('pl_right', 'pl_right'), ('pl_nph', 'pl_photons'),
                     ('dg_left', 'dg_left'), ('dg_right', 'dg_right'), ('dg_row_off', 'dg_row_off'), ('row_ch', 'row_ch'),
                     ('row_left', 'row_left'), ('row_right', 'row_right'), ('row_data_off', 'row_data_off'), ('row_data', 'row_data')]:
            assert np.array_equal(r[a], d[b]), (a, fma)
        for k in ['ch', 'left', 'right', 'data_off', 'data', 'digit']:
            assert np.array_equal(r['zl_' + k], d['zle_' + k]), (k, fma)
    assert len(d['zle_ch']) >= len(d['dg_left'])


@pytest.mark.parametrize('name', NAMES)
def test_host_scheduler_clusters(name):
    """scheduler.schedule on the stored instructions: its clusters are those of the fixture (np.diff(time) > rext, section F included),
    every digitise the reference made sits in front of one of them, and the rule evaluated on them -- cluster minimum of the keys,
    recorded pulse ends -- gives the reference's verdicts, one by one"""
    from wfsim_amd.scheduler import schedule
    d, cfg, dt, rext, dec = fixture(name)
    ins = d['instructions']
    order, key, cluster = schedule(ins, cfg)
    assert np.array_equal(order, np.arange(len(ins))) and np.array_equal(key, ins['time'])
    starts = np.concatenate([[0], np.flatnonzero(np.diff(cluster)) + 1])
    assert starts.tolist() == d['dec_first'].tolist()
    flushed = set(d['flush_at_call'][:-1].tolist())
    assert flushed <= set(starts.tolist())
    run, verdicts = None, []
    for c, k0 in enumerate(starts):
        k1 = starts[c + 1] if c + 1 < len(starts) else len(ins)
        verdicts.append(run is not None and int(key[k0:k1].min()) - run > rext)
        a, b = int(d['call_pulse_off'][k0]), int(d['call_pulse_off'][k1])
        if b > a:
            e = int(d['pl_right'][a:b].max()) * dt
            run = e if run is None else max(run, e)
    assert [int(k) for k, v in zip(starts, verdicts) if v] == sorted(flushed)
