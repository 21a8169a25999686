"""Full readout (config 'full_readout', wfs_set_full_readout) pinned on the unchanged oracle; a helper, not a test.

The oracle, like the reference, digitises a window only on the channels that hold a pulse.  A photon of gain 0 adds a current of exactly
0 but makes a pulse, and thereby a masked row: give the oracle, on every TPC channel of every window, two such photons at the times of
the window's earliest and latest photon, and every row slot has a row of the window's union range while dg_left / dg_right, the
ix_rand draw and every sample with a pulse stay what they were (``with_anchors``).  The oracle's records for that input are the
engine's records in full-readout mode on the original input.  (The HE rows follow their top channels in the oracle, whatever the HE
factor; the engine has them when they can differ from a flat baseline.)
"""
import numpy as np

from tests import noise_slow as NS
from tests.noise_model import oracle_rows
from tests.test_gpu_noise_model import MS, T34, _designed_windows, _off_config, _oracle_photons, _photon_sets, _table_config

ZLE_ADC = 15                    # zle_threshold of the bundled configuration: a sample 16 ADC counts below the baseline is a hit
LOUD = tuple(range(20, 32)) + tuple(range(300, 312))        # channels with sigma around 5: their pulse-less rows reach the threshold
QUIET = 3                       # sigma 0: a flat row


def sigmas(n):
    """a few channels around 5 ADC counts (LOUD), one with 0 (QUIET), the rest near 2: rows of the last kind never reach the threshold
    (16 / 2.3 = 7 sigma), a row of 270 samples of the first kind does in about two cases of five"""
    s = np.random.default_rng(11).uniform(1.7, 2.3, n)
    loud = [c for c in LOUD if c < n]
    s[loud] = np.random.default_rng(12).uniform(5.0, 6.0, len(loud))
    s[QUIET] = 0.0
    return s


def windows_of(p):
    """the nine designed windows of tests/test_gpu_noise_model.py and one whose union range is 256 samples"""
    n_top, dt, tw = int(p['n_top']), int(p['dt']), int(p['trigger_window'])
    per = int(p['store_before'] + p['samples_before'] + p['store_after'] + p['samples_after']) + 1 + 2 * tw
    w = _designed_windows(p)
    w.insert(7, (80 * MS, [(n_top + 4, [400, 400 + dt * (256 - per)], 1.0), (16, [420], 1.0)]))
    return w


def extremes(window):
    """absolute times of the window's earliest and latest photon"""
    base, entries = window
    t = np.concatenate([np.asarray(times, dtype=np.int64) for _, times, _ in entries])
    return int(base) + int(t.min()), int(base) + int(t.max())


def with_anchors(calls, windows, n_tpc, first_set):
    """calls of _photon_sets with one more Pulse call per (window, TPC channel): two photons of gain 0 at the window's extremes"""
    out, k = [], first_set
    for w, window in enumerate(calls):
        tt = np.array(extremes(windows[w]), dtype=np.int64)
        out.append(list(window) + [(k + c, tt, c, 0.0) for c in range(n_tpc)])
        k += n_tpc
    return out


def photon_input(cfg, p, windows):
    gains = np.asarray(cfg['gains'], dtype=np.float64)
    sets, calls = _photon_sets(windows, gains)
    return sets, calls, with_anchors(calls, windows, int(p['n_tpc']), len(sets[0]))


def pulse_less(o_plain, o_full):
    """rows of the anchored run that the plain run does not have, as (window, channel, first absolute sample, length)"""
    have = {(w, ch) for w, ch, _, _ in oracle_rows(o_plain)}
    return [r for r in oracle_rows(o_full) if (r[0], r[1]) not in have]


def model_expectation(cfg, model, seed, calls, anchored, extra_rows=()):
    """The anchored oracle on the model's values: the full rows of a noise-free anchored run (and ``extra_rows``, the sum rows of the
    plain run) are materialised into a table with one stretch per window (tests/noise_slow.py), which the oracle replays.
    Returns (oracle, table config, ix_rand per window, full rows)."""
    off = _oracle_photons(_off_config(cfg), anchored)
    o_off = off.results()
    rows = oracle_rows(o_off)
    table, ix = NS.materialise_slow(rows + list(extra_rows), len(o_off['dg_left']), model, seed)
    tab_cfg = _table_config(cfg, table)
    return _oracle_photons(tab_cfg, anchored, ix), tab_cfg, ix, rows


def replay(orc, o, n_tpc=0, gains=None):
    """Feeds ``orc`` the Pulse calls of a finished oracle run ``o`` (its photons with their drawn gains, which are the device's own:
    the callers compare them) and digitises where that run did; with n_tpc > 0 every window gets its anchors first -- one call, two
    photons of gain 0 on every TPC channel at the window's earliest and latest photon (photons on a dead PMT make no pulse and do
    not count).  Returns the oracle."""
    ends = (o['dg_first_pulse'] + o['dg_n_pulses']).tolist()
    off = o['call_ph_off']
    assert off[0] == 0 and len(off) == len(o['call_kind']) + 1
    live = np.ones(1 << 15, dtype=bool) if gains is None else np.concatenate([np.asarray(gains) > 0, np.ones((1 << 15) - len(gains), dtype=bool)])
    w, extra, lo, hi = 0, 0, None, None
    for k in range(len(o['call_kind'])):
        a, b = int(off[k]), int(off[k + 1])
        t, ch = o['ph_t'][a:b], o['ph_ch'][a:b]
        orc.pulse_call(int(o['call_kind'][k]), int(o['call_runset'][k]), t, ch, o['ph_dpe'][a:b], o['ph_gain'][a:b], True)
        tl = t[live[ch]]
        if len(tl):
            lo, hi = (int(tl.min()), int(tl.max())) if lo is None else (min(lo, int(tl.min())), max(hi, int(tl.max())))
        if w < len(ends) and len(orc.get('pl_ch')) - extra == ends[w]:
            if n_tpc:
                before = len(orc.get('pl_ch'))
                orc.pulse_call(0, 0, np.tile([lo, hi], n_tpc), np.repeat(np.arange(n_tpc), 2).astype(np.int16), np.zeros(2 * n_tpc, np.uint8), np.zeros(2 * n_tpc), True)
                extra += len(orc.get('pl_ch')) - before
            orc.digitize_and_zle(0)
            w, lo, hi = w + 1, None, None
    assert w == len(ends)
    return orc


def reassemble(rec, channel):
    """{first absolute sample: int64 samples} of every interval of a channel, from its record fragments"""
    r = rec[rec['channel'] == channel]
    r = r[np.lexsort((r['record_i'], r['time']))]
    out, k = {}, 0
    while k < len(r):
        assert r['record_i'][k] == 0
        plen, dt = int(r['pulse_length'][k]), int(r['dt'][k])
        n = (plen + 109) // 110
        frag = r[k:k + n]
        assert np.array_equal(frag['record_i'], np.arange(n)) and np.array_equal(frag['time'], r['time'][k] + dt * 110 * np.arange(n))
        data = np.concatenate([f['data'][:f['length']] for f in frag]).astype(np.int64)
        assert len(data) == plen
        out[int(r['time'][k]) // dt] = data
        k += n
    return out


__all__ = ['LOUD', 'MS', 'QUIET', 'T34', 'ZLE_ADC', 'extremes', 'model_expectation', 'photon_input', 'pulse_less', 'reassemble', 'replay', 'sigmas',
           'windows_of', 'with_anchors']
