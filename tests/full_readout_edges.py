"""Full readout on the designed rows of tests/golden/zle_edges.npz; a helper, not a test.  Shared by
tests/test_full_readout_edges_cpu.py and tests/test_gpu_full_readout_edges.py.

A designed row of the fixture is a pair of photons of gain 1 -- their pulse rounds to 0 ADC counts everywhere -- plus spikes in the
channel's column of the noise table: the row is noise, baseline and clamp.  Move the pair to another channel whose column is all zero
(the CARRIER) and the case channel has no pulse; in full-readout mode it still has a row of the same range, the same ix_rand and the
same table column, so the reference's finished row, its ZLE tuples and its record bytes are what the engine must give -- from
k_row_empty.  Per family one batch with ONE digitise window per case, in two forms:
  * 'transposed': the weak pair sits on the carrier (at the case's earliest and latest weak photon), the case's real photons
    (pulse_peak_*, clamp_pulse_*, he_huge_pulse_*) stay on the case channel: every case without a real photon is a row without a pulse
  * 'widened': as above, and the case channel gets two weak photons in one bin in the middle of the range: its row has a tile shorter
    than the row that begins behind the row's first sample (k_rows_widen, then the accumulator or the resident kernels)
The other cases' columns lie inside every window too: their pulse-less rows have hits and records of their own, which the anchored
oracle (tests/full_readout.py: with_anchors) pins with the rest of the batch.
"""
import numpy as np

from tests import full_readout as FR
from tests import zle_edges as ZE
from tests.test_gpu_noise_model import _photon_sets
from tests.test_zle_edges_reference import fixture
from wfsim_amd.config import kernel_params

FORMS = ('transposed', 'widened')
N_CASES = 481                   # over all families
N_CASE_RECORDS = 2499           # the reference's records of every case channel and its HE channel, over all families


def carrier_of(name):
    """the family's carrier: the last bottom channel that is on no case, has no special threshold, a live PMT and an all-zero column"""
    a, cfg, fam, rows, index = fixture(name)
    table, gains = cfg['noise_data'], np.asarray(cfg['gains'], dtype=np.float64)
    used = {c['channel'] for c in fam.cases}
    n_tpc = int(kernel_params(cfg)['n_tpc'])
    for ch in range(n_tpc - 1, ZE.FIRST_BOTTOM - 1, -1):
        if ch not in used and ch not in fam.special and gains[ch] > 0 and not table[:, ch].any():
            return ch
    raise AssertionError(f'{name}: no bottom channel is free to carry the weak pairs')


def _subset_tuples(a, window, channels):
    """the reference's ZLE tuples of one window on the given channels, in the order it yielded them, as expected_records reads them"""
    keep = np.flatnonzero((a['zle_digit'] == window) & np.isin(a['zle_ch'], channels))
    off = a['zle_data_off']
    data = [a['zle_data'][off[k]:off[k + 1]] for k in keep]
    return dict(zle_left=a['zle_left'][keep], zle_right=a['zle_right'][keep], zle_ch=a['zle_ch'][keep],
                zle_data_off=np.concatenate([[0], np.cumsum([len(x) for x in data])]).astype(np.int64),
                zle_data=np.concatenate(data) if data else np.zeros(0, dtype=a['zle_data'].dtype))


_batches = {}


def batch(name, form):
    """The batch of one family in one form: dict(
         cfg, p, fam, carrier,
         cases: per case dict(case, offset (ns, of the new window against the original one), ix_rand, real (has a real photon),
                lo / hi (the window's time range in ns, for picking its records), rows ({channel: (absolute first sample, reference row)}
                of the case channel and its HE channel, shifted), expected (the reference's records of both, time shifted)),
         sets: the load_photons arguments of the input, calls / anchored: the oracle's calls without / with the anchors,
         ix: the ix_rand of every window)"""
    assert form in FORMS
    if (name, form) in _batches:
        return _batches[(name, form)]
    a, cfg, fam, rows, index = fixture(name)
    p = kernel_params(cfg)
    dt, n_tpc = int(p['dt']), int(p['n_tpc'])
    carrier = carrier_of(name)
    assert list(a['call_case']) == list(range(len(fam.cases)))         # one Pulse call per case, in case order
    off = a['call_ph_off']
    windows, cases = [], []
    for k, case in enumerate(fam.cases):
        w, ch = case['window'], case['channel']
        t, g = a['ph_t'][off[k]:off[k + 1]].astype(np.int64), a['ph_gain'][off[k]:off[k + 1]].astype(np.float64)
        assert np.all(a['ph_ch'][off[k]:off[k + 1]] == ch) and np.array_equal(np.sort(t), np.sort(case['times']))
        bins = ZE.GROUP_SPACING * (k + 1) // dt - ZE.GROUP_SPACING * (w + 1) // dt          # (the case's own shift stays in its times)
        assert bins % 2 == 0
        offset = bins * dt
        weak = g == ZE.WEAK_GAIN
        assert weak.sum() == 2 and np.all(g[~weak] > ZE.WEAK_GAIN)
        lo, hi = int(t[weak].min()), int(t[weak].max())
        assert lo <= t.min() and t.max() <= hi and lo // dt == fam.windows[w]['b0'] + case['shift']
        entries = [(carrier, [lo, hi], ZE.WEAK_GAIN)] + [(ch, [int(x)], float(y)) for x, y in zip(t[~weak], g[~weak])]
        if form == 'widened':
            mid = (lo // dt + (hi // dt - lo // dt) // 2) * dt
            entries.append((ch, [mid, mid], ZE.WEAK_GAIN))
        windows.append((offset, entries))
        he = fam.he_first + ch
        own = {c: (rows[index[(w, c)]]['abs'] + bins, rows[index[(w, c)]]) for c in (ch, he) if (w, c) in index}
        exp = ZE.expected_records(_subset_tuples(a, w, [ch, he]), dt)
        exp['time'] += offset
        centre = ZE.GROUP_SPACING * (k + 1)
        cases.append(dict(case=case, offset=offset, ix_rand=int(a['dg_ix_rand'][w]), real=bool((~weak).any()), rows=own, expected=exp,
                          lo=centre - ZE.GROUP_SPACING // 2, hi=centre + ZE.GROUP_SPACING // 2))
    sets, calls = _photon_sets(windows, np.ones(n_tpc))             # (absolute gains: the factor of a live PMT of gain 1)
    anchored = FR.with_anchors(calls, windows, n_tpc, len(sets[0]))
    out = dict(name=name, form=form, cfg=cfg, p=p, fam=fam, carrier=carrier, cases=cases, windows=windows, sets=sets, calls=calls, anchored=anchored,
               ix=np.array([c['ix_rand'] for c in cases], dtype=np.int64))
    _batches[(name, form)] = out
    return out


def case_records(rec, b, k):
    """the records of case k's channel and HE channel in its window, out of the records of the whole batch (in the batch's order)"""
    c = b['cases'][k]
    ch = c['case']['channel']
    return rec[(rec['time'] >= c['lo']) & (rec['time'] < c['hi']) & ((rec['channel'] == ch) | (rec['channel'] == b['fam'].he_first + ch))]


def assert_case_records(rec, b, what=''):
    """THE comparison of the CPU and the GPU tests: for every case of the batch the records of its channel and its HE channel in its
    window are the reference's, byte for byte.  ``rec``: the records of the whole batch (unsorted: window by window, rows in channel
    order).  Returns the number of records compared."""
    n = 0
    for k, c in enumerate(b['cases']):
        got, exp = case_records(rec, b, k), c['expected']
        assert len(got) == len(exp), (what, b['name'], b['form'], c['case']['name'], len(got), len(exp))
        if got.tobytes() != exp.tobytes():
            j = int(np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(got, exp)])[0])
            raise AssertionError(f'{what} {b["name"]} / {b["form"]}: case {c["case"]["name"]}: record {j} differs (channel {exp["channel"][j]}, fragment '
                                 f'{exp["record_i"][j]} of a pulse of {exp["pulse_length"][j]} at sample {(exp["time"][j] - c["offset"]) // int(exp["dt"][j])})')
        n += len(exp)
    return n


def designed_window(c):
    """(dg_left, dg_right) of a case's window: the case row's range, the left end moved down to an even sample (rawdata.py:358-361)"""
    first, row = c['rows'][c['case']['channel']]
    return first - first % 2, first + len(row['data']) - 1
