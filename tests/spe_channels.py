"""Per-channel SPE rows: the designed distributions behind tests/golden/spe_channels.npz (make_golden.py spe_channels runs the reference
on them), the designed photon lists and the law every photon's gain must obey.  Shared by make_golden.py,
tests/test_spe_channels_reference.py and tests/test_gpu_spe_channels.py.  No test lives here.

A real SPE file has one column per PMT and Pulse.uniform_to_pe_arr(p, channel) reads row `channel` of a [n_columns, 2001] table
(pulse.py:189-227); the bundled configuration ships ONE shared column, so nothing else ever ran the row lookup.  Two families, both
on the bundled charge axis (1099 bins, 999 of them with positive charge):

  delta    column c has all its mass in ONE bin, a different bin for every column, every charge positive: row c of the table is constant
           from index 1 on, so the gain of every photon NAMES the row it was read from, whatever uniform was drawn.  Bins are
           scrambled (c -> 142 + 37 c mod 900), so neighbours in c, c +- 64 and c +- 256 lie far apart in charge.  Special columns:
           ZERO_CH all zero (the reference's dummy axes: gain 0), FIRST_CH all mass in the first positive bin, LAST_CH all mass in the
           last bin of the axis (the fill_value ends of interp1d); DEAD_CH is an ordinary column on a PMT with gains == 0.
  shaped   column c is the bundled pdf rolled by c mod 7 - 3 bins, raised to a power set by c mod 11 and tilted by c mod 13, in whole numbers: full step
           functions, pairwise distinct (7 x 11 x 13 = 1001 > 500 columns) -- index and row offset are tested together, a stride of
           2000 or an index applied to another row changes the value.  ZERO_CH is all zero here as well.

The law (pulse.py:97-103): gain == G[c] * row[c][k] for some k >= 1 (the index is int(2000 u) + 1), and for a double PE the float sum of
two such terms.
"""
import os

import numpy as np

from tests import pulse_edges as PE

FAMILIES = ('delta', 'shaped')
N_TPC, N_GRID = 494, 2001
ZERO_CH, FIRST_CH, LAST_CH, DEAD_CH = 11, 12, 13, 7        # (all below 120: the nVeto configuration has them too; its channel 7 is dead anyway)
SPECIAL = (ZERO_CH, FIRST_CH, LAST_CH, DEAD_CH)
EDGE_CHANNELS = (0, 252, 253, 493)                         # first, last of the top array | first of the bottom array, last
N_WIDE = 500                                               # more columns than PMTs: n_spe > n_tpc
DELTA_FIRST_BIN, DELTA_STEP, DELTA_SPAN = 142, 37, 900


def charge_axis():
    """(charge, pdf) of the bundled single-channel distribution (mean SPE scaling factor 1)"""
    from wfsim_amd.config import DATA_DIR
    spe = np.load(os.path.join(DATA_DIR, 'spe_single_channel.npz'))
    return np.asarray(spe['charge'], dtype=np.float64), np.asarray(spe['pdf'], dtype=np.float64)


def delta_bin(c, charge):
    """the one bin of column c; -1: the all-zero column"""
    if c == ZERO_CH:
        return -1
    if c == FIRST_CH:
        return int(np.flatnonzero(charge > 0)[0])
    if c == LAST_CH:
        return len(charge) - 1
    return DELTA_FIRST_BIN + (DELTA_STEP * c) % DELTA_SPAN


def pdfs(family, n_columns=N_TPC):
    """f64[n_columns, n_bins]"""
    charge, pdf = charge_axis()
    out = np.zeros((n_columns, len(charge)))
    for c in range(n_columns):
        if family == 'delta':
            b = delta_bin(c, charge)
            if b >= 0:
                out[c, b] = 1.0
        elif c != ZERO_CH:
            x = np.roll(pdf, c % 7 - 3) ** (0.8 + 0.04 * (c % 11)) * (1.0 + (c % 13) / 13.0 * np.linspace(0.0, 1.0, len(charge)))
            out[c] = np.round(x / x.max() * 1e6)          # whole numbers: a CSV gives them back exactly, whatever parser reads it
    return out


def delta_values(n_columns=N_TPC, charge=None):
    """the charge every photon of column c gets under `delta` (charge: the axis the table was built on, default the bundled one)"""
    charge = charge_axis()[0] if charge is None else np.asarray(charge)
    b = np.array([delta_bin(c, charge) for c in range(n_columns)])
    return np.where(b >= 0, charge[np.maximum(b, 0)], 0.0)


def assert_design(family, p, table=None, charge=None):
    """what the families promise, on the pdfs (and on a table built from them on the axis `charge`)"""
    charge = charge_axis()[0] if charge is None else np.asarray(charge)
    n = len(p)
    assert len({row.tobytes() for row in p}) == n, 'columns pairwise distinct'
    assert not p[ZERO_CH].any() and all(p[c].any() for c in range(n) if c != ZERO_CH)
    if family == 'delta':
        v = delta_values(n, charge)
        assert np.all((p > 0).sum(axis=1) == (np.arange(n) != ZERO_CH)) and np.all(v[np.arange(n) != ZERO_CH] > 0)
        assert len(set(v.tolist())) == n                                      # a value names its column (0.0: the all-zero one)
        assert p[FIRST_CH, :np.flatnonzero(charge > 0)[0]].sum() == 0 and charge[np.flatnonzero(charge > 0)[0] - 1] <= 0 and p[LAST_CH, -1] == 1
        ordinary = [c for c in range(n) if c not in (ZERO_CH, FIRST_CH, LAST_CH)]
        assert all(0.3 < v[c] < 7.0 for c in ordinary) and all(c in ordinary for c in EDGE_CHANNELS + (DEAD_CH,))
        for c in range(n):
            for o in (1, 64, 256):
                for q in (c - o, c + o):
                    if 0 <= q < n and c in ordinary and q in ordinary:
                        assert abs(v[c] - v[q]) > 0.1, (c, q)          # (bins 37, 568 and 472 apart, 0.0072 a bin)
    if table is not None:
        assert table.shape == (n, N_GRID) and len({row[1:].tobytes() for row in table}) == n, 'rows pairwise distinct'
        assert not table[ZERO_CH].any()
        if family == 'delta':
            assert np.all(table[:, 1:] == delta_values(n, charge)[:, None])
        else:
            assert all(len(np.unique(table[c, 1:])) > 100 for c in range(n) if c != ZERO_CH)          # full step functions
            assert all(not np.array_equal(table[c, 1:2001], table[c + 1, 0:2000]) for c in range(n - 1))


def as_dict(family, n_columns=N_TPC, charge=None):
    """charge: the axis as a CSV reader gave it back (pandas' default parser is off by an ulp on a few bins of the bundled axis), for
    comparisons with a table built from a CSV"""
    return dict(charge=charge_axis()[0] if charge is None else np.asarray(charge, dtype=np.float64), pdfs=pdfs(family, n_columns), n_channels=n_columns)


def write_csv(family, path, n_columns=N_TPC):
    """the form of a real SPE file: 'charge' and one column per PMT, named by its number"""
    import pandas as pd
    p = pdfs(family, n_columns)
    cols = {'charge': charge_axis()[0]}
    cols.update({str(c): p[c] for c in range(n_columns)})
    pd.DataFrame(cols).to_csv(path, index=False)
    return path


def gains(n_channels=N_TPC):
    """non-uniform gains, so that a gain read for another channel shows as well; DEAD_CH is turned off"""
    c = np.arange(n_channels)
    g = np.round(2.0e6 * (0.8 + 0.4 * ((29 * c) % 97) / 97.0))
    g[DEAD_CH] = 0.0
    return g


def config(family, n_columns=N_TPC, base=None, **overrides):
    """the bundled configuration (or `base`) with the family's columns as dict(charge=, pdfs=) and the gains above"""
    from wfsim_amd.config import xenonnt_test_config
    c = dict(base) if base is not None else xenonnt_test_config()
    n = len(c['gains'])
    c.update(gains=gains(n), photon_area_distribution=as_dict(family, n_columns))
    c.update(overrides)
    return c


# ---------------------------------------------------------------------------------------------------------------- the law
class Law:
    """gain == G[c] row[c][k], k >= 1; double PE: the float sum of two such terms"""

    def __init__(self, table, gains):
        self.table, self.gains = np.asarray(table), np.asarray(gains, dtype=np.float64)
        self._single, self._double = {}, {}

    def single(self, c):
        if c not in self._single:
            self._single[c] = np.unique(self.gains[c] * self.table[c, 1:])
        return self._single[c]

    def double(self, c):
        if c not in self._double:
            s = self.single(c)
            self._double[c] = np.unique(s[:, None] + s[None, :])
        return self._double[c]

    def violations(self, ch, dpe, gain):
        """indices of the photons that break the law (photons on turned-off PMTs carry no gain: whatever is stored must be 0)"""
        ch, dpe, gain = np.asarray(ch), np.asarray(dpe).astype(bool), np.asarray(gain)
        ok = np.zeros(len(ch), dtype=bool)
        for c in np.unique(ch):
            m = ch == c
            if self.gains[c] == 0:
                ok[m] = gain[m] == 0
                continue
            ok[m & ~dpe] = np.isin(gain[m & ~dpe], self.single(int(c)))
            if (m & dpe).any():
                ok[m & dpe] = np.isin(gain[m & dpe], self.double(int(c)))
        return np.flatnonzero(~ok)

    def area(self, ch, gain, channels=None):
        """sum of gain / G over the photons of live PMTs (of `channels`): raw_area (pulse.py:256)"""
        ch, gain = np.asarray(ch), np.asarray(gain)
        m = self.gains[ch] > 0
        if channels is not None:
            m &= np.isin(ch, channels)
        return float(np.sum(gain[m] / self.gains[ch[m]]))


# ---------------------------------------------------------------------------------------------------------------- reference calls
GROUPS = ('all_channels', 'double_pe')
P_DPE_HIGH = 0.6


def reference_cases(n_channels=N_TPC, dt=10):
    """the Pulse calls of the fixture, as tests/pulse_edges.py lists its cases (tiles: (times, None, channel), sorted by channel; the
    gains are the reference's to draw).  Group all_channels: 3 photons on every channel, then 60 on each special column and edge
    channel; group double_pe: p_double_pe_emision = P_DPE_HIGH, 60 photons on the same channels and 8 on every 7th other one."""
    rng = np.random.default_rng(4301)
    marked = sorted(SPECIAL + EDGE_CHANNELS)
    cases = []
    t0 = PE.GROUP_SPACING
    cases.append(dict(name='every_channel', group=0, p_dpe=None, set_tmin=t0,
                      tiles=[(PE.spread(rng, 3, 3, dt, t0), None, c) for c in range(n_channels)]))
    t1 = t0 + 4000
    cases.append(dict(name='marked_channels', group=0, p_dpe=None, set_tmin=t1,
                      tiles=[(PE.spread(rng, 60, 20, dt, t1), None, c) for c in marked]))
    t2 = 2 * PE.GROUP_SPACING
    chans = sorted(set(marked) | set(range(3, n_channels, 7)))
    cases.append(dict(name='double_pe', group=1, p_dpe=P_DPE_HIGH, set_tmin=t2,
                      tiles=[(PE.spread(rng, 60 if c in marked else 8, 12, dt, t2), None, c) for c in chans]))
    return cases


# ---------------------------------------------------------------------------------------------------------------- supplied photons
# per-channel photon lists from the class table of tests/pulse_edges.py: (photons, start bins) on both sides of every class boundary,
# one group per kernel (the dense and sparse kernels are chosen from batch maxima, so a group is a batch of its own)
SUPPLIED_GROUPS = dict(
    tiny=[(4, 32)],
    sparse=[(5, 32), (32, 64)],
    wave=[(33, 64), (64, 16384)],
    dense_128_res=[(65, 2), (1024, 107)],
    dense_256_res=[(400, 236)],
    dense_128_win=[(1025, 107)],
    dense_256_win=[(2049, 236)],
)
DENSE_VARIANT = dict(dense_128_res=(128, True), dense_256_res=(256, True), dense_128_win=(128, False), dense_256_win=(256, False))


def supplied_channels(n_channels=N_TPC):
    """the channels every supplied-photon case hits: first and last, both sides of the top | bottom boundary (or the middle), the
    special columns, and c, c + 1, c + 64, c + 256 of one ordinary channel where they exist"""
    mid = 252 if n_channels == N_TPC else n_channels // 2 - 1
    ch = [0, n_channels - 1, mid, mid + 1, ZERO_CH, FIRST_CH, LAST_CH, DEAD_CH, 30, 31, 94]
    if n_channels > 286:
        ch.append(286)
    return sorted(ch)


def supplied_photons(group, n_channels=N_TPC, dt=10, time=1_000_000):
    """one optical instruction (time, channels[], timings[] relative to it, in ns) whose tiles have the shapes of `group`, the shapes
    handed out to supplied_channels() in turn; returns (channels, timings, {channel: shape})"""
    rng = np.random.default_rng(4400 + sorted(SUPPLIED_GROUPS).index(group))
    shapes = SUPPLIED_GROUPS[group]
    ch, tt, shape_of = [], [], {}
    for i, c in enumerate(supplied_channels(n_channels)):
        n, nb = shapes[i % len(shapes)]
        t = PE.spread(rng, n, nb, dt, time) - time
        ch.append(np.full(n, c, dtype=np.int32)); tt.append(t.astype(np.int64)); shape_of[c] = (n, nb)
    return np.concatenate(ch), np.concatenate(tt), shape_of


def tile_shapes(set_off, t, ch, dt):
    """per pulse set {channel: (photons, start bins)} from a photon list"""
    out = []
    for a, b in zip(set_off[:-1], set_off[1:]):
        d = {}
        for c in np.unique(ch[a:b]):
            x = t[a:b][ch[a:b] == c]
            d[int(c)] = (len(x), int(x.max() // dt - x.min() // dt + 1))
        out.append(d)
    return out
