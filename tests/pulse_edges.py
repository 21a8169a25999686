"""Designed edge photon lists for the pulse kernels: the case table behind tests/golden/pulse_edges.npz and pulse_edges_geometry.npz
(make_golden.py pulse_edges runs the reference on them), exact rational currents with their forward error bound, and what the
tests read back from the fixtures.  Shared by make_golden.py, tests/test_pulse_edges_reference.py and tests/test_gpu_pulse_edges.py.

A CASE is one Pulse.__call__ (one pulse set) on a few channels; a tile is its photons on one channel.  A GROUP is the set of cases that
share one digitise window; groups are the replay units of the GPU tests (the dense and sparse kernels are chosen from batch maxima).
"""
from fractions import Fraction

import numpy as np

# The dispatch constants of the HIP path, mirrored HERE and nowhere else in the tests: wfsim_amd/csrc/wfs_kernels.h:149-157 (tile classes,
# RES_SHORT_LEN), DENSE_PPT (wfs_kernels.h), and the dispatch after k_tile_desc in wfs_engine.hip (128 / 256 threads by live samples,
# resident photons up to threads x DENSE_PPT, NWIN_MAX windows, tap_sparse_max, res_max_len).
TINY_MAX_PHOTONS, TINY_MAX_BINS = 4, 32
SPARSE_MAX_PHOTONS, SPARSE_MAX_BINS = 32, 64
WAVE_MAX_PHOTONS, WAVE_MAX_BINS = 64, 16384
DENSE_PPT = 8
NWIN_MAX = 8
TAP_SPARSE_MAX = 48
RES_SHORT_LEN = 768
RES_SEGMENT = 1024          # res_max_len; WFS_RES_MAX_LEN=256 selects the 256-sample segment
KERNEL_OF_CLASS = dict(tiny='k_pulse_tiny', sparse='k_pulse_sparse', wave='k_pulse_wave', dense='k_pulse_dense')
TILE_KERNELS = set(KERNEL_OF_CLASS.values()) | {'k_pulse_generic'}

GROUP_SPACING = 10_000_000          # ns between groups: far above right_raw_extension plus the longest designed pulse
EPOCH = 1_700_000_000_000_000_007   # 1.7e18 + 7 ns


def tile_class(n, nb):
    if n <= TINY_MAX_PHOTONS and nb <= TINY_MAX_BINS:
        return 'tiny'
    if n <= SPARSE_MAX_PHOTONS and nb <= SPARSE_MAX_BINS:
        return 'sparse'
    if n <= WAVE_MAX_PHOTONS and nb <= WAVE_MAX_BINS:
        return 'wave'
    return 'dense'


def dense_variant(max_nb, max_photons, tlen=22):
    """(threads, photons resident in registers, windows per tile) of the k_pulse_dense instantiation a batch with these maxima gets"""
    live = max_nb + tlen - 1
    tpb = 128 if live <= 128 else 256
    resident = max_photons <= tpb * DENSE_PPT
    n_win = 1 if resident else min(NWIN_MAX, max(1, -(-live // tpb)))
    return tpb, resident, n_win


# ---------------------------------------------------------------------------------------------------------------- the cases
def spread(rng, n, nb, dt, t0):
    """n photon times over exactly nb start bins from the bin of t0 (a multiple of dt): the first and the last photon fix the bin
    count, the ns remainders cycle through all dt values, the order inside the tile is shuffled"""
    assert n >= (2 if nb > 1 else 1)
    bins = np.zeros(n, dtype=np.int64)
    if n > 1:
        bins[-1] = nb - 1
        bins[1:-1] = rng.integers(0, nb, n - 2)
    t = t0 + bins * dt + np.arange(n) % dt
    return t[rng.permutation(n)]


class Builder:
    """collects cases; channels are handed out one per tile (across the top / bottom array boundary) unless a case names one"""

    def __init__(self, dt, n_channels=494, first_channel=240):
        self.dt, self.cases, self.groups = dt, [], []
        self.n_channels, self.first_channel = n_channels, first_channel
        self._next = first_channel

    def group(self, name, t0=None):
        self.groups.append(name)
        self._next = self.first_channel
        self.t0 = GROUP_SPACING * len(self.groups) if t0 is None else t0
        return self.t0

    def channel(self):
        c = self._next
        self._next += 1
        assert c < self.n_channels
        return c

    def case(self, name, tiles, set_tmin=None, expect=None):
        """tiles: list of (times, gains or None, channel or None); gains None: drawn by the generator (uniform 1e6 .. 3e6, redrawn with
        the next seed when a sample comes near a rounding tie); a callable gains(rng, times) draws designed ones the same way; an array
        gives them as they are"""
        out = []
        for t, g, ch in tiles:
            out.append((np.asarray(t, dtype=np.int64), g, self.channel() if ch is None else ch))
        out.sort(key=lambda x: x[2])
        tmin = min(int(t.min()) for t, _, _ in out)
        self.cases.append(dict(name=name, group=len(self.groups) - 1, tiles=out, set_tmin=tmin if set_tmin is None else set_tmin,
                               expect=expect or {}))


def _gain_range(rng, t):
    return 10.0 ** np.linspace(3, 9, len(t)) * rng.uniform(1.0, 1.5, len(t))


def _huge(rng, t):
    return 2e9 * rng.uniform(0.8, 1.2, len(t))


def _negative(rng, t):
    return -rng.uniform(1e6, 3e6, len(t))


def _truth_sides(thr_gain, dt):
    """gains on both sides of the truth trigger threshold (pulse.py:252-253), alternating, 10 .. 30 % away from it; thr_gain[r]: the
    gain at which a photon in ns remainder r reaches it"""
    def f(rng, t):
        side = np.where(np.arange(len(t)) % 2 == 0, 1.0, -1.0)
        return np.asarray(thr_gain)[np.asarray(t) % dt] * (1.0 + side * rng.uniform(0.1, 0.3, len(t)))
    return f


def _tap_cells(rng, n_cells, n_photons, dt, t0):
    """n_photons photons on exactly n_cells distinct (start bin, ns) cells of 42 start bins, few of them in the middle of the reach of
    the wave (where tap_block looks first): 64 live samples, one wave"""
    lo = [(b, r) for b in range(0, 9) for r in range(dt)]
    mid = [(b, r) for b in range(10, 36) for r in range(dt)]
    hi = [(b, r) for b in range(37, 42) for r in range(dt)]
    n_mid = 8
    n_lo = (n_cells - n_mid) // 2
    n_hi = n_cells - n_mid - n_lo
    cells = [(0, 0), (41, dt - 1)]
    for pool, k in ((lo[1:], n_lo - 1), (mid, n_mid), (hi[:-1], n_hi - 1)):
        cells += [pool[i] for i in rng.choice(len(pool), k, replace=False)]
    assert len(set(cells)) == n_cells
    pick = np.concatenate([np.arange(n_cells), rng.integers(0, n_cells, n_photons - n_cells)])
    t = np.array([t0 + cells[i][0] * dt + cells[i][1] for i in pick], dtype=np.int64)
    return t[rng.permutation(len(t))]


def common_cases(b, rng, thr_gain, ties, prefix=''):
    """sections d, e, g of the case list: both fixtures.  ties: {'even' / 'odd': (k, gain, ns remainder)} -- single photons whose gain
    the generator searched so that the peak sample of the pulse is exactly k + 0.5 ADC counts"""
    dt = b.dt
    # ---- d: time structure
    t0 = b.group(prefix + 'neg_time', t0=0)
    b.case('d_negative_times', [(np.array([-37, -31, -5, 0, 3, 9, 10]), None, None)], expect=dict(negative=True))
    b.group(prefix + 'time')
    t0 = b.t0
    b.case('d_2_in_one_ns', [(np.array([t0 + 13, t0 + 13, t0 + 4 * dt + 1]), None, None)], expect=dict(max_per_ns=2))
    b.case('d_3_in_one_ns', [(np.array([t0 + 17, t0 + 17, t0 + 17, t0 + 3 * dt]), None, None)], expect=dict(max_per_ns=3))
    b.case('d_40_in_one_ns', [(np.full(40, t0 + 2 * dt + 3), None, None)], expect=dict(max_per_ns=40))
    b.case('d_all_remainders', [(t0 + 5 * dt + rng.permutation(dt), None, None)], expect=dict(shape=(dt, 1)))
    b.case('d_tmin_not_on_a_sample', [(t0 + 3 + np.array([0, 8, 21, 39]), None, None)], set_tmin=t0 + 3, expect=dict(tmin_mod=3))
    b.case('d_before_set_tmin', [(t0 + 2000 + np.array([-1000, -993, -512, -1, 0, 7, 31]), None, None),
                                 (t0 + 2000 + np.array([-640, 12]), None, None)], set_tmin=t0 + 2000, expect=dict(before_tmin=1000))
    # ---- e: rounding and range
    b.group(prefix + 'ties')
    t0 = b.t0
    for kind in ('even', 'odd'):
        k, gain, rem = ties[kind]
        b.case('e_tie_' + kind, [(np.array([t0 + rem]), np.array([gain]), None)], expect=dict(tie=int(k)))
    b.case('e_negative_gain', [(np.array([t0 + 4]), _negative, None)])
    b.group(prefix + 'range')
    t0 = b.t0
    b.case('e_gain_range', [(spread(rng, 10, 5, dt, t0), _gain_range, None)])
    b.case('e_huge_gain_clamp_before_narrowing', [(spread(rng, 12, 3, dt, t0), _huge, None)], expect=dict(below_baseline=(1e5, 1e6)))
    # ---- g: truth threshold inside one tile, a tile of each class
    b.group(prefix + 'truth')
    t0 = b.t0
    for name, n, nb in [('tiny', 4, 3), ('sparse', 12, 20), ('wave', 50, 40), ('dense', 100, 30)]:
        b.case('g_truth_' + name, [(spread(rng, n, nb, dt, t0), _truth_sides(thr_gain, dt), None)], expect=dict(shape=(n, nb), truth_sides=True))
    return b


def main_cases(thr_gain, ties, dt=10):
    """the case list of pulse_edges.npz (bundled XENONnT configuration: 10 ns samples, 2 + 20 template samples, 50 + 50 stored, trigger
    window 50)"""
    rng = np.random.default_rng(4201)
    b = Builder(dt)
    common_cases(b, rng, thr_gain, ties)
    # ---- a: both sides of every class boundary, one group per class so that the group names its kernel
    a_cases = [((4, 32), 'tiny'), ((1, 1), 'tiny'), ((5, 32), 'sparse'), ((4, 33), 'sparse'), ((32, 64), 'sparse'), ((33, 64), 'wave'),
               ((32, 65), 'wave'), ((64, 16384), 'wave'), ((65, 2), 'dense'), ((64, 16385), 'dense')]
    for cls in ('tiny', 'sparse', 'wave', 'dense'):
        b.group('class_' + cls)
        for (n, nb), c in a_cases:
            if c == cls:
                b.case(f'a_{n}x{nb}_{cls}', [(spread(rng, n, nb, dt, b.t0), None, None)], expect=dict(shape=(n, nb), cls=cls))
        if cls == 'tiny':       # (2 and 3 photons in one ns once more, on the thread-per-tile kernel alone)
            b.case('d_3_in_one_ns_tiny', [(np.array([b.t0 + 8, b.t0 + 8, b.t0 + 8]), None, None)], expect=dict(max_per_ns=3, cls='tiny'))
        if cls == 'sparse':
            b.case('d_all_remainders_sparse', [(b.t0 + rng.permutation(dt), None, None)], expect=dict(shape=(dt, 1), cls='sparse'))
        if cls == 'wave':
            b.case('d_40_in_one_ns_wave', [(np.full(40, b.t0 + 9), None, None)], expect=dict(max_per_ns=40, cls='wave'))
    # ---- b: each k_pulse_dense instantiation in a batch of its own; c: the tap_block threshold
    b.group('dense_128_res')
    b.case('b_1024x107', [(spread(rng, 1024, 107, dt, b.t0), None, None), (spread(rng, 65, 2, dt, b.t0), None, None)],
           expect=dict(variant=(128, True)))
    for n_cells in (TAP_SPARSE_MAX - 1, TAP_SPARSE_MAX, TAP_SPARSE_MAX + 1):
        b.case(f'c_tap_{n_cells}_cells', [(_tap_cells(rng, n_cells, 70, dt, b.t0), None, None)], expect=dict(cells=n_cells, shape=(70, 42)))
    b.group('dense_256_res')
    b.case('b_2048x235', [(spread(rng, 2048, 235, dt, b.t0), None, None)], expect=dict(variant=(256, True), shape=(2048, 235)))
    b.case('b_400x236_400x237', [(spread(rng, 400, 236, dt, b.t0), None, None), (spread(rng, 400, 237, dt, b.t0), None, None)])
    core = b.t0 + 100 * dt + rng.integers(0, 30 * dt, 800)
    tails = spread(rng, 24, 230, dt, b.t0)
    b.case('c_tap_sparse_tails_dense_core', [(np.concatenate([core, tails]), None, None)], expect=dict(shape=(824, 230)))
    b.group('dense_128_win')
    b.case('b_1025x107', [(spread(rng, 1025, 107, dt, b.t0), None, None), (spread(rng, 200, 50, dt, b.t0), None, None)],
           expect=dict(variant=(128, False)))
    b.group('dense_256_win')
    b.case('b_2049x236', [(spread(rng, 2049, 236, dt, b.t0), None, None), (spread(rng, 300, 235, dt, b.t0), None, None),
                          (spread(rng, 300, 237, dt, b.t0), None, None)], expect=dict(variant=(256, False)))
    b.case('b_2049x2100_more_windows_than_NWIN_MAX', [(spread(rng, 2049, 2100, dt, b.t0), None, None)], expect=dict(shape=(2049, 2100)))
    b.case('e_saturation_2049_in_one_bin', [(b.t0 + 50 * dt + rng.integers(0, dt, 2049), None, None)], expect=dict(saturates=True))
    b.group('dense_256_win_one_chunk')          # more photons than the registers hold, live samples of one chunk: windows, n_win = 1
    b.case('b_2049x235_alone', [(spread(rng, 2049, 235, dt, b.t0), None, None)], expect=dict(variant=(256, False), shape=(2049, 235)))
    # ---- f: several tiles in one row
    b.group('overlap')
    ch = b.channel()
    for k, shift in enumerate([0, 30, 65, 210]):
        b.case(f'f_overlap_{k}', [(spread(rng, 10, 6, dt, b.t0) + shift, None, ch)], expect=dict(shared_row=True))
    b.group('row_lengths')
    for length in (RES_SHORT_LEN, RES_SHORT_LEN + 1, 1024, 1025):
        nb = length - 222           # 50 + 50 stored, 2 + 20 template samples, 2 x 50 trigger window
        b.case(f'f_row_of_{length}', [(spread(rng, 3, nb, dt, b.t0), None, None)], expect=dict(row_length=length))
    b.group('seams')
    ch = b.channel()
    L0 = b.t0 // dt - 102           # the row's left edge: the first pulse's left (start bin - 52) minus the trigger window
    # (name, photons, start bins, offset of the pulse's first / last sample from the row's left edge that is pinned)
    seam_tiles = [('first', 3, 2, ('left', 50)), ('ends_at_1023', 2, 2, ('right', 1023)), ('begins_at_1024', 9, 4, ('left', 1024)),
                  ('straddles_1280', 4, 3, ('left', 1280 - 60)), ('straddles_2048', 40, 12, ('left', 2048 - 70)),
                  ('ends_at_2559', 20, 8, ('right', 2559)), ('begins_at_2560', 1, 1, ('left', 2560)), ('last', 6, 5, ('right', 2999 - 50))]
    for name, n, nb, (side, off) in seam_tiles:
        first_bin = L0 + off + 52 if side == 'left' else L0 + off - 70 - (nb - 1)
        b.case('f_seam_' + name, [(spread(rng, n, nb, dt, first_bin * dt), None, ch)], expect=dict(seam=(side, off), shared_row=True))
    b.group('epoch', t0=EPOCH - 7)
    b.case('d_epoch_scale', [(EPOCH + np.array([0, 3, 14, 120]), None, None), (EPOCH + spread(rng, 20, 9, dt, 0), None, None)],
           set_tmin=EPOCH, expect=dict(epoch=True))
    return b


def geometry_cases(thr_gain, ties, dt=5):
    """the case list of pulse_edges_geometry.npz (chain I's geometry: 5 ns samples, 3 + 37 template samples): d, e, g again plus wide
    tiles -- every tile goes through k_pulse_generic, the class boundaries do not apply"""
    rng = np.random.default_rng(4202)
    b = Builder(dt)
    common_cases(b, rng, thr_gain, ties)
    b.group('wide')
    b.case('b_300x235_236_237', [(spread(rng, 300, nb, dt, b.t0), None, None) for nb in (235, 236, 237)])
    b.case('b_2049x236', [(spread(rng, 2049, 236, dt, b.t0), None, None)], expect=dict(shape=(2049, 236)))
    b.case('e_saturation_2049_in_one_bin', [(b.t0 + 50 * dt + rng.integers(0, dt, 2049), None, None)], expect=dict(saturates=True))
    b.group('epoch', t0=EPOCH - 7)
    b.case('d_epoch_scale', [(EPOCH + np.array([0, 3, 14, 120]), None, None)], set_tmin=EPOCH, expect=dict(epoch=True))
    return b


def truth_threshold_gain(current_max, current_2_adc, zle_threshold):
    """per ns remainder: the gain at which a photon reaches the truth trigger threshold (pulse.py:243, 252-253)"""
    return (zle_threshold - 0.5) / (np.asarray(current_max, dtype=np.float64) * float(current_2_adc))


def search_tie_gain(template_value, c2a, k, reach=4000):
    """a gain g with fl(fl(template_value * g) * c2a) == k + 0.5 exactly (numpy's expression, rawdata.py:236), or None: the doubles
    next to (k + 0.5) / (c2a * template_value) are scanned"""
    tv, c = np.float64(template_value), np.float64(c2a)
    g = np.float64((k + 0.5) / (c * tv))
    lo = hi = g
    for _ in range(reach):
        for x in (lo, hi):
            if (tv * x) * c == k + 0.5:
                return float(x)
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    return None


def find_ties(templates, c2a, rem=3):
    """{'even' / 'odd': (k, gain, ns remainder)}: the first even and odd k from 20 up for which a gain exists"""
    tv = float(np.max(np.asarray(templates)[rem]))
    out = {}
    for kind, k0 in (('even', 20), ('odd', 21)):
        for k in range(k0, k0 + 40, 2):
            g = search_tie_gain(tv, c2a, k)
            if g is not None:
                out[kind] = (k, g, rem)
                break
    return out


# ---------------------------------------------------------------------------------------------------------------- exact arithmetic
U = Fraction(1, 2 ** 53)


def gamma(m):
    return m * U / (1 - m * U)


def exact_tile(t, g, left, length, dt, TF):
    """Pulse.add_current in exact rational arithmetic.  Per sample of the pulse: the exact current, sum |template * gain| over the terms
    that reach it and their number n.  TF: the templates as Fractions, [remainder][sample]."""
    tlen = len(TF[0])
    cur, mag, n = [Fraction(0)] * length, [Fraction(0)] * length, [0] * length
    by_ns = {}
    for ti, gi in zip(np.asarray(t).tolist(), np.asarray(g).tolist()):
        e = by_ns.setdefault(ti, [Fraction(0), Fraction(0), 0])
        f = Fraction(gi)
        e[0] += f
        e[1] += abs(f)
        e[2] += 1
    for ns, (gs, ga, cnt) in by_ns.items():
        start, r = ns // dt - left, ns % dt
        row = TF[r]
        for k in range(tlen):
            s = start + k
            cur[s] += row[k] * gs
            mag[s] += abs(row[k]) * ga
            n[s] += cnt
    return cur, mag, n


def fixture_exact(d, templates, c2a, dt):
    """per pulse of a fixture: (exact currents, bound B on |computed current x c2a - exact x c2a|, distance of exact x c2a to the nearest
    half-integer) as lists over the samples; B = gamma(n + 1) x sum |term| x c2a (Higham, Accuracy and Stability of Numerical
    Algorithms, section 3.1: n + 1 roundings per term at most -- merging the gains of one ns, the product, the additions -- in ANY
    order, fused or not)"""
    TF = [[Fraction(float(x)) for x in row] for row in np.asarray(templates)]
    C = Fraction(float(c2a))
    half = Fraction(1, 2)
    out = []
    calls = np.repeat(np.arange(len(d['call_pulse_off']) - 1), np.diff(d['call_pulse_off']))
    for j in range(len(d['pl_ch'])):
        k = int(calls[j])
        a, b_ = int(d['call_ph_off'][k]), int(d['call_ph_off'][k + 1])
        m = d['ph_ch'][a:b_] == d['pl_ch'][j]
        left, length = int(d['pl_left'][j]), int(d['pl_right'][j] - d['pl_left'][j] + 1)
        cur, mag, n = exact_tile(d['ph_t'][a:b_][m], d['ph_gain'][a:b_][m], left, length, dt, TF)
        B = [gamma(n[s] + 1) * mag[s] * C if n[s] else Fraction(0) for s in range(length)]
        dist = []
        for s in range(length):
            if not n[s]:
                dist.append(None)
                continue
            v = cur[s] * C
            dist.append(abs(v - (v.__floor__() + half)))
        out.append(dict(cur=cur, B=B, dist=dist, n=n))
    return out


def near_ties(exact, skip=()):
    """(samples within 4 B of a rounding tie as (pulse, sample), smallest distance / B met elsewhere, smallest distance); skip: the
    designed exact ties"""
    bad, worst_ratio, worst = [], None, None
    for j, e in enumerate(exact):
        for s, (dist, B) in enumerate(zip(e['dist'], e['B'])):
            if dist is None or (j, s) in skip:
                continue
            if dist <= 4 * B:
                bad.append((j, s))
            if worst is None or dist < worst:
                worst = dist
            if B and (worst_ratio is None or dist / B < worst_ratio):
                worst_ratio = dist / B
    return bad, worst_ratio, worst


def currents_within_bound(cur, e, c2a):
    """largest |cur - exact| / (B / c2a) over the samples of one pulse (0 where no term reaches: the current must be 0.0 there)"""
    C = Fraction(float(c2a))
    worst = Fraction(0)
    for s, x in enumerate(np.asarray(cur).tolist()):
        if not e['n'][s]:
            if x != 0.0:
                return float('inf')
            continue
        err = abs(Fraction(x) - e['cur'][s])
        if err:
            if not e['B'][s]:
                return float('inf')
            worst = max(worst, err * C / e['B'][s])
    return float(worst)


# ---------------------------------------------------------------------------------------------------------------- reading a fixture
def case_of_call(d):
    return [str(d['case_names'][i]) for i in d['call_case']]


def subset(d, calls):
    """the fixture restricted to some Pulse calls (whole groups): the arrays replay_chain_on_oracle / replay_chain_on_engine and the
    chain checks read, renumbered"""
    calls = np.asarray(calls)
    out = {}
    ph = np.concatenate([np.arange(d['call_ph_off'][k], d['call_ph_off'][k + 1]) for k in calls] + [np.zeros(0, np.int64)]).astype(np.int64)
    pl = np.concatenate([np.arange(d['call_pulse_off'][k], d['call_pulse_off'][k + 1]) for k in calls] + [np.zeros(0, np.int64)]).astype(np.int64)
    for k in d.keys() if hasattr(d, 'keys') else d.files:
        if k.startswith('call_') and not k.endswith('_off'):
            out[k] = d[k][calls]
    for k in ('set_cluster', 'set_tmin'):
        out[k] = d[k][calls]
    out['call_ph_off'] = np.concatenate([[0], np.cumsum((d['call_ph_off'][1:] - d['call_ph_off'][:-1])[calls])]).astype(np.int64)
    out['call_pulse_off'] = np.concatenate([[0], np.cumsum((d['call_pulse_off'][1:] - d['call_pulse_off'][:-1])[calls])]).astype(np.int64)
    for k in ('ph_t', 'ph_ch', 'ph_dpe', 'ph_gain'):
        out[k] = d[k][ph]
    for k in ('pl_ch', 'pl_left', 'pl_right', 'pl_photons'):
        out[k] = d[k][pl]
    out['pl_index'] = pl
    lens = (d['pl_cur_off'][1:] - d['pl_cur_off'][:-1])[pl]
    out['pl_cur_off'] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out['pl_current'] = np.concatenate([d['pl_current'][d['pl_cur_off'][j]:d['pl_cur_off'][j + 1]] for j in pl] + [np.zeros(0)])
    # the digitise windows whose pulses are all inside the subset
    first, n = d['dg_first_pulse'], d['dg_n_pulses']
    keep = [g for g in range(len(first)) if np.all(np.isin(np.arange(first[g], first[g] + n[g]), pl))]
    assert sum(int(n[g]) for g in keep) == len(pl), 'a subset must be made of whole digitise windows'
    pos = {int(j): i for i, j in enumerate(pl)}
    for k in ('dg_left', 'dg_right', 'dg_n_pulses', 'dg_ix_rand'):
        out[k] = d[k][keep]
    out['dg_first_pulse'] = np.array([pos[int(first[g])] for g in keep], dtype=np.int64)
    rows = np.concatenate([np.arange(d['dg_row_off'][g], d['dg_row_off'][g + 1]) for g in keep] + [np.zeros(0, np.int64)]).astype(np.int64)
    out['dg_row_off'] = np.concatenate([[0], np.cumsum([d['dg_row_off'][g + 1] - d['dg_row_off'][g] for g in keep])]).astype(np.int64)
    for k in ('row_ch', 'row_left', 'row_right'):
        out[k] = d[k][rows]
    rl = (d['row_data_off'][1:] - d['row_data_off'][:-1])[rows]
    out['row_data_off'] = np.concatenate([[0], np.cumsum(rl)]).astype(np.int64)
    out['row_data'] = np.concatenate([d['row_data'][d['row_data_off'][r]:d['row_data_off'][r + 1]] for r in rows] + [np.zeros(0, np.int32)])
    z = np.flatnonzero(np.isin(d['zle_digit'], keep))
    renum = {g: i for i, g in enumerate(keep)}
    out['zle_digit'] = np.array([renum[int(g)] for g in d['zle_digit'][z]], dtype=np.int64)
    for k in ('zle_ch', 'zle_left', 'zle_right'):
        out[k] = d[k][z]
    zl = (d['zle_data_off'][1:] - d['zle_data_off'][:-1])[z]
    out['zle_data_off'] = np.concatenate([[0], np.cumsum(zl)]).astype(np.int64)
    out['zle_data'] = np.concatenate([d['zle_data'][d['zle_data_off'][i]:d['zle_data_off'][i + 1]] for i in z] + [np.zeros(0, np.int32)])
    return out


def group_calls(d, name):
    g = [str(x) for x in d['group_names']].index(name)
    return np.flatnonzero(d['call_group'] == g)


def tile_shapes(d, dt):
    """per pulse of the fixture: (photons, start bins, distinct (start bin, ns) cells, most photons in one ns)"""
    out = []
    calls = np.repeat(np.arange(len(d['call_pulse_off']) - 1), np.diff(d['call_pulse_off']))
    for j in range(len(d['pl_ch'])):
        k = int(calls[j])
        a, b = int(d['call_ph_off'][k]), int(d['call_ph_off'][k + 1])
        t = d['ph_t'][a:b][d['ph_ch'][a:b] == d['pl_ch'][j]]
        _, cnt = np.unique(t, return_counts=True)
        out.append((len(t), int(t.max() // dt - t.min() // dt + 1), len(cnt), int(cnt.max())))
    return out
