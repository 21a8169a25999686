"""Designed finished rows for the back end of a row -- finishing a sample, zero-length encoding, the interval-slot reservation, record
keys and the three packers: the case table behind tests/golden/zle_edges.npz (make_golden.py zle_edges runs the reference on it), the
noise tables that make the rows, and what the tests read back from the fixture.  Shared by make_golden.py,
tests/test_zle_edges_reference.py and tests/test_gpu_zle_edges.py.  No test lives here.

A designed NOISE TABLE gives per-sample control over a finished row: the reference finishes sample i of a channel's row as
    clamp0(adc[i] + noise[(ix_rand + i) mod N, ch] + baseline)          (rawdata.py:398-458; i counts from the channel's own row start)
so a pair of photons too weak to reach one ADC count (gain 1) makes the row exist and fixes its length, and spikes in the channel's
column put hits on any sample, sample 0 and len - 1 included.  A CASE is one channel in one digitise window; a FAMILY is one
configuration (trigger window, thresholds, HE factor) with one noise table and a few windows, each with a designed ix_rand that the
reference could have drawn (0 <= ix < high, rawdata.py:407-417 -- so a row wraps only in a window longer than the table).

Inside +-(trigger_window + 6) table rows of every spike the column carries a small position-dependent background (-2 .. 2): the samples
of an interval differ from each other, and a record read one sample off is a different record.
"""
import numpy as np

# The dispatch constants of the HIP back end, mirrored HERE and nowhere else in the tests, with the place they come from.
CHUNK = 64                  # ZleFast (wfs_kernels.h): "only the first hit of a 64-sample chunk can open an interval"; 64 slots per flush (ZleFast::close)
BLOCK = 256                 # samples per wave load of k_zle's fast path, the step of the scalar noise start (k_zle: fetch, noise_advance)
TRIP = 1024                 # G = 4 blocks per trip of k_zle's fast path (k_zle: G)
FAST_HOLD = 63              # ZleFast / resident rows need a hold-off of at least this (wfs_rows.h ZLE_FAST_HOLD: k_zle's dispatch, wfs_engine.hip run_geometry: res_on)
NOISE_MIN_FAST = 512        # shortest table of the fast row loads and of resident rows (wfs_rows.h NOISE_MIN_FAST, wfs_engine.hip run_geometry: res_on)
NOISE_PAD = 4               # a noise row is followed by its own first samples (wfs_device.h NOISE_PAD)
WFS_SPR = 110               # samples per record (wfs_rows.h WFS_SPR)
PACK_U = 4                  # records in flight in k_pack (k_pack: PACK_U)
RES_SEGMENTS = (1024, 256)  # resident segment: wfs_handle::res_max_len and WFS_RES_MAX_LEN=256 (wfs_engine.hip wfs_create)
RES_SHORT_LEN = 768         # resident rows up to this length take the short launch (wfs_layout.h RES_SHORT_LEN)
SEAMS = (64, 256, 512, 768, 1024, 2048)          # chunk, block / 256-sample segment, RES_SHORT_LEN, trip / 1024-sample segment, second trip

GROUP_SPACING = 10_000_000  # ns between windows: far above right_raw_extension plus the longest designed row
FIRST_BOTTOM = 253          # rows of the families without HE rows sit on bottom channels (a top channel has an HE row next to it)
WEAK_GAIN = 1.0             # a photon of one electron: its pulse rounds to 0 ADC counts everywhere
FRAGMENT_PLENS = (109, 111, 219, 221, 439, 441, 879, 881)       # 1|2, 2|3, 4|5 (PACK_U) and 8|9 records
INTERVAL_COUNTS = (1, 63, 64, 65, 127, 128, 129)

TW_FAMILIES = {f'tw{tw}': tw for tw in (0, 1, 10, 31, 32, 50)}
FAMILIES = list(TW_FAMILIES) + ['he801', 'he494', 'n512', 'n513', 'n700', 'n100', 'n511', 'nfloat']
SPECIAL_CHANNELS, SPECIAL_THRESHOLD = (300, 301, 302), 40
SPECIAL_CHANNEL = SPECIAL_CHANNELS[0]


def overrides(name):
    """the config overrides of a family (tests/golden/zle_edges_config.json holds them): settings only"""
    ov = dict(enable_noise=True)
    if name in TW_FAMILIES:
        ov['trigger_window'] = TW_FAMILIES[name]
    if name in ('tw50', 'tw1'):
        ov['special_thresholds'] = {str(c): SPECIAL_THRESHOLD for c in SPECIAL_CHANNELS}
    if name.startswith('he'):
        ov['high_energy_deamplification_factor'] = 20
    if name == 'n100':
        ov['trigger_window'] = 10           # (a hold-off below the table length: the hits of one spike stay apart)
    return ov


def background(j, ch):
    """the small background of table row j, column ch: -2 .. 2"""
    return int((int(j) * 2654435761 + int(ch) * 40503 + 12345) >> 7) % 5 - 2


class Family:
    """the windows and cases of one family, and the noise table they ask for"""

    def __init__(self, name, cfg, N, columns=494, float_table=False):
        self.name, self.N, self.columns, self.float_table = name, int(N), int(columns), float_table
        self.tw = int(cfg['trigger_window'])
        self.hold = max(2 * self.tw + 1, 1)
        self.dt = int(cfg.get('sample_duration', 10))
        self.before = int(cfg['samples_to_store_before']) + int(cfg.get('samples_before_pulse_center', 2))
        self.after = int(cfg['samples_to_store_after']) + int(cfg.get('samples_after_pulse_center', 20))
        self.min_len = self.before + self.after + 1 + 2 * self.tw           # the row of a single photon
        self.base = int(cfg['digitizer_reference_baseline'])
        self.zle = int(cfg['zle_threshold'])
        self.special = {int(k): int(v) for k, v in cfg.get('special_thresholds', {}).items()}
        self.he_first = int(cfg['channel_map']['he'][0])
        self.windows, self.cases = [], []
        self._next = FIRST_BOTTOM
        self.col = {}                       # (table row, column) -> noise value

    def threshold(self, ch):
        """a sample is a hit when it is BELOW this (rawdata.py:290-294)"""
        return self.base - self.special.get(ch if ch < self.he_first else -1, self.zle) - 1

    def hit(self, i, depth=4):
        """a finished value below the default threshold, different from sample to sample"""
        return self.base - self.zle - 2 - depth - (i % 7)

    def window(self, ix_rand):
        w = len(self.windows)
        b0 = GROUP_SPACING * (w + 1) // self.dt
        self.windows.append(dict(ix_rand=int(ix_rand), b0=b0, cases=[]))
        return w

    def row(self, name, length, hits=None, column=None, channel=None, shift=0, photons=(), expect=None, he_hits=None):
        """one case in the last window.  length: of the row; hits: {row sample: finished value it gets (from noise alone)};
        column: {table row: noise value} set directly (rows that wrap); shift: of the row start against the window's first bin;
        photons: [(bin offset inside the pair, gain)] real photons on top of the weak pair; he_hits: hits of the channel's HE row"""
        assert length >= self.min_len, (name, length, self.min_len)
        w = len(self.windows) - 1
        W = self.windows[w]
        if channel is None:
            channel = self._next
            self._next += 1
            while self._next in self.special:          # (kept for the threshold cases)
                self._next += 1
        assert 0 <= channel < 494 and all(c['channel'] != channel for c in self.cases), (name, channel)
        D = length - self.min_len
        b = W['b0'] + shift
        ph = [(b, WEAK_GAIN), (b + D, WEAK_GAIN)] + [(b + k, g) for k, g in photons]
        assert all(0 <= k <= D for k, _ in photons)
        ph.sort(key=lambda x: x[0])
        case = dict(name=name, window=w, channel=int(channel), length=int(length), shift=shift,
                    times=np.array([x[0] * self.dt for x in ph], dtype=np.int64), gains=np.array([x[1] for x in ph], dtype=np.float64),
                    hits=dict(hits or {}), column=dict(column or {}), he_hits=dict(he_hits or {}), expect=dict(expect or {}),
                    row_abs=b - self.before - self.tw)
        for col_ch, hh in ((channel, case['hits']), (self.he_first + channel, case['he_hits'])):
            for i, v in hh.items():
                assert 0 <= i < length and i + W['ix_rand'] < self.N, (name, i, 'a hit given by its row sample sits before the wrap')
                self._set((W['ix_rand'] + i) % self.N, col_ch, v - self.base)
        for j, v in case['column'].items():
            self._set(j % self.N, channel, v)
        self.cases.append(case)
        W['cases'].append(len(self.cases) - 1)
        return case

    def _set(self, j, ch, v):
        assert ch < self.columns, ch
        assert self.col.get((j, ch), v) == v, ('two cases want table cell', j, ch)
        assert self.float_table or -32768 <= v <= 32767
        self.col[(j, ch)] = v

    def table(self):
        """the noise table: N x columns, int16 (float64 for the float family), quiet = 0"""
        t = np.zeros((self.N, self.columns), dtype=np.float64 if self.float_table else np.int16)
        reach = self.tw + 6
        for q, ch in sorted({(q % self.N, ch) for (j, ch) in self.col for q in range(j - reach, j + reach + 1)}):
            t[q, ch] = background(q, ch)
            if self.float_table:            # integers plus fractions in (-0.9, 0.9), of the integer's sign
                fr = ((q * 37 + ch) % 17 - 8) / 10.0
                t[q, ch] += -abs(fr) if t[q, ch] < 0 else (abs(fr) if t[q, ch] > 0 else fr)
        for (j, ch), v in self.col.items():
            t[j, ch] = v
        return t

    def ix_rands(self):
        return np.array([w['ix_rand'] for w in self.windows], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _pair_row(f, tag, a, b, margin):
    """two hits a < b, the row long enough for b and its trigger window plus a margin that walks through len % 4"""
    length = max(f.min_len, b + 1 + margin)
    f.row(tag, length, {a: f.hit(a), b: f.hit(b)}, expect=dict(hits=(a, b), merged=(b - a) <= f.hold))


def holdoff_cases(f):
    """hit pairs hold - 1 .. hold + 2 apart: inside one chunk where they fit, on both sides of every seam; three hits in one interval"""
    hold = f.hold
    gaps = [g for g in (hold - 1, hold, hold + 1, hold + 2) if g >= 1]
    k = 0
    for gap in gaps:
        if gap < CHUNK:
            a = CHUNK * 2 + (CHUNK - 1 - gap)            # the second hit is the chunk's last sample
            _pair_row(f, f'pair_gap{gap}_one_chunk', a, a + gap, k % 4)
            f.cases[-1]['expect']['same_chunk'] = True
            k += 1
        # both sides of every seam: seams far enough apart for the pairs to stay apart share a row
        for place in ('first_before', 'second_at'):
            for seams in ((64, 512, 1024, 2048), (256, 768)):
                pairs = [(seam - 1, seam - 1 + gap, seam) if place == 'first_before' else (seam - gap, seam, seam) for seam in seams]
                pairs = [p for p in pairs if p[0] >= 0]
                assert all(q[0] - p[1] > hold + 2 * f.tw for p, q in zip(pairs[:-1], pairs[1:]))
                f.row(f'pairs_gap{gap}_{place}_seams_{"_".join(str(x) for x in seams)}', max(f.min_len, pairs[-1][1] + 1 + k % 4),
                      {i: f.hit(i) for p in pairs for i in p[:2]}, expect=dict(pairs=tuple(pairs), pairs_merged=gap <= hold))
                k += 1
    for seam in (64, 1024):
        a = seam - hold - 1 if seam - hold - 1 >= 0 else seam - 1
        hits = (a, a + hold, a + 2 * hold)
        f.row(f'three_hits_seam{seam}', max(f.min_len, hits[2] + 3), {i: f.hit(i) for i in hits}, expect=dict(hits=hits, n_intervals=1))


def row_end_cases(f):
    tw, hold = f.tw, f.hold
    L0 = max(f.min_len, 2 * hold + 8)
    L0 += (-L0) % 4
    for m in range(4):
        L = L0 + m
        f.row(f'ends_len_mod4_{m}', L, {0: f.hit(0), L - 1: f.hit(L - 1)}, expect=dict(hits=(0, L - 1), n_intervals=2, len_mod4=m, left_clip=tw > 0, right_clip=tw > 0))
        if tw > 0:          # the last samples whose window still clips, and the first that does not
            f.row(f'clip_edge_len_mod4_{m}', L, {tw - 1: f.hit(tw - 1), L - tw: f.hit(L - tw)},
                  expect=dict(hits=(tw - 1, L - tw), n_intervals=2, len_mod4=m, left_clip=True, right_clip=True))
            f.row(f'no_clip_len_mod4_{m}', L, {tw: f.hit(tw), L - 1 - tw: f.hit(L - 1 - tw)},
                  expect=dict(hits=(tw, L - 1 - tw), n_intervals=2, len_mod4=m, left_clip=False, right_clip=False))
    f.row('no_hit', L0 + 1, {}, expect=dict(hits=(), n_intervals=0))
    for m in (0, 1):
        L = L0 + m
        hits = tuple(sorted(set(range(0, L, hold)) | {L - 1}))
        f.row(f'one_interval_end_to_end_{m}', L, {i: f.hit(i) for i in hits}, expect=dict(hits=hits, n_intervals=1, spans_row=True))


def landing_cases(f):
    """raw left - tw and raw right + tw odd and even, on rows whose absolute start is odd and even"""
    tw = f.tw
    for start in (0, 1):
        shift = (start - (f.windows[-1]['b0'] - f.before - tw)) % 2
        for pl in (0, 1):
            for pr in (0, 1):
                a = tw + 20 + pl
                a += (pl - (a - tw)) % 2
                b = a + 4 + ((pr - (a + 4 + tw)) % 2)
                hits = {i: f.hit(i) for i in range(a, b + 1)}       # (consecutive hits: one interval at any hold-off)
                f.row(f'landing_start{start}_left{pl}_right{pr}', f.min_len + 6, hits, shift=shift,
                      expect=dict(start_parity=start, raw_left_parity=pl, raw_right_parity=pr, n_intervals=1))
    if tw == 0:
        f.row('single_hit_odd_sample', f.min_len + 1, {57: f.hit(57)}, expect=dict(hits=(57,), n_intervals=1, empty_intervals=1, n_records=0))
        f.row('single_hit_even_sample', f.min_len + 1, {58: f.hit(58)}, expect=dict(hits=(58,), n_intervals=1, empty_intervals=0, n_records=1))


def _interval(f, left, plen, length, last_hit=None):
    """hits that make one interval [left, left + plen - 1] (both even) in a row of `length`"""
    right = left + plen - 1
    a = left + f.tw
    b = right - f.tw if last_hit is None else last_hit
    assert left % 2 == 0 and right % 2 == 0 and a <= b < length
    return tuple(sorted(set(range(a, b, f.hold)) | {b}))


def fragment_cases(f):
    for plen in FRAGMENT_PLENS:
        left = 2 * ((f.tw + 7) // 2) + 2
        length = max(f.min_len, left + plen + f.tw + 9)
        hits = _interval(f, left, plen, length)
        f.row(f'fragments_plen{plen}', length, {i: f.hit(i) for i in hits}, expect=dict(n_intervals=1, plens=(plen,), n_records=-(-plen // WFS_SPR)))
    for m, plen in zip(range(4), (111, 221, 441, 881)):
        length = plen + f.tw + 60
        length += (m - length) % 4
        length = max(length, f.min_len + (m - f.min_len) % 4)
        right = (length - 1) // 2 * 2
        hits = _interval(f, right - plen + 1, plen, length, last_hit=length - 1)
        f.row(f'fragments_plen{plen}_at_row_end_len_mod4_{m}', length, {i: f.hit(i) for i in hits},
              expect=dict(n_intervals=1, plens=(plen,), len_mod4=m, ends_at_row_end=True, n_records=-(-plen // WFS_SPR)))


def count_cases(f):
    """rows of exactly 1 .. 129 intervals (hits hold + 2 apart), and the tightest row with a neighbour behind it"""
    step = f.hold + 2
    for n in INTERVAL_COUNTS:
        hits = tuple(5 + step * k for k in range(n))
        f.row(f'intervals_{n}', max(f.min_len, hits[-1] + 9), {i: f.hit(i) for i in hits}, expect=dict(n_intervals=n))


def tightest_cases(f, n):
    """hits exactly hold + 1 apart from sample 0 to the last sample: every interval slot k_row_len reserved is used"""
    step = f.hold + 1
    length = step * (n - 1) + 1
    while length < f.min_len:
        n, length = n + 1, length + step
    hits = tuple(range(0, length, step))
    f.row('tightest_row', length, {i: f.hit(i) for i in hits}, expect=dict(n_intervals=n, fills_reserved_slots=True))
    f.row('tightest_row_neighbour', f.min_len + 2, {0: f.hit(0), f.min_len: f.hit(3)}, expect=dict(hits=(0, f.min_len), first_interval_at_row_start=True))


def threshold_cases(f, templates, c2a, channel=None, tag=''):
    """noise-made samples at the threshold (no hit) and one below (a hit); pulse-made peaks of threshold + 1 and + 2 ADC counts"""
    thr_adc = f.special.get(channel, f.zle) if channel is not None else f.zle
    thr = f.base - thr_adc - 1
    L = f.min_len + 40
    f.row(f'noise_at_threshold{tag}', L, {60: thr, 61 + f.hold + 4: thr - 1, L - 3: thr}, channel=channel,
          expect=dict(hits=(61 + f.hold + 4,), values={60: thr, 61 + f.hold + 4: thr - 1, L - 3: thr}))
    peak = int(np.argmax(templates[0]))
    tmax = float(templates[0][peak])
    for k, hit in ((thr_adc + 1, False), (thr_adc + 2, True)):
        gain = k / (c2a * tmax)
        at = 20 + f.tw + f.before + peak    # photon 20 bins into the pair: its pulse starts at row sample 20 + tw, the template `before` behind
        f.row(f'pulse_peak_{"hit" if hit else "no_hit"}{tag}', L, {}, photons=[(20, gain)], channel=None if channel is None else channel + 1 + int(hit),
              expect=dict(hits=(at,) if hit else (), values={at: f.base - k}, pulse_made=True))


def clamp_cases(f, templates, top=False):
    """samples driven below 0 by noise alone, by a huge pulse alone and by both; finished 32767; one sample above 32767"""
    peak = int(np.argmax(templates[0]))
    at = 20 + f.tw + f.before + peak
    L = f.min_len + 40
    kw = lambda: dict(channel=(f._top() if top else None))
    deep = -f.base - 5
    f.row('clamp_noise_alone', L, {70: f.base + deep, 71: f.base + deep + 4}, expect=dict(values={70: 0, 71: 0}), **kw())
    f.row('clamp_pulse_alone', L, {}, photons=[(20, 2e9)], expect=dict(values={at: 0}, pulse_made=True), **kw())
    f.row('clamp_pulse_and_noise', L, {at: f.base + deep}, photons=[(20, 2e9)], expect=dict(values={at: 0}, pulse_made=True), **kw())
    f.row('finished_32767', L, {80: 32767, L - 20: f.hit(0)}, expect=dict(values={80: 32767}), **kw())
    # the sample above 32767 sits inside an interval: its ZLE tuple keeps 32768, the record what an int16 holds of it
    # (with a trigger window of 0 an interval holds hits only: the wide sample stays outside every record)
    inside = f.tw > 0
    f.row('finished_32768_inside_an_interval' if inside else 'finished_32768', L, {91: f.hit(91), 92: 32768, 93: f.hit(93)},
          expect=dict(values={92: 32768}, wide_sample_in_interval=True) if inside else dict(values={92: 32768}, n_intervals=2, empty_intervals=2), **kw())


def tw_family(name, cfg, templates, c2a):
    tw = TW_FAMILIES[name]
    f = Family(name, cfg, N=12288 if tw == 31 else 4096)
    f.window(777)
    holdoff_cases(f)
    f.window(5)
    row_end_cases(f)
    landing_cases(f)
    f.window(1234)
    fragment_cases(f)
    if tw == 31:
        f.window(2001)
        count_cases(f)
    if tw in (0, 31):
        f.window(311)
        tightest_cases(f, 21)
    f.window(63)
    threshold_cases(f, templates, c2a)
    if f.special:
        threshold_cases(f, templates, c2a, channel=SPECIAL_CHANNEL, tag='_special')
    clamp_cases(f, templates)
    return f


def he_family(name, cfg, templates, c2a):
    """rows of top channels with their HE rows (factor 20): a table of 801 columns (noise on the HE rows too) and one of 494"""
    f = Family(name, cfg, N=4096, columns=801 if name == 'he801' else 494)
    f._top_next = 17
    def _top():
        f._top_next += 3
        return f._top_next
    f._top = _top
    f.window(401)
    clamp_cases(f, templates, top=True)
    he = name == 'he801'
    L = f.min_len + 300
    a = 255 - f.hold
    f.row('he_pair_merges', L, {a: f.hit(a), 255: f.hit(255)}, channel=_top(), he_hits={100: f.hit(100), 100 + f.hold + 1: f.hit(1)} if he else None,
          expect=dict(hits=(a, 255), he_row=True))
    f.row('he_huge_pulse_between_hits', L, {30: f.hit(30)}, channel=_top(), photons=[(150, 2e9)], he_hits={L - 1: f.hit(2)} if he else None,
          expect=dict(he_row=True, pulse_made=True))
    f.window(9)
    fragment_cases_top(f, _top)
    return f


def fragment_cases_top(f, top):
    for plen in (111, 441):
        left = 2 * ((f.tw + 7) // 2) + 2
        length = left + plen + f.tw + 10
        hits = _interval(f, left, plen, length)
        f.row(f'he_fragments_plen{plen}', length, {i: f.hit(i) for i in hits}, channel=top(), he_hits={3: f.hit(3)} if f.columns > 494 else None,
              expect=dict(plens=(plen,), he_row=True))


def _wrap_column(f, rng):
    """a non-periodic spike pattern over the table rows of one column: the last row and rows 0, 1, 3 (the pad of a four-sample load
    repeats rows 0 .. 3), a spike 60 rows before the end (the interval across the wrap begins there), a few more far from both"""
    N = f.N
    col = {N - 1: -30, 0: -45, 1: -25, 3: -33, N - 60: -21}
    if N >= 400:
        lo, hi = 3 + f.hold + 12, N - 60 - f.hold - 12
        for j in sorted(rng.choice(np.arange(lo, hi), size=3, replace=False).tolist()):
            col[int(j)] = -18 - int(rng.integers(0, 20))
    return col


def wrap_family(name, cfg, N, wrap_at, general=False):
    """tables shorter than the windows: per window an ix_rand that puts the first wrap on row sample `wrap_at` (N - ix_rand), rows that
    wrap one, two and three times"""
    f = Family(name, cfg, N=N)
    rng = np.random.default_rng(7000 + N)
    for wi in wrap_at:
        ix = N - wi
        assert 0 <= ix < N - 1, (N, wi)          # (high = N - 1 in a window longer than the table)
        f.window(ix)
        for k in (1, 2, 3):
            length = max(f.min_len, k * N + (150 if N >= 400 else 45) + 37 * k + len(f.cases) % 4)
            assert (ix + length - 1) // N >= k
            f.row(f'wrap_at_{wi}_x{k}', length, column=_wrap_column(f, rng), expect=dict(wraps_at_least=k, first_wrap=wi))
    return f


def float_family(name, cfg):
    """a float64 table: truncation toward zero of adc + noise decides a hit at the threshold (tests/golden/noise_float.npz pins the
    rule on the reference's add_noise)"""
    f = Family(name, cfg, N=700, float_table=True)
    t = -(f.zle + 1)                        # noise that lands exactly on the threshold (no hit); t - 1 is a hit
    col = {100: t - 0.5, 101: t - 0.8, 102: float(t - 1), 103: t - 1.3, 104: t + 0.5, 300: t - 1 + 0.4, 301: t - 1 - 0.4, 699: t - 1.0, 0: t - 0.7, 2: t - 1.7}
    for ix, lengths in ((650, (f.min_len + 5, 760, 1500)), (12, (f.min_len + 70, 400))):
        f.window(ix)
        for L in lengths:
            f.row(f'float_ix{ix}_len{L}', L, column=col, expect=dict(float_truncation=True))
    return f


def family(name, cfg, templates=None, c2a=None):
    """the designed family `name` under its config (the bundled one plus overrides(name))"""
    if name in TW_FAMILIES:
        return tw_family(name, cfg, templates, c2a)
    if name in ('he801', 'he494'):
        return he_family(name, cfg, templates, c2a)
    if name in ('n512', 'n513', 'n700'):
        N = int(name[1:])
        return wrap_family(name, cfg, N, wrap_at=(256, 301, 302, 303, 2, N))
    if name in ('n100', 'n511'):
        N = int(name[1:])
        return wrap_family(name, cfg, N, wrap_at=(2, N // 2 + 1, N))
    if name == 'nfloat':
        return float_family(name, cfg)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- reading a fixture
def family_arrays(d, name):
    """the arrays of one family of the fixture, under the names replay_chain_on_oracle / replay_chain_on_engine read"""
    p = name + '/'
    return {k[len(p):]: d[k] for k in d.files if k.startswith(p)}


def rows_of(a):
    """per finished row of a family: dict(window, channel, abs (absolute first sample), data, intervals [(left, right) relative to the
    row, as the reference yielded them], zle [the data of each])"""
    dig = np.repeat(np.arange(len(a['dg_left'])), np.diff(a['dg_row_off']))
    out, index = [], {}
    for r in range(len(a['row_ch'])):
        g = int(dig[r])
        row = dict(window=g, channel=int(a['row_ch'][r]), abs=int(a['dg_left'][g]) + int(a['row_left'][r]),
                   data=np.asarray(a['row_data'][a['row_data_off'][r]:a['row_data_off'][r + 1]], dtype=np.int64), intervals=[], zle=[])
        index[(g, row['channel'])] = len(out)
        out.append(row)
    for k in range(len(a['zle_ch'])):
        row = out[index[(int(a['zle_digit'][k]), int(a['zle_ch'][k]))]]
        row['intervals'].append((int(a['zle_left'][k]) - row['abs'], int(a['zle_right'][k]) - row['abs']))
        row['zle'].append(np.asarray(a['zle_data'][a['zle_data_off'][k]:a['zle_data_off'][k + 1]], dtype=np.int64))
    return out, index


def expected_records(a, dt=10):
    """the strax records of the reference's ZLE tuples, in the order they were yielded (strax_interface.py:425-435): per tuple
    ceil(plen / 110) records of (time, length, dt, channel, pulse_length, record_i, baseline 0, data) -- the data what numpy's assignment
    of the int64 samples to the int16 field stores (the low 16 bits), zero padded; a tuple with left > right makes none"""
    from wfsim_amd.dtypes import raw_record_dtype
    n = [max(0, -(-(int(r) - int(l) + 1) // WFS_SPR)) for l, r in zip(a['zle_left'], a['zle_right'])]
    out = np.zeros(sum(n), dtype=raw_record_dtype())
    q = 0
    for k in range(len(n)):
        left, plen = int(a['zle_left'][k]), int(a['zle_right'][k]) - int(a['zle_left'][k]) + 1
        data = np.asarray(a['zle_data'][a['zle_data_off'][k]:a['zle_data_off'][k + 1]], dtype=np.int64)
        assert len(data) == max(plen, 0)
        for i in range(n[k]):
            m = min(plen, WFS_SPR * (i + 1)) - WFS_SPR * i
            r = out[q]
            r['time'], r['length'], r['dt'], r['channel'], r['pulse_length'], r['record_i'] = dt * (left + WFS_SPR * i), m, dt, a['zle_ch'][k], plen, i
            r['data'][:m] = data[WFS_SPR * i:WFS_SPR * i + m].astype(np.int16)
            q += 1
    return out


def measure(f, case, row, he_row, ix_rand):
    """what the reference's output says about one case: the seams it reached"""
    thr = f.threshold(case['channel'])
    data, itv = row['data'], row['intervals']
    L = len(data)
    hits = tuple(np.flatnonzero(data < thr).tolist())
    plens = tuple(b - a + 1 for a, b in itv)
    wraps = [k * f.N - ix_rand for k in range(1, (ix_rand + L - 1) // f.N + 1)]
    m = dict(length=L, len_mod4=L % 4, start_parity=row['abs'] % 2, hits=hits, n_intervals=len(itv), plens=plens,
             empty_intervals=sum(1 for p in plens if p <= 0), n_records=sum(-(-p // WFS_SPR) for p in plens if p > 0),
             reserved=(L + f.hold) // (f.hold + 1), wraps=len(wraps), first_wrap=wraps[0] if wraps else None,
             wrap_record_pos=tuple(sorted({(w - a) % WFS_SPR for w in wraps for a, b in itv if a <= w <= b})),
             he_row=he_row is not None)
    # consecutive hits inside one interval (the even landing moves an end by at most one sample)
    m['joined'] = tuple(any(l - 1 <= a and b <= r + 1 for l, r in itv) for a, b in zip(hits[:-1], hits[1:]))
    if len(hits) >= 2:
        m['merged'] = len(itv) == 1
        m['same_chunk'] = hits[0] // CHUNK == hits[1] // CHUNK
    if hits:
        m['raw_left_parity'], m['raw_right_parity'] = (hits[0] - f.tw) % 2, (hits[-1] + f.tw) % 2
        m['left_clip'], m['right_clip'] = hits[0] - f.tw < 0, hits[-1] + f.tw > L - 1
    if itv:
        m['spans_row'] = itv[0][0] == 0 and itv[-1][1] == (L - 1) // 2 * 2 and len(itv) == 1
        m['ends_at_row_end'] = itv[-1][1] == (L - 1) // 2 * 2 and hits[-1] == L - 1
        m['first_interval_at_row_start'] = itv[0][0] == 0 and hits[0] == 0
    m['fills_reserved_slots'] = len(itv) == m['reserved']
    return m


def check_case(f, case, row, he_row, ix_rand):
    """the list of seams the case was designed for and did not reach (empty: all reached)"""
    m = measure(f, case, row, he_row, ix_rand)
    e, bad = case['expect'], []
    data = row['data']
    if m['length'] != case['length']:
        bad.append(('length', m['length'], case['length']))
    designed = tuple(sorted(i for i, v in case['hits'].items() if v < f.threshold(case['channel'])))
    if not case['column'] and not e.get('pulse_made') and m['hits'] != designed:
        bad.append(('designed hits', m['hits'], designed))
    for k, v in e.items():
        if k == 'values':
            for i, want in v.items():
                if int(data[i]) != want:
                    bad.append(('value', i, int(data[i]), want))
        elif k == 'pairs':
            h = m['hits']
            for q, (a, b, seam) in enumerate(v):
                if not (len(h) == 2 * len(v) and h[2 * q] == a and h[2 * q + 1] == b and a < seam <= b and m['joined'][2 * q] == e['pairs_merged']):
                    bad.append((k, h, (a, b, seam)))
            if any(m['joined'][1::2]):
                bad.append(('two pairs in one interval', m['joined']))
        elif k == 'pairs_merged':
            pass
        elif k == 'wraps_at_least':
            if m['wraps'] < v:
                bad.append((k, m['wraps'], v))
        elif k == 'wide_sample_in_interval':
            if not any(z.max() == 32768 for z in row['zle'] if len(z)):
                bad.append((k,))
        elif k == 'float_truncation':
            pass                            # (asserted on the table and the rows by the test itself)
        elif k == 'pulse_made':
            pass
        elif m.get(k) != v:
            bad.append((k, m.get(k), v))
    return bad
