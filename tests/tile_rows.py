"""Designed ZLE seams on rows that are read IN PLACE from the tile buffers of k_s2_tile and k_s2_bright (`src = 1` descriptors of
k_row_desc): the sources, the families, the case table and the noise tables behind tests/test_tile_rows_cpu.py and
tests/test_gpu_tile_rows.py.  No test lives here; everything is computed on the CPU, from the oracle alone.

The samples of such a row come out of the tile generator and cannot be designed, but its HITS can: with noise on a finished sample is
    clamp0(adc[i] + noise[(ix_rand + i) mod N, ch] + baseline)
and a tile-made pulse only lowers it.  Every family puts the ZLE threshold (ZLE) deeper than the deepest pulse sample of any source, so a
pulse alone never makes a hit, and spikes in the channel's noise column put hits on any row sample -- the method of tests/zle_edges.py,
whose constants and background are reused.  The oracle is run once per (source, family) with noise off: that gives every row's absolute
start, its length L, its noise-free samples and the pulses it holds.  A spike that is to finish sample i as v is the table cell
v - noise_free[i]; a CASE is one (window, channel) row, picked among the rows the helper EXPECTS to be read in place (one pulse, whose
instruction is alone in its Pulse call and passes fuse_eligible -- tests/hot_patterns.py) by what the case needs of (L, acc_off % 4).

acc_off % 4: a tile's buffer begins at ins_boff[ins] + ch * ins_bcap[ins] ints (k_row_desc), ins_bcap the restatement below of
k_fuse_electrons' formula -- span / dt plus constants, no multiple of 4, so the 16-byte loads of k_zle's fast path meet every alignment
from channel to channel.  tests/test_gpu_tile_rows.py asserts the restatement's inputs (first and last electron) on the device.
"""
import numpy as np

from tests import hot_patterns as HP
from tests import zle_edges as ZE
from tests.helpers import make_oracle, with_fma
from tests.sum_signal import SUM_CHANNEL, expected_sum_rows
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype
from wfsim_amd.resource import Resource

MS = 1_000_000
SEED = 20261021
ZLE = 5000                  # zle_threshold of every family: deeper than the deepest pulse sample of any source (bright: 4761 ADC counts)
TILE_MAX_PHOTONS = 2048     # wfs_tilegen.h: a tile above it takes k_s2_bright (kind 3), one up to it k_s2_tile (kind 1)
BRIGHT_MAX_BINS = 1480      # start bins a bright source here may span: well inside what bright_fits admits (wfs_tilegen.h; 128 KB of H table)
TABLE_SPAN = 8192           # cells of the S2 delay table (FuseArgs::table_span; the CPU test reads it off the oracle's alias table)

_S = lambda **kw: dict(type=2, **kw)
# name -> (s2_secondary_sc_gain, instructions); windows are 3 ms apart.  The depths and amplitudes were settled on the oracle: see COVERAGE
# in tests/test_tile_rows_cpu.py for the row lengths they give.
SOURCES = {
    'tile_shallow': (21.3, [_S(time=MS, x=2, y=1, z=-8, amp=2500)]),
    'tile_deep': (21.3, [_S(time=MS, x=2, y=1, z=-95, amp=2500)]),                      # rows beyond 1024 samples
    'bright': (100.0, [_S(time=MS, x=0, y=0, z=-8, amp=20000)]),
    'bright_deep': (100.0, [_S(time=MS, x=0, y=0, z=-24.5, amp=28000)]),                # the deepest S2 whose tiles still fit k_s2_bright with a margin
    'mixed_window': (21.3, [_S(time=MS, x=2, y=1, z=-8, amp=2500), _S(time=MS + 2000, x=2, y=1, z=-8, amp=15),       # shared rows on about half the channels
                            dict(type=1, time=4 * MS, x=0, y=0, z=-30, amp=60)]),                                  # a small S1: rows that go resident on request
    'three_windows': (100.0, [_S(time=MS, x=2, y=1, z=-8, amp=2500), _S(time=4 * MS, x=0, y=0, z=-8, amp=20000), _S(time=7 * MS, x=5, y=-3, z=-8, amp=60)]),
}
KERNEL = {'tile_shallow': 'k_s2_tile', 'tile_deep': 'k_s2_tile', 'bright': 'k_s2_bright', 'bright_deep': 'k_s2_bright'}

# name -> trigger window, table rows, columns, float table, HE factor, sum row
FAMILIES = {f'tw{tw}': dict(tw=tw) for tw in (0, 1, 10, 31, 32, 50)}
FAMILIES.update(n700=dict(N=700), n513=dict(N=513), n100=dict(N=100, tw=10), nfloat=dict(float_table=True),
                he801=dict(he=20, columns=801), sum801=dict(he=20, columns=801, sum_row=True))
IX_RAND = (777, 5, 1234)    # of the windows of a source, in order
WRAP_AT = 150


def family_config(source, family, noise=None):
    f = FAMILIES[family]
    kw = dict(seed=SEED, tile_local_min_photons=0, s2_secondary_sc_gain=SOURCES[source][0], zle_threshold=ZLE, trigger_window=f.get('tw', 50),
              enable_noise=noise is not None)
    if f.get('he'):
        kw['high_energy_deamplification_factor'] = f['he']
    if f.get('sum_row'):
        kw['emit_sum_signal'] = True
    if noise is not None:
        kw['noise_data'] = noise
    return with_fma(xenonnt_test_config(**kw), False)


def instructions(source):
    rows = SOURCES[source][1]
    ins = np.zeros(len(rows), dtype=instruction_dtype)
    for k, r in enumerate(rows):
        for f, v in r.items():
            ins[k][f] = v
    ins['recoil'], ins['event_number'] = 7, np.arange(len(rows))
    return ins


def buffer_caps(p, o, fused, tw):
    """ins_bcap per instruction (k_fuse_electrons) and ins_boff (the scan of n_tpc * ins_bcap): from the first and last electron of
    every primary call of the oracle -- such an instruction is alone in its call"""
    prim = HP.primary_calls(o)
    cap = np.zeros(len(prim), dtype=np.int64)
    for q, c in enumerate(prim):
        e = o['e_t'][o['call_e_off'][c]:o['call_e_off'][c + 1]]
        if fused[q] and len(e):
            span = int(e.max()) - int(e.min()) + TABLE_SPAN
            cap[q] = span // int(p['dt']) + 2 + int(p['store_before']) + int(p['samples_before']) + int(p['store_after']) + int(p['samples_after']) + 2 * tw + 4
    boff = np.concatenate([[0], np.cumsum(cap * int(p['n_tpc']))])
    return cap, boff


_geometry = {}


def geometry(source, family):
    """the noise-free oracle run of a source under a family's settings: dict(cfg, p, sched, o, rows {(window, channel): row}, caps, boff).
    row: window, ch, abs, L, data (int64, noise free), n_pulses, direct (expected read in place), kind (1 / 3 expected of its tile), ins
    (the instruction of its first pulse), acc_mod4; an HE row has `top` (its top channel) and is direct when that row is."""
    f = FAMILIES[family]
    key = (source, f.get('tw', 50), f.get('he', 0), bool(f.get('sum_row')))
    if key in _geometry:
        return _geometry[key]
    cfg = family_config(source, family)
    p = kernel_params(cfg)
    ins = instructions(source)
    res = Resource(cfg)
    s = HP.scheduled(cfg, ins, res)
    orc = make_oracle(cfg)
    orc.simulate(s['s_ins'], s['gid'], s['ip'])
    o = orc.results()
    fused = HP.tile_generated(cfg, s)
    assert s['n_calls'] == len(ins) and len(HP.primary_calls(o)) == len(ins)          # every instruction alone in its Pulse call
    cap, boff = buffer_caps(p, o, fused, int(p['trigger_window']))
    sizes = HP.tile_sizes(o)[HP.primary_calls(o)]
    call_of = HP.pulse_calls(o)
    n_tpc, he_first = int(p['n_tpc']), int(p['he_first'])
    rows = {}
    for w in range(len(o['dg_left'])):
        a, b = int(o['dg_first_pulse'][w]), int(o['dg_first_pulse'][w] + o['dg_n_pulses'][w])
        pulses = {}
        for q in range(a, b):
            pulses.setdefault(int(o['pl_ch'][q]), []).append(int(call_of[q]))
        for r in range(int(o['dg_row_off'][w]), int(o['dg_row_off'][w + 1])):
            ch = int(o['row_ch'][r])
            row = dict(window=w, ch=ch, abs=int(o['dg_left'][w] + o['row_left'][r]), L=int(o['row_right'][r] - o['row_left'][r] + 1),
                       data=o['row_data'][o['row_data_off'][r]:o['row_data_off'][r + 1]].astype(np.int64))
            if ch < n_tpc:
                calls = pulses[ch]
                i = calls[0]
                row.update(n_pulses=len(calls), ins=i, direct=len(calls) == 1 and bool(fused[i]), kind=3 if sizes[i, ch] > TILE_MAX_PHOTONS else 1,
                           acc_mod4=int((boff[i] + ch * cap[i]) % 4), cap=int(cap[i]))
            rows[(w, ch)] = row
    for (w, ch), row in rows.items():
        if ch >= he_first:
            top = rows[(w, ch - he_first)]
            row.update(top=ch - he_first, **{k: top[k] for k in ('n_pulses', 'ins', 'direct', 'kind', 'acc_mod4', 'cap')})
    sums = expected_sum_rows(o, p, orc.tables['thr_zle']) if f.get('sum_row') else []
    g = dict(cfg=cfg, p=p, sched=s, o=o, rows=rows, cap=cap, boff=boff, fused=fused, sizes=sizes, sum_rows=sums,
             deepest=min(int(r['data'].min()) for r in rows.values() if r['ch'] < n_tpc))
    _geometry[key] = g
    return g


# ---------------------------------------------------------------------------------------------------------------- the cases
class Family:
    """the case table of one source under one family: cases picked on the rows of geometry(), and the noise table they ask for"""

    def __init__(self, source, family):
        f = FAMILIES[family]
        self.source, self.name, self.g = source, family, geometry(source, family)
        p = self.g['p']
        self.tw = int(p['trigger_window'])
        self.hold = max(2 * self.tw + 1, 1)
        self.N, self.columns, self.float_table = int(f.get('N', 4096)), int(f.get('columns', 494)), bool(f.get('float_table'))
        self.base, self.he_first, self.n_top, self.n_tpc = int(p['baseline']), int(p['he_first']), int(p['n_top']), int(p['n_tpc'])
        self.thr = self.base - ZLE - 1                       # a sample is a hit when it is BELOW this (tables.thresholds)
        n_win = len(self.g['o']['dg_left'])
        # (a table shorter than the rows: the first wrap lands on row sample WRAP_AT - window, inside every row)
        self.ix = np.array([IX_RAND[w] if self.N >= 4096 else (self.N - WRAP_AT + w if self.N > WRAP_AT else IX_RAND[w] % (self.N - 1)) for w in range(n_win)], dtype=np.int64)
        self.cases, self.used, self.col, self.missing = [], set(), {}, []
        self.wraps = self.N < 4096
        _cases(self)

    def hit(self, i, depth=4):
        return self.thr - 1 - depth - (i % 7)

    def pick(self, name, fits, hits, expect=None, pool='direct', behind=False):
        """the case `name` on the first unused row of `pool` ('direct': expected read in place; 'shared': several pulses; 'he': the HE
        row of a direct top row) for which fits(row); hits(row) -> {row sample: finished value}; a case no row qualifies for is listed
        in `missing` (the CPU test fails on it).  behind: spikes also in the column's cells of the samples L .. ceil4(L) - 1 BEHIND the
        row (four cells where L is a multiple of 4): the oracle never reads them, and a device that looked at the whole last four-sample
        load of the row, or at a lane past its end, would find hits there"""
        for key in sorted(self.g['rows']):
            r = self.g['rows'][key]
            he = r['ch'] >= self.he_first
            ok = (pool == 'he') == he and (r['direct'] if pool in ('direct', 'he') else r['n_pulses'] > 1)
            if self.name == 'sum801' and pool == 'direct':
                ok = ok and r['ch'] >= self.n_top               # the rows k_sum_signal adds up
            if not ok or key in self.used or not fits(r):
                continue
            try:
                h = {int(i): int(v) for i, v in hits(r).items()}
            except _NoFit:
                continue
            assert all(0 <= i < r['L'] for i in h), (name, sorted(h), r['L'])
            self.used.add(key)
            e = dict(expect(r) if callable(expect) else (expect or {}))
            if pool == 'he':        # an HE row is its top row times the factor: the pulse makes hits of its own there, the oracle says which
                e = dict(he_row=True)
            if self.wraps:          # a table shorter than the row: a spike returns every N samples, the designed seam is not claimed
                e = dict(wraps=True)
            case = dict(name=name, window=r['window'], channel=r['ch'], length=r['L'], hits=h, expect=e, pool=pool, acc_mod4=r['acc_mod4'], kind=r['kind'])
            for i, v in h.items():
                self._set((int(self.ix[r['window']]) + i) % self.N, r['ch'], v - int(r['data'][i]) + (0 if v > 0 else -5))
            if behind:
                case['behind'] = [(int(self.ix[r['window']]) + r['L'] + j) % self.N for j in range(4 - r['L'] % 4)]
                for j, cell in enumerate(case['behind']):
                    self._set(cell, r['ch'], self.hit(r['L'] + j) - self.base)
            self.cases.append(case)
            return case
        self.missing.append(name)
        return None

    def _set(self, j, ch, v):
        assert ch < self.columns and -32768 <= v <= 32767, (j, ch, v)
        if self.col.setdefault((j, ch), v) != v:
            assert self.wraps, ('two hits of a case want table cell', j, ch)

    def table(self, spikes=True):
        """N x columns, int16 (float64: integers plus fractions of the integer's sign, as zle_edges.Family.table); spikes=False: the
        background alone, on the same cells"""
        t = np.zeros((self.N, self.columns), dtype=np.float64 if self.float_table else np.int16)
        reach = self.tw + 6
        cells = set(self.col)
        if self.name == 'sum801':
            cells |= {(j, SUM_CHANNEL) for j in self.sum_spikes()}
        for q, ch in sorted({(q % self.N, ch) for (j, ch) in cells for q in range(j - reach, j + reach + 1)}):
            t[q, ch] = ZE.background(q, ch)
            if self.float_table:
                fr = ((q * 37 + ch) % 17 - 8) / 10.0
                t[q, ch] += -abs(fr) if t[q, ch] < 0 else (abs(fr) if t[q, ch] > 0 else fr)
        if spikes:
            for (j, ch), v in self.col.items():
                t[j, ch] = v - (((j * 37 + ch) % 8) / 10.0 if self.float_table and v < 0 else 0.0)
            for j, v in (self.sum_spikes() if self.name == 'sum801' else {}).items():
                t[j, SUM_CHANNEL] = v
        return t

    def sum_spikes(self):
        """table cells of column 800: spikes on the first and last samples of every sum row, on both sides of the seams inside it"""
        out = {}
        for e in self.g['sum_rows']:
            n, ix = len(e['S']), int(self.ix[e['window']])
            for i in (0, 1, self.tw, 63, 64, 255, 256, 511, 512, n - 1 - self.tw, n - 2, n - 1):
                if 0 <= i < n:
                    out[(ix + i) % self.N] = -6000 - i % 11
        return out

    def case_rows(self):
        return [(c, self.g['rows'][(c['window'], c['channel'])]) for c in self.cases]


class _NoFit(Exception):
    pass


def _cases(f):
    tw, hold = f.tw, f.hold
    H = f.hit
    longest = sorted(r['L'] for r in f.g['rows'].values() if r['direct'] and r['ch'] < f.n_tpc)[-10]          # (ten rows are at least this long)
    gaps = [g for g in (hold - 1, hold, hold + 1, hold + 2) if g >= 1]
    pools = ['direct'] + (['shared'] if f.source == 'mixed_window' else [])
    for pool in pools:
        tag = '' if pool == 'direct' else '_shared'
        # ---- hit pairs inside one chunk and on both sides of every seam below L
        for gap in gaps:
            if gap < ZE.CHUNK:
                a = ZE.CHUNK * 2 + (ZE.CHUNK - 1 - gap)
                f.pick(f'pair_gap{gap}_one_chunk{tag}', lambda r, b=a + gap: r['L'] > b, lambda r, a=a, gap=gap: {a: H(a), a + gap: H(a + gap)},
                       dict(hits=(a, a + gap), merged=gap <= hold, same_chunk=True), pool)
            for seam in ZE.SEAMS:
                if seam + gap + 1 > longest:
                    continue
                for place, (a, b) in (('first_before', (seam - 1, seam - 1 + gap)), ('second_at', (seam - gap, seam))):
                    if a < 0:
                        continue
                    f.pick(f'pair_gap{gap}_{place}_seam{seam}{tag}', lambda r, b=b: r['L'] > b, lambda r, a=a, b=b: {a: H(a), b: H(b)},
                           dict(hits=(a, b), merged=gap <= hold, seam=seam), pool)
        # ---- sample 0 and L - 1 for each of the 16 classes (L % 4, acc_off % 4)
        for m in range(4):
            for am in range(4):
                f.pick(f'ends_len_mod4_{m}_acc_mod4_{am}{tag}', lambda r, m=m, am=am: r['L'] % 4 == m and r['acc_mod4'] == am and r['L'] > 2 * hold + 8,
                       lambda r: {0: H(0), r['L'] - 1: H(r['L'] - 1)},
                       lambda r, m=m, am=am: dict(hits=(0, r['L'] - 1), n_intervals=2, len_mod4=m, acc_mod4=am, left_clip=tw > 0, right_clip=tw > 0), pool, behind=True)
    # ---- one hit on sample 0 and spikes BEHIND the row, for each of the 16 classes: a hit found there is farther than the hold-off
    # from the row's only hit and would open an interval of its own (behind a hit on L - 1 it would only merge into that one)
    for m in range(4):
        for am in range(4):
            f.pick(f'behind_len_mod4_{m}_acc_mod4_{am}', lambda r, m=m, am=am: r['L'] % 4 == m and r['acc_mod4'] == am and r['L'] > 2 * hold + 8,
                   lambda r: {0: H(0)}, lambda r, m=m, am=am: dict(hits=(0,), n_intervals=1, len_mod4=m, acc_mod4=am), behind=True)
    for seam in (64, 1024):
        a = seam - hold - 1 if seam - hold - 1 >= 0 else seam - 1
        hits = (a, a + hold, a + 2 * hold)
        if hits[2] + 3 <= longest:
            f.pick(f'three_hits_seam{seam}', lambda r, b=hits[2]: r['L'] >= b + 3, lambda r, hits=hits: {i: H(i) for i in hits}, dict(hits=hits, n_intervals=1))
    # ---- the clip edges for every L % 4
    for m in range(4):
        fit = lambda r, m=m: r['L'] % 4 == m and r['L'] > 2 * hold + 8
        if tw > 0:
            f.pick(f'clip_edge_len_mod4_{m}', fit, lambda r: {tw - 1: H(tw - 1), r['L'] - tw: H(r['L'] - tw)},
                   lambda r, m=m: dict(hits=(tw - 1, r['L'] - tw), n_intervals=2, len_mod4=m, left_clip=True, right_clip=True), behind=True)
            f.pick(f'no_clip_len_mod4_{m}', fit, lambda r: {tw: H(tw), r['L'] - 1 - tw: H(r['L'] - 1 - tw)},
                   lambda r, m=m: dict(hits=(tw, r['L'] - 1 - tw), n_intervals=2, len_mod4=m, left_clip=False, right_clip=False), behind=True)
    f.pick('no_hit', lambda r: True, lambda r: {}, dict(hits=(), n_intervals=0))
    for m in (0, 1):
        def whole(r):
            return {i: H(i) for i in sorted(set(range(0, r['L'], hold)) | {r['L'] - 1})}
        f.pick(f'one_interval_end_to_end_{m}', lambda r, m=m: r['L'] % 2 == m, whole, lambda r: dict(n_intervals=1, spans_row=True))
    # ---- the eight even landings: row start, raw left, raw right
    for start in (0, 1):
        for pl in (0, 1):
            for pr in (0, 1):
                a = tw + 20 + pl
                a += (pl - (a - tw)) % 2
                b = a + 4 + ((pr - (a + 4 + tw)) % 2)
                f.pick(f'landing_start{start}_left{pl}_right{pr}', lambda r, start=start, b=b: r['abs'] % 2 == start and r['L'] > b + tw + 2,
                       lambda r, a=a, b=b: {i: H(i) for i in range(a, b + 1)}, dict(start_parity=start, raw_left_parity=pl, raw_right_parity=pr, n_intervals=1))
    # ---- intervals of every fragment length; ending on the row's last even sample for every L % 4
    for plen in ZE.FRAGMENT_PLENS:
        left = 2 * ((tw + 7) // 2) + 2
        if left + plen + tw + 9 > longest:
            continue
        f.pick(f'fragments_plen{plen}', lambda r, n=left + plen + tw + 9: r['L'] >= n, lambda r, left=left, plen=plen: {i: H(i) for i in _interval(f, left, plen)},
               dict(n_intervals=1, plens=(plen,), n_records=-(-plen // ZE.WFS_SPR)))
    fitting = [q for q in (881, 441, 221, 111) if q + tw + 70 <= longest]          # (the fragment lengths that fit the source's rows)
    for m in range(4 if fitting else 0):
        plen = fitting[m % len(fitting)]

        def at_end(r, plen=plen):
            right = (r['L'] - 1) // 2 * 2
            return {i: H(i) for i in _interval(f, right - plen + 1, plen, last_hit=r['L'] - 1)}
        f.pick(f'fragments_plen{plen}_at_row_end_len_mod4_{m}', lambda r, m=m, plen=plen: r['L'] % 4 == m and r['L'] >= plen + tw + 4, at_end,
               dict(n_intervals=1, plens=(plen,), len_mod4=m, ends_at_row_end=True, n_records=-(-plen // ZE.WFS_SPR)))
    # ---- rows of 1 .. 129 intervals where the hold-off lets them fit
    step = hold + 2
    for n in ZE.INTERVAL_COUNTS:
        if 5 + step * (n - 1) + 9 <= longest:
            f.pick(f'intervals_{n}', lambda r, n=n: r['L'] >= 5 + step * (n - 1) + 9, lambda r, n=n: {5 + step * k: H(5 + step * k) for k in range(n)}, dict(n_intervals=n))
    # ---- every slot k_row_len reserved: hits hold + 1 apart from sample 0 to the last sample
    f.pick('tightest_row', lambda r: True, lambda r: {i: H(i) for i in range(0, r['L'], hold + 1)},
           lambda r: dict(n_intervals=(r['L'] - 1) // (hold + 1) + 1, fills_reserved_slots=True))
    # ---- on the threshold and one count above it (no hits), one below (a hit): in the zeros in front of the pulse and on the pulse
    def at_threshold(r, on_pulse):
        d = r['data']
        if on_pulse:
            i = int(np.argmin(d))
        else:
            flat = np.flatnonzero((d[:-1] == f.base) & (d[1:] == f.base))
            if not len(flat):
                raise _NoFit
            i = int(flat[0])
        if d[i] == f.base and on_pulse or i + hold + 5 >= r['L']:
            raise _NoFit
        return {i: f.thr, i + 1: f.thr + 1, i + hold + 4: f.thr - 1}
    for on_pulse in (False, True):
        f.pick(f'threshold_{"on_pulse" if on_pulse else "in_zeros"}', lambda r: True, lambda r, q=on_pulse: at_threshold(r, q),
               lambda r, q=on_pulse: dict(n_intervals=1, threshold_values=True))
    # ---- the pulse's deepest sample clamped to 0
    f.pick('clamp_deepest', lambda r: True, lambda r: {int(np.argmin(r['data'])): 0}, lambda r: dict(values={int(np.argmin(r['data'])): 0}, n_intervals=1))
    # ---- the highest live channel of the last instruction: its buffer ends tbuf
    last = max((k for k, r in f.g['rows'].items() if r['ch'] < f.n_tpc and r['direct'] and r['window'] == len(f.ix) - 1), default=None)
    if last is not None and last not in f.used:
        f.pick('last_buffer_of_tbuf', lambda r: (r['window'], r['ch']) == last, lambda r: {0: H(0), r['L'] - 1: H(r['L'] - 1)},
               lambda r: dict(hits=(0, r['L'] - 1), last_buffer=True))
    # ---- HE rows of direct top rows: a second descriptor on the same buffer
    if f.name == 'he801':
        for m in range(4):
            f.pick(f'he_ends_acc_mod4_{m}', lambda r, m=m: r['acc_mod4'] == m and r['L'] > 2 * hold + 8, lambda r: {0: H(0), r['L'] - 1: H(r['L'] - 1)},
                   lambda r, m=m: dict(hits=(0, r['L'] - 1), n_intervals=2, acc_mod4=m), pool='he', behind=True)
        a = 255 - hold
        f.pick('he_pair_merges_at_256', lambda r: r['L'] > 300 + tw and a >= 0, lambda r: {a: H(a), 255: H(255)}, dict(hits=(a, 255), merged=True), pool='he')


def _interval(f, left, plen, last_hit=None):
    """hits that make one interval [left, left + plen - 1] (both even)"""
    right = left + plen - 1
    a = left + f.tw
    b = right - f.tw if last_hit is None else last_hit
    if not (left >= 0 and left % 2 == 0 and right % 2 == 0 and a <= b):
        raise _NoFit
    return tuple(sorted(set(range(a, b, f.hold)) | {b}))


# ---------------------------------------------------------------------------------------------------------------- the oracle's answer
_runs = {}


def oracle_run(source, family, spikes=True):
    """(Family, oracle, results) of the source under the family's table, every window's ix_rand injected"""
    key = (source, family, spikes)
    if key not in _runs:
        for k in [k for k in _runs if k[:2] != (source, family)]:
            del _runs[k]
        fam = Family(source, family)
        cfg = family_config(source, family, noise=fam.table(spikes))
        s = fam.g['sched']
        orc = make_oracle(cfg)
        orc.set_noise_override(fam.ix)
        orc.simulate(s['s_ins'], s['gid'], s['ip'])
        _runs[key] = (fam, cfg, orc, orc.results())
    return _runs[key]


def finished_rows(o):
    """{(window, channel): (absolute first sample, finished samples int64, [(left, right)] of its intervals relative to the row)}"""
    out = {}
    for w in range(len(o['dg_left'])):
        for r in range(int(o['dg_row_off'][w]), int(o['dg_row_off'][w + 1])):
            out[(w, int(o['row_ch'][r]))] = (int(o['dg_left'][w] + o['row_left'][r]), o['row_data'][o['row_data_off'][r]:o['row_data_off'][r + 1]].astype(np.int64), [])
    for k in range(len(o['zl_ch'])):
        key = (int(o['zl_digit'][k]), int(o['zl_ch'][k]))
        if key in out:              # (the sum row is no row of the list)
            out[key][2].append((int(o['zl_left'][k]) - out[key][0], int(o['zl_right'][k]) - out[key][0]))
    return out


def measure(f, case, data, itv):
    """what the oracle's output says about one case: zle_edges.measure for a row whose length was given"""
    L = len(data)
    hits = tuple(np.flatnonzero(data < f.thr).tolist())
    plens = tuple(b - a + 1 for a, b in itv)
    m = dict(length=L, len_mod4=L % 4, acc_mod4=case['acc_mod4'], hits=hits, n_intervals=len(itv), plens=plens,
             n_records=sum(-(-p // ZE.WFS_SPR) for p in plens if p > 0), reserved=(L + f.hold) // (f.hold + 1),
             wraps=(int(f.ix[case['window']]) + L - 1) // f.N >= 1)
    if len(hits) >= 2:
        m['merged'] = len(itv) == 1
        m['same_chunk'] = hits[0] // ZE.CHUNK == hits[1] // ZE.CHUNK
        m['seam'] = next((s for s in ZE.SEAMS if hits[0] < s <= hits[1]), None)
    if hits:
        m['raw_left_parity'], m['raw_right_parity'] = (hits[0] - f.tw) % 2, (hits[-1] + f.tw) % 2
        m['left_clip'], m['right_clip'] = hits[0] - f.tw < 0, hits[-1] + f.tw > L - 1
    if itv:
        m['spans_row'] = itv[0][0] == 0 and itv[-1][1] == (L - 1) // 2 * 2 and len(itv) == 1
        m['ends_at_row_end'] = itv[-1][1] == (L - 1) // 2 * 2 and hits[-1] == L - 1
    m['fills_reserved_slots'] = len(itv) == m['reserved']
    return m


def check_case(f, case, row_abs, data, itv):
    """the seams the case was designed for and did not reach (empty: all reached), in the manner of zle_edges.check_case.  In the
    families whose table is shorter than the rows (n700, n513, n100) a spike returns every N samples, so a case's expectations are
    replaced by `wraps` and its designed hits are not compared: there the CPU side checks only that the row wraps (and, in the test,
    that the stand-alone finder agrees with the oracle); the device is still compared byte for byte with the oracle"""
    m = measure(f, case, data, itv)
    m['start_parity'] = row_abs % 2
    e, bad = case['expect'], []
    if m['length'] != case['length']:
        bad.append(('length', m['length'], case['length']))
    designed = tuple(sorted(i for i, v in case['hits'].items() if v < f.thr))
    if not f.wraps and case['pool'] != 'he' and m['hits'] != designed:
        bad.append(('designed hits', m['hits'], designed))
    for k, v in e.items():
        if k == 'values':
            bad += [('value', i, int(data[i]), want) for i, want in v.items() if int(data[i]) != want]
        elif k == 'threshold_values':
            got = sorted(int(data[i]) for i in case['hits'])
            if got != [f.thr - 1, f.thr, f.thr + 1]:
                bad.append((k, got))
        elif k in ('last_buffer', 'he_row'):
            pass
        elif m.get(k) != v:
            bad.append((k, m.get(k), v))
    return bad


def standalone_intervals(f, data):
    """the stand-alone interval finder plus window, clip and even landing (rawdata.py:290-311), as tests/sum_signal.py restates them"""
    from oracle.oracle import Oracle
    out = []
    for a, b in Oracle.find_intervals_below_threshold(data, f.thr, f.hold):
        a, b = np.clip([a - f.tw, b + f.tw], 0, len(data) - 1)
        out.append((int(np.ceil(a / 2) * 2), int(np.floor(b / 2) * 2)))
    return out


# ---------------------------------------------------------------------------------------------------------------- without noise (NK = 0)
NOISELESS = ('tile_shallow', 'bright')


def noiseless_config(source):
    """enable_noise off, the benchmark's own instantiation: special_thresholds per channel from the oracle's noise-free rows, so that
    the 1, 2 or 3 deepest samples of the channel's pulse (by channel % 3) are its only hits; returns (config, {channel: hit samples})"""
    g = geometry(source, 'tw50')
    base, special, hits = int(g['p']['baseline']), {}, {}
    for (w, ch), r in g['rows'].items():
        if ch >= int(g['p']['n_tpc']) or not r['direct']:
            continue
        v = np.unique(r['data'])              # (sorted)
        k = min(ch % 3 + 1, len(v) - 1)
        if k < 1:
            continue
        special[str(ch)] = base - int(v[k]) - 1         # tables.thresholds: thr_zle = base - special - 1 = v[k]; a hit lies below it
        hits[ch] = tuple(np.flatnonzero(r['data'] < int(v[k])).tolist())
    cfg = dict(family_config(source, 'tw50'), special_thresholds=special, zle_threshold=base - 1)
    return cfg, hits
