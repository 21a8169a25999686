"""Noise-hit seeds of the lone-hit rows (config 'noise_lone_hits', wfs_set_lone_noise_hits) restated in numpy on top of the
``Lone`` / ``Dark`` restatements (tests/lone_hits.py, tests/dark_counts.py) and the noise restatements (tests/noise_model.py,
tests/noise_colour.py, tests/noise_slow.py); a helper, not a test.

    v(ch, t)  the finished sample a row without a pulse would hold at absolute sample t: clamp(D(ch, t) + noise(ch, t) + baseline),
              D = 0 where no dark-count rate is set, noise = 0 at and beyond the model's channels
    seed      a sample t of a PMT channel inside the model with v(ch, t) < thr_zle[ch] that lies in no row (l, r) of the channel; its
              start is t itself
    rows      the seeds of a channel -- its lone dark photons (tests/lone_hits.py) and its noise-hit seeds -- merged by start; a
              maximal chain with consecutive starts at most G apart is one row of range first - tw .. last + tlen - 1 + tw, clipped in
              front of the next row of the channel, behind the one before it and at s_limit - 1; owner, look-back, ix_rand and content
              as in tests/lone_hits.py

``rows`` asserts for every chain that it straddles no row, and for every noise-hit seed that it lies inside a stored interval of the
row that holds it.
"""
import numpy as np

from tests import lone_hits as LH
from tests import noise_slow as NS

PHOTON, NOISE = 0, 1            # the kind of a seed; at one start a photon sorts in front of a noise hit


class LoneNoise:
    def __init__(self, lone, model, seed, thr_zle, baseline, n_pmt, photons=True):
        """lone: LH.Lone (its Dark without thresholds: no dark counts anywhere); model: the dict of NS.slow_model (white, coloured or
        with slow levels); thr_zle: the thresholds by channel; n_pmt: PMT channels of the array; photons=False: a pass without rates"""
        self.lone, self.model, self.seed = lone, model, int(seed)
        self.thr, self.baseline, self.n_pmt = np.asarray(thr_zle, dtype=np.int64), int(baseline), int(n_pmt)
        self.tw, self.tlen, self.G = lone.tw, lone.tlen, lone.G
        self.photons_on = bool(photons)
        self._v = {}

    @property
    def channels(self):
        """the PMT channels inside the noise model: those that can have noise-hit seeds"""
        return min(int(self.model['n_channels']), self.n_pmt)

    # ---- the stream value
    def noise(self, ch, t0, n):
        if ch >= int(self.model['n_channels']) or n <= 0:
            return np.zeros(max(int(n), 0), dtype=np.int64)
        return NS.slow_noise_values(self.model, self.seed, ch, int(t0) + np.arange(int(n), dtype=np.int64))

    def dark(self, ch, t0, n):
        return self.lone.dark.samples(ch, int(t0), int(n)) if self.photons_on else np.zeros(int(n), dtype=np.int64)

    def prime(self, ch, a, b):
        """v(ch, a .. b - 1) computed once; ``value`` then serves every range inside it"""
        self._v[ch] = (int(a), self._value(ch, int(a), int(b) - int(a)))

    def _value(self, ch, t0, n):
        return LH.finish(self.dark(ch, t0, n), self.baseline, self.noise(ch, t0, n))

    def value(self, ch, t0, n):
        """v(ch, t0 .. t0 + n - 1)"""
        if ch in self._v:
            a, v = self._v[ch]
            if a <= t0 and t0 + n <= a + len(v):
                return v[t0 - a:t0 - a + n]
        return self._value(ch, int(t0), int(n))

    # ---- seeds
    def crossings(self, ch, a, b):
        """every t in [a, b) with v(ch, t) < thr_zle[ch], in a row or not"""
        if b <= a or ch >= self.channels:
            return np.zeros(0, dtype=np.int64)
        return int(a) + np.flatnonzero(self.value(ch, int(a), int(b) - int(a)) < self.thr[ch]).astype(np.int64)

    def noise_seeds(self, ch, a, b, rows=()):
        t = self.crossings(ch, a, b)
        for l, r in rows:
            t = t[(t < l) | (t > r)]
        return t

    def seeds(self, ch, a, b, rows=()):
        """(start, kind, t_ns, gain) of the channel's seeds with start in [a, b), by (start, kind); t_ns and gain are 0 for a noise hit"""
        if self.photons_on:
            st, t, g = self.lone.photons(ch, a, b)
            keep = np.array([self.lone.is_lone(int(s), rows) for s in st], dtype=bool)
            st, t, g = st[keep], t[keep], g[keep]
        else:
            st, t, g = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
        nz = self.noise_seeds(ch, a, b, rows)
        start = np.concatenate([st, nz]).astype(np.int64)
        kind = np.concatenate([np.full(len(st), PHOTON), np.full(len(nz), NOISE)]).astype(np.int64)
        t_ns, gain = np.concatenate([t, np.zeros(len(nz), np.int64)]), np.concatenate([g, np.zeros(len(nz))])
        o = np.lexsort((t_ns, kind, start))
        return start[o], kind[o], t_ns[o], gain[o]

    # ---- rows of a pass
    def rows(self, ch, s0, s1, s_limit, rows=()):
        """the lone rows of channel ch the pass owns: dicts(channel, left, right, n_photons, n_noise, starts, kinds, t_ns, gain,
        ix_rand) in time order; starts / kinds: every seed of the chain, t_ns / gain: its photons"""
        assert s0 <= s1 <= s_limit
        start, kind, t, g = self.seeds(ch, s0 - self.G, s_limit, rows)
        out, k = [], 0
        while k < len(start):
            j = k + 1
            while j < len(start) and start[j] - start[j - 1] <= self.G:
                j += 1
            first, last = int(start[k]), int(start[j - 1])
            if s0 <= first < s1:
                # two seeds on the two sides of a row of len >= G start at least len + 1 > G apart: a chain straddles no row
                assert not any(first < l and r < last for l, r in rows), (ch, first, last)
                assert all(r - l + 1 >= self.G for l, r in rows)
                left, right = first - self.tw, last + self.tlen - 1 + self.tw
                prev = [r for l, r in rows if r < first]
                nxt = [l for l, r in rows if l > last]
                if prev and max(prev) >= left:
                    left = max(prev) + 1
                if nxt and min(nxt) <= right:
                    right = min(nxt) - 1
                right = min(right, int(s_limit) - 1)
                ph = kind[k:j] == PHOTON
                row = dict(channel=ch, left=left, right=right, n_photons=int(ph.sum()), n_noise=int((~ph).sum()), starts=start[k:j].copy(),
                           kinds=kind[k:j].copy(), t_ns=t[k:j][ph].copy(), gain=g[k:j][ph].copy(), ix_rand=self.lone.ix_rand(ch, left))
                self.check_row(row)
                out.append(row)
            k = j
        return out

    def check_row(self, row):
        """every noise-hit seed of a row is a hit of that row: it lies inside exactly one stored interval"""
        nz = row['starts'][row['kinds'] == NOISE]
        if not len(nz):
            return
        assert row['left'] <= nz.min() and nz.max() <= row['right'], row
        itv = LH.intervals(self.content(row), int(self.thr[row['channel']]), self.tw)
        for s in (nz - row['left']).tolist():
            # (the even landing moves an interval's ends inwards by at most a sample; a hit sits tw inside them, or at an end of the row)
            assert sum(l - 1 <= s <= r + 1 for l, r in itv) == 1, (row['channel'], row['left'] + s, itv)

    def pass_rows(self, channels, s0, s1, s_limit, rows_of=None):
        """every channel's rows of a pass, in (channel, time) order -- the order of Engine.lone_hit_rows; rows_of: {channel: [(l, r)]}"""
        rows_of = rows_of or {}
        return [r for ch in channels for r in self.rows(ch, s0, s1, s_limit, rows_of.get(ch, ()))]

    # ---- content
    def content(self, row):
        """the finished samples of a row: v over its range"""
        return self.value(row['channel'], row['left'], row['right'] - row['left'] + 1)

    def records(self, rows, dt):
        return LH.records_of_rows(rows, [self.content(r) for r in rows], lambda ch: int(self.thr[ch]), self.tw, dt)


def spike_pmf(n_channels, spike, p_spike=2.0 ** -9, small=None, p_small=0.0):
    """(pmf[n_channels][spike + 1], vmin = -spike): almost all mass on 0, p_spike on -spike (a value that crosses the threshold on its
    own) and, where asked for, p_small on -small (one that crosses only together with the tail of a dark pulse)"""
    pmf = np.zeros((int(n_channels), int(spike) + 1), dtype=np.float64)
    pmf[:, 0] = p_spike
    if small is not None:
        pmf[:, int(spike) - int(small)] = p_small
    pmf[:, int(spike)] = 1.0 - pmf.sum(axis=1)
    return pmf, -int(spike)


def model_of(config, n_rows=801):
    """(NS.slow_model, seed) of config['noise_model'] -- white, coloured or with slow levels"""
    from wfsim_amd.config import kernel_params
    from wfsim_amd.noise_model import noise_colour, noise_pmf, noise_slow
    pmf, vmin = noise_pmf(config, n_rows)
    return NS.slow_model(pmf, vmin, noise_colour(config, n_rows), noise_slow(config, n_rows)), int(kernel_params(config)['seed'])


def oracle_records(orc_of, rows, ln, params, noise_of=None, dark_of=None):
    """The unchanged oracle on restated rows.  Every seed of a row is one Pulse call of its own at the sample the seed starts -- a lone
    photon with its restated gain (as LH.oracle_records feeds it), a noise-hit seed as a photon of gain 0, which only spans the row --
    and the calls of a row share one digitise window.  The model's samples are materialised as a noise table with a forced ix_rand per
    window: the oracle's row is samples_to_store_before + before / samples_to_store_after wider than the lone row on either side, and
    the table holds the model's value inside the lone row and 0 outside it (the baseline: no hit; the width in front is even, which the
    callers assert, so the even landing does not move).  Inside the row D must be what the fed photons make (asserted): then what the
    oracle accumulates and the table adds is D + noise.  orc_of(table or None) makes an oracle; noise_of / dark_of (channel, first sample,
    samples): the model's and D's values from elsewhere than the restatement (the device's read-backs).  Returns records by (time, channel)."""
    noise_of, dark_of = noise_of or ln.noise, dark_of or ln.dark
    dt, before, n_tpc = int(params['dt']), int(params['samples_before']), int(params['n_tpc'])
    rows = sorted(rows, key=lambda r: r['left'])

    def feed(orc):
        for k, row in enumerate(rows):
            ph = iter(zip(row['t_ns'].tolist(), row['gain'].tolist()))
            for s, kind in zip(row['starts'].tolist(), row['kinds'].tolist()):
                t, g = next(ph) if kind == PHOTON else ((s + before) * dt, 0.0)
                assert t // dt - before == s
                orc.pulse_call(0, k, np.array([t - before * dt], dtype=np.int64), np.array([row['channel']], dtype=np.int16), np.zeros(1, np.uint8), np.array([g]), True)
            orc.digitize_and_zle(0)
        return orc

    from tests.noise_model import oracle_rows
    plain = feed(orc_of(None)).results()
    mine = [(w, ch, first, length) for w, ch, first, length in oracle_rows(plain) if ch < n_tpc]
    assert [(w, ch) for w, ch, _, _ in mine] == [(k, r['channel']) for k, r in enumerate(rows)]
    longest = max(length for _, _, _, length in mine)
    table = np.zeros(((longest + 8) * len(rows), n_tpc), dtype=np.int16)
    ix = np.arange(len(rows), dtype=np.int64) * (longest + 8)
    for (w, ch, first, length), row in zip(mine, rows):
        assert first <= row['left'] and row['right'] <= first + length - 1 and (row['left'] - first) % 2 == 0
        n = row['right'] - row['left'] + 1
        fed = np.zeros(n, dtype=np.int64)
        for t, g in zip(row['t_ns'].tolist(), row['gain'].tolist()):
            v = -np.rint(g * ln.lone.dark.templates[t % dt] * ln.lone.dark.c2a).astype(np.int64)
            a = t // dt - before - row['left']
            lo, hi = max(a, 0), min(a + ln.tlen, n)
            fed[lo:hi] += v[lo - a:hi - a]
        assert np.array_equal(fed, dark_of(ch, row['left'], n)), 'a dark photon outside the chain reaches the row'
        table[ix[w] + row['left'] - first:ix[w] + row['left'] - first + n, ch] = noise_of(ch, row['left'], n)
    orc = orc_of(table)
    orc.set_noise_override(ix)
    feed(orc)
    from wfsim_amd.dtypes import raw_record_dtype
    rec = np.frombuffer(orc.pack_records().tobytes(), dtype=raw_record_dtype())
    rec = rec[rec['channel'] < n_tpc]
    return rec[np.lexsort((rec['channel'], rec['time']))]


# ---------------------------------------------------------------------------------------------------- designed positions, found by a scan
def seed_table(ln, channels, a, b, rows_of=None):
    """{channel: (start, kind)} of the seeds in [a, b) -- the scan the finders below walk (v is computed once per channel)"""
    out = {}
    for ch in channels:
        ln.prime(ch, a - ln.tlen, b + ln.tlen)
        st, kind, _, _ = ln.seeds(ch, a, b, (rows_of or {}).get(ch, ()))
        out[ch] = (st, kind)
    return out


def find_isolated(table, clear, kind=NOISE, skip=0):
    """(channel, start) of a seed of the kind with no other seed of its channel within `clear` samples (the skip-th such)"""
    for ch, (st, kd) in table.items():
        for k in range(1, len(st) - 1):
            if kd[k] == kind and st[k] - st[k - 1] > clear and st[k + 1] - st[k] > clear:
                if skip == 0:
                    return ch, int(st[k])
                skip -= 1
    raise AssertionError('no isolated seed')


def find_pair(table, gap, clear, kinds=(NOISE, NOISE)):
    """(channel, start) of the first of two consecutive seeds of the kinds exactly `gap` apart, nothing else within `clear` of either"""
    for ch, (st, kd) in table.items():
        for k in range(1, len(st) - 2):
            if (kd[k], kd[k + 1]) == tuple(kinds) and st[k + 1] - st[k] == gap and st[k] - st[k - 1] > clear and st[k + 2] - st[k + 1] > clear:
                return ch, int(st[k])
    raise AssertionError(f'no pair {gap} apart')


def find_inside_pulse(ln, table):
    """(channel, start) of a noise-hit seed inside the pulse of a lone photon of its chain that is not its first sample"""
    for ch, (st, kd) in table.items():
        ph = st[kd == PHOTON]
        for s in st[kd == NOISE].tolist():
            if np.any((ph < s) & (s < ph + ln.tlen)):
                return ch, int(s)
    raise AssertionError('no noise hit inside a pulse')


def find_needs_both(ln, table):
    """(channel, start) of a seed that neither D nor the noise makes on its own: baseline + D and baseline + noise stay at or above the
    threshold, their sum does not"""
    for ch, (st, kd) in table.items():
        for s in st[kd == NOISE].tolist():
            D, nz = int(ln.dark(ch, s, 1)[0]), int(ln.noise(ch, s, 1)[0])
            if D < 0 and nz < 0 and ln.baseline + D >= ln.thr[ch] and ln.baseline + nz >= ln.thr[ch]:
                assert ln.baseline + D + nz < ln.thr[ch]
                return ch, int(s)
    raise AssertionError('no seed made by D and noise together')
