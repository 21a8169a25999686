"""PMT dark counts (config 'dark_count_rate', wfs_set_dark_counts) restated in numpy; a helper, not a test.

    L = 64, m = cell of a channel's absolute sample axis (samples 64 m .. 64 m + 63; numpy's >> on int64 is arithmetic)
    w    = philox4x32_10(counter (low 32 bits of m, high 32 bits of m, ch, 112), key = seed)
    n    = sum_{k = 1 .. 4} [w[0] < T[ch][k]]                       (T: the thresholds, an ARGUMENT here -- the device's own)
    photon j < n: W = the call at site 113 + (j >> 1), a = 2 (j & 1)
        t_ns = m L dt + ((W[a] * (L dt)) >> 32),  gain = gains[ch] * spe_row[ch][((W[a + 1] * 2000) >> 32) + 1]
        idx = t_ns // dt, r = t_ns % dt;  sample idx - before + k, k < tlen, gets -rint(gain * templates[r][k] * c2a)
    D(ch, t) = the sum over the channel's photons that reach t

``materialise`` writes D into a noise table with one stretch per digitise window (the layout of tests/noise_model.materialise), on top
of the values another materialiser put there; the UNCHANGED oracle, replaying that table from forced ix_rand, gives the records an
engine with dark counts must produce.
"""
import numpy as np

from tests.noise_model import philox4x32_10

L = 64
SITE_COUNT, SITE_PHOTON = 112, 113
SPE_BINS = 2000
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


class Dark:
    """everything the rule reads, taken from an Engine (its tables and parameters) or given by hand"""

    def __init__(self, seed, dt, before, tlen, c2a, templates, spe, gains, thr):
        self.seed, self.dt, self.before, self.tlen, self.c2a = int(seed), int(dt), int(before), int(tlen), float(c2a)
        self.templates = np.asarray(templates, dtype=np.float64).reshape(self.dt, self.tlen)
        self.spe = np.asarray(spe, dtype=np.float64)
        self.gains = np.asarray(gains, dtype=np.float64)
        self.thr = np.asarray(thr, dtype=np.uint64)              # [n_channels][4]
        self._cache = {}

    @classmethod
    def of_engine(cls, eng, thr=None):
        p, t = eng.params, eng.tables
        if thr is None:
            n = len(eng.dark_count_rate) if eng.dark_count_rate is not None else 0
            thr = np.stack([eng.dark_count_thresholds(c) for c in range(n)]) if n else np.zeros((0, 4), dtype=np.uint32)
        return cls(p['seed'], p['dt'], p['samples_before'], p['tlen'], p['c2a'], t['templates'], t['spe'], t['gains'], thr)

    @classmethod
    def of_config(cls, config, thr):
        """without a device: the tables the host builds for the oracle (tests/helpers.host_tables), thresholds given"""
        from tests.helpers import host_tables
        from wfsim_amd.config import kernel_params
        p, t = kernel_params(config), host_tables(config)
        return cls(p['seed'], p['dt'], p['samples_before'], p['tlen'], p['c2a'], t['templates'], t['spe'], t['gains'], thr)

    def spe_row(self, ch):
        return self.spe[ch if self.spe.shape[0] > 1 else 0]

    def live(self, ch):
        return 0 <= ch < len(self.thr) and int(self.thr[ch][0]) > 0 and self.gains[ch] != 0.0

    def _call(self, ch, m, site):
        mu = np.asarray(m, dtype=np.int64).view(np.uint64)
        return philox4x32_10(mu & _LOW, mu >> _S32, np.uint64(ch), np.uint64(site), self.seed)

    def counts(self, ch, m):
        """n(ch, m) for every cell of the int64 array m"""
        m = np.atleast_1d(np.asarray(m, dtype=np.int64))
        if not self.live(ch):
            return np.zeros(len(m), dtype=np.int64)
        w0 = self._call(ch, m, SITE_COUNT)[0].astype(np.uint64)
        return sum((w0 < self.thr[ch][k]).astype(np.int64) for k in range(4))

    def photons(self, ch, m_lo, m_hi):
        """the photons of the cells m_lo .. m_hi of a channel, cells ascending, j ascending inside a cell:
        dict(m, j, t_ns, gain, idx, r) of int64 / float64 arrays"""
        key = (ch, int(m_lo), int(m_hi))
        if key in self._cache:
            return self._cache[key]
        m = np.arange(int(m_lo), int(m_hi) + 1, dtype=np.int64)
        n = self.counts(ch, m)
        cells = np.repeat(m, n)
        j = np.concatenate([np.arange(k) for k in n]).astype(np.int64) if len(cells) else np.zeros(0, dtype=np.int64)
        span = np.uint64(L * self.dt)
        t_ns, gain = np.zeros(len(cells), dtype=np.int64), np.zeros(len(cells), dtype=np.float64)
        for pair in (0, 1):
            sel = (j >> 1) == pair
            if not sel.any():
                continue
            W = self._call(ch, cells[sel], SITE_PHOTON + pair).astype(np.uint64)
            a = 2 * (j[sel] & 1)
            k = np.arange(int(sel.sum()))
            off = ((W[a, k] * span) >> _S32).astype(np.int64)
            code = ((W[a + 1, k] * np.uint64(SPE_BINS)) >> _S32).astype(np.int64) + 1
            t_ns[sel] = cells[sel] * (L * self.dt) + off
            gain[sel] = self.gains[ch] * self.spe_row(ch)[code]
        out = dict(m=cells, j=j, t_ns=t_ns, gain=gain, idx=t_ns // self.dt, r=t_ns % self.dt)
        self._cache[key] = out
        return out

    def photons_in(self, ch, t0, n):
        """(t_ns, gain) of the photons whose idx lies in [t0, t0 + n), in time order (equal times: in the order of j)"""
        if n <= 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
        p = self.photons(ch, int(t0) >> 6, (int(t0) + int(n) - 1) >> 6)
        keep = (p['idx'] >= t0) & (p['idx'] < t0 + n)
        t, g = p['t_ns'][keep], p['gain'][keep]
        order = np.argsort(t, kind='stable')
        return t[order], g[order]

    def samples(self, ch, t0, n):
        """D(ch, t0 .. t0 + n - 1) as int64"""
        D = np.zeros(int(n), dtype=np.int64)
        if n <= 0 or not self.live(ch):
            return D
        p = self.photons(ch, (int(t0) + self.before - self.tlen + 1) >> 6, (int(t0) + int(n) - 1 + self.before) >> 6)
        for idx, r, g in zip(p['idx'].tolist(), p['r'].tolist(), p['gain'].tolist()):
            v = -np.rint(g * self.templates[r] * self.c2a).astype(np.int64)        # a pulse of its own, rounded on its own
            first = idx - self.before - int(t0)
            lo, hi = max(first, 0), min(first + self.tlen, int(n))
            if lo < hi:
                D[lo:hi] += v[lo - first:hi - first]
        return D


def pmt_channel(ch, params):
    """the PMT whose dark counts the row of a channel gets, or -1: an HE channel its top PMT, the sum channel none"""
    n_tpc, he_first, n_top = int(params['n_tpc']), int(params['he_first']), int(params['n_top'])
    if ch < n_tpc:
        return ch
    if params['detector_nt'] and he_first <= ch < he_first + n_top:
        return ch - he_first
    return -1


def row_term(dark, params, ch, first, length):
    """what the dark counts add to the FINISHED sum of a row in front of noise and baseline: D, times int(he_factor) in an HE row"""
    c = pmt_channel(ch, params)
    if c < 0 or not dark.live(c):
        return np.zeros(int(length), dtype=np.int64)
    D = dark.samples(c, first, length)
    return D * int(params['he_factor']) if ch >= int(params['n_tpc']) else D


def layout(rows, n_windows, pad=8):
    """the stretches of tests/noise_model.materialise: (ix_rand int64[n_windows], table length)"""
    longest = np.zeros(n_windows, dtype=np.int64)
    seen = set()
    for w, ch, first, length in rows:
        assert (w, ch) not in seen, 'one row per (window, channel)'
        seen.add((w, ch))
        longest[w] = max(longest[w], length)
    return np.concatenate([[0], np.cumsum(longest + pad)])[:-1].astype(np.int64), max(int((longest + pad).sum()), 1)


def materialise(rows, n_windows, dark, params, n_columns, base=None, pad=8):
    """rows: (window, channel, first absolute sample, length) of every row of a run.  Returns (table[N][n_columns], ix_rand
    int64[n_windows]) with table[ix_rand[g] + k, ch] = base[ix_rand[g] + k, ch] + row_term(ch, row_abs(g, ch) + k): the dark counts
    on top of the noise another materialiser wrote into the same stretches (``base``: its table, int16 or float64; None: no noise).
    An HE column gets int(he_factor) D(top channel); columns at or beyond n_columns are left out, as their noise is."""
    ix, N = layout(rows, n_windows, pad)
    if base is None:
        table = np.zeros((N, int(n_columns)), dtype=np.int64)
    else:
        assert base.shape[0] == N and base.shape[1] <= n_columns
        table = np.zeros((N, int(n_columns)), dtype=np.float64 if base.dtype.kind == 'f' else np.int64)
        table[:, :base.shape[1]] = base
    for w, ch, first, length in rows:
        if ch < n_columns:
            table[ix[w]:ix[w] + length, ch] += row_term(dark, params, ch, first, length)
    if table.dtype.kind == 'f':
        return table, ix
    assert np.abs(table).max(initial=0) < 2 ** 15
    return table.astype(np.int16), ix


def stretches_of_table(rows, n_windows, noise, starts, pad=8):
    """what a recorded table adds to the rows of a run whose window g reads it from starts[g]: the same values laid out as
    ``materialise`` lays them out, table[ix_rand[g] + k, ch] = noise[(starts[g] + k) mod len, ch]"""
    ix, N = layout(rows, n_windows, pad)
    out = np.zeros((N, noise.shape[1]), dtype=noise.dtype)
    for w, ch, first, length in rows:
        if ch < noise.shape[1]:
            out[ix[w]:ix[w] + length, ch] = noise[(int(starts[w]) + np.arange(length)) % len(noise), ch]
    return out


def dark_hits(dark, params, rows, zle_adc, quiet_intervals):
    """rows (as above) that hold a dark pulse crossing the ZLE threshold where no instruction pulse is: a sample whose row term alone
    lies more than zle_adc counts below the baseline, outside every interval of the run without dark counts and without noise
    (quiet_intervals: {channel: [(first absolute sample, length)]}).  Shown by the restatement alone."""
    out = []
    for w, ch, first, length in rows:
        term = row_term(dark, params, ch, first, length)
        hit = term < -int(zle_adc)
        for a, n in quiet_intervals.get(ch, ()):
            hit[max(a - first, 0):max(a + n - first, 0)] = False
        if hit.any():
            out.append((w, ch, first, length))
    return out
