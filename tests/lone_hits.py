"""Lone-hit rows (config 'dark_count_lone_hits', wfs_lone_hits) restated in numpy on top of the ``Dark`` restatement of
tests/dark_counts.py; a helper, not a test.

    start = idx - before: first sample of a dark photon's pulse;  G = tlen + 2 tw
    lone     none of start .. start + tlen - 1 lies in a row (l, r) of the channel
    row      lone photons of a channel in time order, consecutive starts at most G apart: one row of range
             first - tw .. last + tlen - 1 + tw, clipped in front of the next row of the channel and behind the one before it
    owner    the pass [s0, s1) owns the chains whose first photon starts there; a photon at or after s0 with a lone photon at most G in
             front of it (back to s0 - G) begins none; photons at or behind s_limit are not taken, the row ends at s_limit - 1 at the latest
    ix_rand  ((u64) w[0] noise_len) >> 32, w = philox4x32_10(low, high word of the row's first sample, ch, 115); 0 without a table
    content  clamp(D + noise + baseline), then ZLE (hits below thr, hold-off 2 tw + 1, tw on either side clipped into the row, left up and
             right down to an even sample of the row) and fragments of 110 samples

Unlike the device, which looks one window up by bisection, the restatement walks every row it is given: the two agree where the windows
lie more than G apart, which wfs_lone_hits checks.
"""
import numpy as np

from tests.dark_counts import Dark, row_term          # noqa: F401  (Dark: re-exported for the tests)
from tests.noise_model import philox4x32_10

SITE_IX = 115
SPR = 110
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


class Lone:
    def __init__(self, dark, tw, noise_len=0):
        self.dark, self.tw, self.noise_len = dark, int(tw), int(noise_len)
        self.tlen, self.before = dark.tlen, dark.before
        self.G = self.tlen + 2 * self.tw

    # ---- photons
    def photons(self, ch, a, b):
        """(start, t_ns, gain) of the channel's dark photons with start in [a, b), by (start, t_ns)"""
        if b <= a or not self.dark.live(ch):
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
        p = self.dark.photons(ch, (int(a) + self.before) >> 6, (int(b) - 1 + self.before) >> 6)
        start = p['idx'] - self.before
        keep = (start >= a) & (start < b)
        start, t, g = start[keep], p['t_ns'][keep], p['gain'][keep]
        o = np.lexsort((t, start))
        return start[o], t[o], g[o]

    def is_lone(self, start, rows):
        """rows: [(l, r)] final ranges of the channel's rows"""
        return not any(start <= r and start + self.tlen - 1 >= l for l, r in rows)

    # ---- rows of a pass
    def rows(self, ch, s0, s1, s_limit, rows=()):
        """the lone rows of channel ch the pass owns: dicts(channel, left, right, n_photons, starts, t_ns, gain, ix_rand), in time order"""
        assert s0 <= s1 <= s_limit
        start, t, g = self.photons(ch, s0 - self.G, s_limit)
        lone = np.array([self.is_lone(int(s), rows) for s in start], dtype=bool)
        start, t, g = start[lone], t[lone], g[lone]
        out, k = [], 0
        while k < len(start):
            j = k + 1
            while j < len(start) and start[j] - start[j - 1] <= self.G:
                j += 1
            first, last = int(start[k]), int(start[j - 1])
            # (a chain that began in front of s0 -- its first photon is in the look-back -- is another pass's, whole)
            if s0 <= first < s1:
                # a chain never straddles a row: a row holds a pulse (or spans a window) and is at least G long
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
                out.append(dict(channel=ch, left=left, right=right, n_photons=j - k, starts=start[k:j].copy(), t_ns=t[k:j].copy(), gain=g[k:j].copy(),
                                ix_rand=self.ix_rand(ch, left)))
            k = j
        return out

    def ix_rand(self, ch, left):
        if self.noise_len <= 0:
            return 0
        u = np.asarray([left], dtype=np.int64).view(np.uint64)
        w0 = philox4x32_10(u & _LOW, u >> _S32, np.uint64(ch), np.uint64(SITE_IX), self.dark.seed)[0].astype(np.uint64)
        return int((w0[0] * np.uint64(self.noise_len)) >> _S32)

    def pass_rows(self, channels, s0, s1, s_limit, rows_of=None):
        """every channel's rows of a pass, in (channel, time) order -- the order of Engine.lone_hit_rows; rows_of: {channel: [(l, r)]}"""
        rows_of = rows_of or {}
        return [r for ch in channels for r in self.rows(ch, s0, s1, s_limit, rows_of.get(ch, ()))]

    # ---- content
    def term(self, row):
        """D over the row: every dark photon that reaches a sample, the tail of one that is not lone included"""
        return self.dark.samples(row['channel'], row['left'], row['right'] - row['left'] + 1)


def finish(term, baseline, noise=None, float_noise=False):
    """the finished samples of wfs_rows.h for a TPC row: accumulated + noise + baseline, clamped at 0; a float table adds in floating
    point and stores the truncated sum"""
    v = np.asarray(term, dtype=np.int64)
    if noise is not None:
        v = (v.astype(np.float64) + noise).astype(np.int64) if float_noise else v + np.asarray(noise, dtype=np.int64)
    return np.maximum(v + int(baseline), 0)


def intervals(data, thr, tw):
    """[(left, right)] relative to the row: hits below thr, two hits at most 2 tw + 1 apart share an interval; tw on either side,
    clipped into the row, left up and right down to an even sample"""
    hits = np.flatnonzero(np.asarray(data) < thr)
    if not len(hits):
        return []
    hold = max(2 * tw + 1, 1)
    cut = np.flatnonzero(np.diff(hits) > hold) + 1
    out, n = [], len(data)
    for grp in np.split(hits, cut):
        l, r = int(np.clip(grp[0] - tw, 0, n - 1)), int(np.clip(grp[-1] + tw, 0, n - 1))
        out.append(((l + 1) // 2 * 2, r // 2 * 2))
    return out


def records_of_rows(rows, data, thr_of, tw, dt):
    """raw_records of finished rows (rows[k] with samples data[k]) in (time, channel) order; thr_of(channel): the ZLE threshold"""
    from wfsim_amd.dtypes import raw_record_dtype
    recs = []
    for row, d in zip(rows, data):
        assert len(d) == row['right'] - row['left'] + 1
        for l, r in intervals(d, thr_of(row['channel']), tw):
            plen = r - l + 1
            if plen <= 0:
                continue
            n = -(-plen // SPR)
            rec = np.zeros(n, dtype=raw_record_dtype())
            for i in range(n):
                m = min(plen, SPR * (i + 1)) - SPR * i
                rec['time'][i], rec['length'][i], rec['dt'][i], rec['channel'][i] = dt * (row['left'] + l + SPR * i), m, dt, row['channel']
                rec['pulse_length'][i], rec['record_i'][i] = plen, i
                rec['data'][i][:m] = d[l + SPR * i:l + SPR * i + m].astype(np.int16)
            recs.append(rec)
    from wfsim_amd.dtypes import raw_record_dtype as _rd
    out = np.concatenate(recs) if recs else np.zeros(0, dtype=_rd())
    return out[np.lexsort((out['channel'], out['time']))]


def sort_records(rec):
    return rec[np.lexsort((rec['record_i'], rec['channel'], rec['time']))]


def oracle_records(orc, rows, n_tpc, before, dt):
    """The unchanged oracle on the restated lone rows: every photon of a row is one Pulse call of its own (a pulse of its own, rounded on
    its own, as D rounds it), the calls of a row share one digitise window, with the restated gains and the restated times moved
    `before` samples down: the reference writes a photon's template from sample t // dt on (pulse.py:305-308), a dark photon's runs
    from idx - before on -- a whole number of samples, the remainder stays.  The oracle's pulse is samples_to_store_before +
    before / samples_to_store_after wider than a lone row on either side -- samples at the baseline without noise, which make no hit
    and, the width in front being even (the callers assert it), do not move the even landing -- and a top PMT gets an HE row and a
    bottom PMT a share of the sum row, which lone hits do not have: the records of the TPC channels are compared.  One row per oracle
    window, so no two channels share a window.  Returns records by (time, channel)."""
    for k, row in enumerate(sorted(rows, key=lambda r: r['left'])):
        for t, g in zip(row['t_ns'].tolist(), row['gain'].tolist()):
            orc.pulse_call(0, k, np.array([t - before * dt], dtype=np.int64), np.array([row['channel']], dtype=np.int16), np.zeros(1, np.uint8), np.array([g]), True)
        orc.digitize_and_zle(0)
    from wfsim_amd.dtypes import raw_record_dtype
    rec = np.frombuffer(orc.pack_records().tobytes(), dtype=raw_record_dtype())
    rec = rec[rec['channel'] < n_tpc]
    return rec[np.lexsort((rec['channel'], rec['time']))]
