"""The overlay rule (wfsim_amd/csrc/wfs_overlay.h) restated twice in numpy, the designed cases and a seeded random generator.

A pulse here is (channel, s0, samples): the int16 samples from absolute sample s0 on.  A stream is a list of pulses of which no two
share a sample on a channel.  ``merge_intervals`` sweeps the pulses of a channel in the order of their starts with the running maximum
of their ends; ``merge_dense`` lays both streams on a dense [channel, sample] array with coverage masks and link masks (a link between
s and s + 1: one pulse covers both) and reads the merged pulses off as the runs of linked samples.  Neither knows the other.
"""
import numpy as np

from wfsim_amd.dtypes import raw_record_dtype

SPR = 110
DTYPE = np.dtype(raw_record_dtype())
EPOCH = 1_700_000_000_000_000_000          # ns: times at the scale of a recorded run


def clamp(v):
    return np.clip(v, 0, 32767)


def fragments(pulses, dt):
    """the records of a list of pulses in (time, channel) order: fragments of 110 samples, the last what is left, zeros behind it"""
    n = sum((len(d) + SPR - 1) // SPR for _, _, d in pulses)
    rec = np.zeros(n, dtype=DTYPE)
    k = 0
    for ch, s0, d in pulses:
        d = np.asarray(d)
        assert len(d) >= 1
        for f in range((len(d) + SPR - 1) // SPR):
            part = d[SPR * f:SPR * (f + 1)]
            r = rec[k]
            r['time'], r['length'], r['dt'], r['channel'] = (s0 + SPR * f) * dt, len(part), dt, ch
            r['pulse_length'], r['record_i'] = len(d), f
            r['data'][:len(part)] = part
            k += 1
    return sort_records(rec)


def sort_records(rec):
    return rec[np.lexsort((rec['channel'], rec['time']))]


def pulses_of(rec, dt):
    """the pulses of a valid stream of records"""
    out = {}
    for r in rec[np.lexsort((rec['time'], rec['channel']))]:
        s0 = int(r['time']) // dt - SPR * int(r['record_i'])
        out.setdefault((int(r['channel']), s0), []).append(r['data'][:r['length']])
    return [(ch, s0, np.concatenate(parts)) for (ch, s0), parts in sorted(out.items())]


def merge_intervals(A, B, baseline, base, dt):
    """the rule by intervals; base: the recorded baseline of a channel, a dict or an array"""
    out = []
    for ch in sorted({p[0] for p in A} | {p[0] for p in B}):
        ps = sorted([(s0, 0, np.asarray(d, dtype=np.int64)) for c, s0, d in A if c == ch] +
                    [(s0, 1, np.asarray(d, dtype=np.int64)) for c, s0, d in B if c == ch], key=lambda p: (p[0], p[1]))
        groups, end = [], None
        for p in ps:
            if end is None or p[0] > end:           # shares no sample with those in front (touching: p[0] == end + 1)
                groups.append([])
                end = p[0] + len(p[2]) - 1
            groups[-1].append(p)
            end = max(end, p[0] + len(p[2]) - 1)
        for g in groups:
            s0 = g[0][0]
            n = max(p[0] + len(p[2]) for p in g) - s0
            val = np.zeros((2, n), dtype=np.int64)
            cov = np.zeros((2, n), dtype=bool)
            for ps0, stream, d in g:
                assert not cov[stream, ps0 - s0:ps0 - s0 + len(d)].any(), 'a stream whose pulses share a sample'
                val[stream, ps0 - s0:ps0 - s0 + len(d)] = d
                cov[stream, ps0 - s0:ps0 - s0 + len(d)] = True
            assert (cov[0] | cov[1]).all()
            v = np.where(cov[0] & cov[1], clamp(val[1] + val[0] - baseline), np.where(cov[0], clamp(val[0] - baseline + int(base[ch])), val[1]))
            out.append((ch, s0, v.astype(np.int16)))
    return fragments(out, dt)


def merge_dense(A, B, baseline, base, dt):
    """the rule by brute force on a dense [channel, sample] array"""
    both = list(A) + list(B)
    if not both:
        return np.zeros(0, dtype=DTYPE)
    chs = sorted({p[0] for p in both})
    lo = min(p[1] for p in both)
    n = max(p[1] + len(p[2]) for p in both) - lo
    val = np.zeros((2, len(chs), n), dtype=np.int64)
    cov = np.zeros((2, len(chs), n), dtype=bool)
    link = np.zeros((len(chs), n), dtype=bool)           # link[c, s]: one pulse covers s and s + 1
    for stream, S in enumerate((A, B)):
        for ch, s0, d in S:
            c, a = chs.index(ch), s0 - lo
            val[stream, c, a:a + len(d)] = d
            cov[stream, c, a:a + len(d)] = True
            link[c, a:a + len(d) - 1] = True
    out = []
    for c, ch in enumerate(chs):
        covered = cov[0, c] | cov[1, c]
        v = np.zeros(n, dtype=np.int64)
        only_b, only_a, ab = cov[1, c] & ~cov[0, c], cov[0, c] & ~cov[1, c], cov[0, c] & cov[1, c]
        v[only_b] = val[1, c][only_b]
        v[only_a] = clamp(val[0, c][only_a] - baseline + int(base[ch]))
        v[ab] = clamp(val[1, c][ab] + val[0, c][ab] - baseline)
        s = 0
        while s < n:
            if not covered[s]:
                s += 1
                continue
            e = s
            while link[c, e]:
                e += 1
            out.append((ch, lo + s, v[s:e + 1].astype(np.int16)))
            s = e + 1
    return fragments(out, dt)


def no_shared_samples(rec, dt):
    """no two pulses of a record stream share a sample on a channel, and every pulse is complete"""
    ps = pulses_of(rec, dt)
    for (c0, s0, d0), (c1, s1, _) in zip(ps, ps[1:]):
        if c0 == c1 and s0 + len(d0) > s1:
            return False
    return all(len(d) == int(rec[(rec['channel'] == ch) & (rec['time'] == s0 * dt)]['pulse_length'][0]) for ch, s0, d in ps)


# ---------------------------------------------------------------------------------------------------- designed cases
def _sig(rng, n, level, depth=300):
    """n samples about `level` with a dip (PMT signals go down)"""
    d = level + rng.integers(-3, 4, size=n)
    k = int(rng.integers(0, n))
    d[k:k + 7] -= int(rng.integers(20, depth))
    return d.astype(np.int16)


def designed_cases(chs, baseline, t0=EPOCH // 10):
    """name -> (A, B, base overrides {channel: value}).  chs: the channels to use -- dict(first=0, last_tpc=.., he=.., sum=..); t0: first sample"""
    rng = np.random.default_rng(20240521)
    c0, c1, che, chs_ = chs['first'], chs['last_tpc'], chs['he'], chs['sum']
    A = lambda ch, s, n, level=baseline: (ch, t0 + s, _sig(rng, n, level))          # noqa: E731
    Bp = lambda ch, s, n, level=baseline: (ch, t0 + s, _sig(rng, n, level))         # noqa: E731
    cases = {}
    cases['front_one_sample'] = ([A(c0, 100, 50)], [Bp(c0, 60, 41)], {})               # B's last sample is A's first
    cases['back_one_sample'] = ([A(c0, 100, 50)], [Bp(c0, 149, 30)], {})               # B's first sample is A's last
    cases['touching'] = ([A(c0, 100, 50)], [Bp(c0, 60, 40), Bp(c0, 150, 30)], {})      # end + 1 == start on either side: three pulses
    cases['b_inside_a'] = ([A(c0, 0, 300)], [Bp(c0, 120, 20)], {})
    cases['a_inside_b'] = ([A(c0, 120, 20)], [Bp(c0, 0, 300)], {})
    cases['chain_abab'] = ([A(c0, 0, 100), A(c0, 180, 100)], [Bp(c0, 90, 100), Bp(c0, 270, 100)], {})
    for n in (109, 110, 111, 220, 221):
        cases[f'merged_{n}'] = ([A(c0, 0, 60)], [Bp(c0, 59, n - 59)], {})
    cases['offset_1'] = ([A(c0, 1, 330)], [Bp(c0, 0, 331)], {})                        # A's fragments one sample behind the output's
    cases['offset_109'] = ([A(c0, 109, 330)], [Bp(c0, 0, 250)], {})
    cases['five_against_one'] = ([A(c0, 0, 520)], [Bp(c0, 515, 30)], {})
    cases['channels'] = ([A(c, 10 * k, 150) for k, c in enumerate((c0, c1, che, chs_))], [Bp(c, 10 * k + 100, 150) for k, c in enumerate((c0, c1, che, chs_))], {})
    cases['equal_times'] = ([A(c0, 0, 130), A(c0 + 1, 0, 130)], [Bp(c0, 50, 130), Bp(c0 + 1, 50, 130)], {})
    cases['epoch'] = ([(c0, EPOCH // 10 + 5, _sig(rng, 200, baseline)), (c1, EPOCH // 10 + 5, _sig(rng, 200, baseline))],
                      [(c0, EPOCH // 10 + 100, _sig(rng, 200, baseline)), (c1, EPOCH // 10 - 50, _sig(rng, 100, baseline))], {})
    lo_a = np.full(40, 100, dtype=np.int16)                    # a far below the baseline on a low b: the sum is negative
    hi_a = np.full(40, 32000, dtype=np.int16)                  # a far above on a high b: beyond 32767
    cases['clamp'] = ([(c0, t0, lo_a), (c0 + 1, t0, hi_a), (c0 + 2, t0, hi_a)],
                      [(c0, t0 + 10, np.full(40, 50, dtype=np.int16)), (c0 + 1, t0 + 10, np.full(40, 30000, dtype=np.int16))], {c0 + 2: 32000})
    cases['base'] = ([A(c0, 0, 150), A(c0 + 1, 0, 150), A(c1, 0, 150)], [Bp(c0, 100, 150, baseline - 900), Bp(c1, 100, 150, baseline + 700)],
                     {c0: baseline - 900, c1: baseline + 700})
    cases['lone_pulses'] = ([A(c0, 0, 230)], [Bp(c0 + 1, 0, 115), Bp(c0, 1000, 5)], {})   # nothing shares a sample: still written by the rule
    return cases


def random_streams(seed, n_pulses=200, channels=8, span=60000, t0=EPOCH // 10, baseline=16000, base_level=None):
    """two valid streams of n_pulses pulses each on `channels` channels: lengths 1 .. 400, placed by rejection so that the pulses of
    one stream share no sample; some touch"""
    rng = np.random.default_rng(seed)
    streams = []
    for stream in range(2):
        used = np.zeros((channels, span), dtype=bool)
        ps = []
        while len(ps) < n_pulses:
            ch, n = int(rng.integers(0, channels)), int(rng.choice([1, 2, 30, 109, 110, 111, 250, 400]))
            s = int(rng.integers(0, span - n))
            if ps and rng.random() < 0.2:                       # right behind an earlier pulse of the stream: touching
                c_, s_, d_ = ps[int(rng.integers(0, len(ps)))]
                ch, s = c_, s_ - t0 + len(d_)
                if s + n > span:
                    continue
            if used[ch, s:s + n].any():
                continue
            used[ch, s:s + n] = True
            level = baseline if stream == 0 or base_level is None else int(base_level[ch])
            ps.append((ch, t0 + s, _sig(rng, n, level)))
        streams.append(ps)
    return streams


def base_array(n_rows, baseline, overrides):
    b = np.full(n_rows, baseline, dtype=np.int32)
    for ch, v in overrides.items():
        b[ch] = v
    return b
