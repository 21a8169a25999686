"""The noise model (config 'noise_model', wfs_set_noise_model) restated in numpy; a helper, not a test.

    q    = t >> 2                                  (t: absolute sample index, signed 64 bit, arithmetic shift)
    w[4] = philox4x32_10(counter (low 32 bits of q, high 32 bits of q, ch, 65), key = seed)
    noise(ch, t) = vmin + alias_sample(cells[ch], w[t & 3])

alias_sample: cell c = word >> shift, value c if (word << (32 - shift)) mod 2^32 < thr[c], else alias[c].  The cells come from
``build_alias``, a transcription of the host's construction (wfs_engine.hip build_alias).  The Philox here is vectorised numpy;
``philox_matches_oracle`` compares it with oracle.oracle.philox, which tests/test_oracle_golden.py pins on the Random123 known answers.

``materialise`` turns the model into what the table-noise path adds exactly the same values from: an int16 table with one stretch
per digitise window and the window's start index, given the rows of a run (row geometry does not depend on noise).
"""
import numpy as np

SITE_NOISE_SAMPLE = 65
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, seed):
    """vectorised Philox4x32-10: counters as arrays (or scalars) of uint32 values, key = (low, high 32 bits of seed); returns uint32[4][n]"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _LOW for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LOW, n2, p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def philox_matches_oracle(seed, counters):
    """the vectorised Philox against the oracle's, counter by counter"""
    from oracle.oracle import philox
    ctr = np.asarray(counters, dtype=np.uint64)
    got = philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], seed)
    key = [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    return all(np.array_equal(got[:, k], philox([int(x) for x in ctr[k]], key)) for k in range(len(ctr)))


def build_alias(pmf_row):
    """(thr uint32[K], alias uint32[K], shift) of one channel: Vose's construction in the host's fixed order, on the running sums of the
    row as the host forms them (cum[i] - cum[i - 1], not the entries themselves)"""
    cum = np.cumsum(np.asarray(pmf_row, dtype=np.float64))        # (sequential additions, as the host's loop)
    n = len(cum)
    K, lg = 2, 1
    while K < n:
        K, lg = K * 2, lg + 1
    q = [0.0] * K
    for i in range(n):
        q[i] = float(cum[i] - (cum[i - 1] if i else 0.0)) * float(K)
    small, large = [i for i in range(K) if q[i] < 1.0], [i for i in range(K) if not q[i] < 1.0]
    thr, alias = [0xFFFFFFFF] * K, list(range(K))
    while small and large:
        s = small.pop()
        big = large[-1]
        t = q[s] * 4294967296.0
        thr[s] = 0xFFFFFFFF if t >= 4294967295.0 else int(t)
        alias[s] = big
        q[big] = (q[big] + q[s]) - 1.0
        if q[big] < 1.0:
            large.pop()
            small.append(big)
    return np.asarray(thr, dtype=np.uint32), np.asarray(alias, dtype=np.uint32), 32 - lg


def build_cells(pmf):
    """cells of every channel of a model: (thr[n_channels][K], alias[n_channels][K], shift)"""
    rows = [build_alias(r) for r in np.asarray(pmf)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), rows[0][2]


def cells_pmf(thr, alias, n_values):
    """the mass every value receives from a channel's cells over the 2^32 words, counted exactly: K = 2^lg cells of equal weight; in
    cell c the word's low 32 - lg bits, left aligned, take the values j << lg, j < 2^(32 - lg), of which ceil(thr[c] / 2^lg) lie below
    the threshold and give c, the others alias[c]"""
    K = len(thr)
    mass = np.zeros(max(K, n_values), dtype=np.float64)
    lg = int(np.log2(K))
    own = np.ceil(thr.astype(np.float64) / 2.0 ** lg) / 2.0 ** (32 - lg)
    for c in range(K):
        mass[c] += own[c] / K
        mass[int(alias[c])] += (1.0 - own[c]) / K
    return mass


def alias_sample(thr, alias, shift, words):
    """values (without vmin) of the 32-bit words drawn from one channel's cells"""
    w = np.asarray(words, dtype=np.uint64) & _LOW
    c = (w >> np.uint64(shift)).astype(np.int64)
    low = (w << np.uint64(32 - shift)) & _LOW
    return np.where(low < thr[c].astype(np.uint64), c, alias[c].astype(np.int64))


def noise_values(cells, shift, vmin, seed, channel, t_array):
    """noise(channel, t) for every t of t_array (int64); cells = (thr[K], alias[K]) of the channel"""
    t = np.asarray(t_array, dtype=np.int64)
    q = t >> 2                                                   # (numpy's >> on int64 is arithmetic)
    uq, inv = np.unique(q, return_inverse=True)                   # one call serves four consecutive t
    qu = uq.view(np.uint64)
    w = philox4x32_10(qu & _LOW, qu >> _S32, np.uint64(channel), np.uint64(SITE_NOISE_SAMPLE), seed)
    word = w[(t & 3).astype(np.int64), inv]
    return (int(vmin) + alias_sample(cells[0], cells[1], shift, word)).astype(np.int64)


def oracle_rows(res):
    """the rows of Oracle.results() as (window, channel, first absolute sample, length)"""
    out = []
    for w in range(len(res['dg_left'])):
        for r in range(int(res['dg_row_off'][w]), int(res['dg_row_off'][w + 1])):
            out.append((w, int(res['row_ch'][r]), int(res['dg_left'][w] + res['row_left'][r]), int(res['row_right'][r] - res['row_left'][r] + 1)))
    return out


def materialise(rows, n_windows, pmf, vmin, seed, n_columns=None, pad=8):
    """rows: (window, channel, first absolute sample, length) of every row of a run, sum rows included under their channel.
    Returns (table int16[N][n_columns], ix_rand int64[n_windows]): one stretch of the table per window, ix_rand[g] its start and
    table[ix_rand[g] + k, ch] = noise(ch, row_abs(g, ch) + k) -- what the table-noise path adds at sample k of the row is the model's
    value.  Rows of channels outside the model are left out (they get no noise either way); a (window, channel) pair is one row."""
    pmf = np.asarray(pmf, dtype=np.float64)
    n_columns = pmf.shape[0] if n_columns is None else int(n_columns)
    thr, alias, shift = build_cells(pmf)
    longest = np.zeros(n_windows, dtype=np.int64)
    seen = set()
    for w, ch, first, length in rows:
        assert (w, ch) not in seen, 'one row per (window, channel)'
        seen.add((w, ch))
        longest[w] = max(longest[w], length)
    ix_rand = np.concatenate([[0], np.cumsum(longest + pad)])[:-1].astype(np.int64)
    N = max(int((longest + pad).sum()), 1)
    table = np.zeros((N, n_columns), dtype=np.int16)
    for w, ch, first, length in rows:
        if ch >= min(n_columns, pmf.shape[0]):
            continue
        v = noise_values((thr[ch], alias[ch]), shift, vmin, seed, ch, first + np.arange(length, dtype=np.int64))
        table[ix_rand[w]:ix_rand[w] + length, ch] = v
    return table, ix_rand


# ---------------------------------------------------------------------------------------------------- statistics
# The inputs of the statistical checks, shared by tests/test_noise_model_cpu.py (the restatement) and tests/test_gpu_noise_model.py
# (Engine.noise_samples): a fixed seed, 2^20 consecutive samples of two channels.  The bounds are the issue's: chi-square against the
# pmf with p > 1e-4, autocorrelation at lags 1 .. 8 and the correlation between the two channels within 5 / sqrt(n).
STAT_SEED = 20261019
STAT_N = 1 << 20
STAT_T0 = 123456789
STAT_CHANNELS = (3, 250)


def chi_square_p(samples, pmf_row, vmin):
    """p-value of the chi-square test of the samples against the pmf; values of expectation below 5 are pooled into one bin, a sample
    outside the support of the pmf gives 0"""
    from scipy.stats import chi2
    s = np.asarray(samples, dtype=np.int64) - int(vmin)
    n_val = len(pmf_row)
    if s.min() < 0 or s.max() >= n_val:
        return 0.0
    obs = np.bincount(s, minlength=n_val).astype(np.float64)
    exp = np.asarray(pmf_row, dtype=np.float64) * len(s)
    if np.any(obs[exp == 0] > 0):
        return 0.0
    big = exp >= 5
    o, e = list(obs[big]), list(exp[big])
    if exp[~big].sum() > 0:
        o.append(obs[~big].sum()); e.append(exp[~big].sum())
    o, e = np.asarray(o), np.asarray(e)
    if len(o) < 2:
        return 1.0 if np.array_equal(o, e) else 0.0
    return float(chi2.sf(((o - e) ** 2 / e).sum(), len(o) - 1))


def correlations(a, b, lags=8):
    """(autocorrelation of a at lags 1 .. lags, correlation of a and b)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a - a.mean(), b - b.mean()
    va = (a * a).mean()
    auto = [float((a[k:] * a[:-k]).mean() / va) for k in range(1, lags + 1)]
    return auto, float((a * b).mean() / np.sqrt(va * (b * b).mean()))


def assert_white(sa, sb, pmf_a, pmf_b, vmin):
    n = len(sa)
    pa, pb = chi_square_p(sa, pmf_a, vmin), chi_square_p(sb, pmf_b, vmin)
    auto, cross = correlations(sa, sb)
    print(f'chi-square p {pa:.4g} {pb:.4g}; autocorrelation {auto}; cross {cross:.3g}; bound {5 / np.sqrt(n):.3g}')
    assert pa > 1e-4 and pb > 1e-4, (pa, pb)
    assert max(abs(x) for x in auto) <= 5 / np.sqrt(n), auto
    assert abs(cross) <= 5 / np.sqrt(n), cross
