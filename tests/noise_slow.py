"""The slow levels of the noise model (config 'noise_model' with 'slow', wfs_set_noise_slow, noise kind 5) restated in numpy; a helper, not
a test.  Philox, the alias cells and the white values come from tests/noise_model.py, the filtered streams from tests/noise_colour.py.

    knot(r, j, m)  = a draw from cells[r] with word m & 3 of the Philox call of (m >> 2 lo, m >> 2 hi, r, 80 + j) for a channel row,
                     (.., g, 96 + j) for common stream g = r - n_channels
    m = t >> s_j,  f = t & (2^s_j - 1),  P0 = slow_q[r][j] knot(r, j, m),  P1 = slow_q[r][j] knot(r, j, m + 1)
    S(r, t)  = sum_j P0 + (((P1 - P0) * f) >> s_j)                                                (arithmetic shifts)
    F'(r, t) = F(r, t) + S(r, t)
    noise(ch, t) = (F'(ch, t) + (group[ch] < 0 ? 0 : (mix_q[ch] * F'(n_channels + group[ch], t)) >> 16) + 32768) >> 16

in int64 numpy arithmetic.  A ``model`` here is the dict of NC.colour_model with 'shifts' and 'slow_q' added (``slow_model``).
"""
import numpy as np

from tests import noise_colour as NC
from tests import noise_model as NM

SITE_NOISE_SLOW = 80
SITE_NOISE_SLOW_COMMON = 96


def slow_model(pmf, vmin, colour=None, slow=None):
    """NC.colour_model of (pmf, vmin, colour) with the dict of wfsim_amd.noise_model.noise_slow (None: no levels)"""
    model = NC.colour_model(pmf, vmin, colour)
    n_rows = model['n_channels'] + model['n_groups']
    if slow is None:
        slow = dict(shifts=np.zeros(0, dtype=np.int64), slow_q=np.zeros((n_rows, 0), dtype=np.int64))
    model['shifts'] = np.asarray(slow['shifts'], dtype=np.int64)
    model['slow_q'] = np.asarray(slow['slow_q'], dtype=np.int64).reshape(n_rows, len(model['shifts']))
    return model


def knot_values(model, seed, row, level, m):
    """knot(row, level, m) for every m of the int64 array m"""
    m = np.asarray(m, dtype=np.int64)
    common = row >= model['n_channels']
    uq, inv = np.unique(m >> 2, return_inverse=True)
    qu = uq.view(np.uint64)
    w = NM.philox4x32_10(qu & np.uint64(0xFFFFFFFF), qu >> np.uint64(32), np.uint64(row - model['n_channels'] if common else row),
                         np.uint64((SITE_NOISE_SLOW_COMMON if common else SITE_NOISE_SLOW) + level), seed)
    word = w[(m & 3).astype(np.int64), inv]
    return (model['vmin'] + NM.alias_sample(model['thr'][row], model['alias'][row], model['shift'], word)).astype(np.int64)


def slow_values(model, seed, row, t):
    """S(row, t) in Q16 for every t of the int64 array t"""
    t = np.asarray(t, dtype=np.int64)
    S = np.zeros(len(t), dtype=np.int64)
    for j, s in enumerate(model['shifts'].tolist()):
        a = int(model['slow_q'][row][j])
        m, f = t >> s, t & ((1 << s) - 1)
        P0, P1 = a * knot_values(model, seed, row, j, m), a * knot_values(model, seed, row, j, m + 1)
        assert max(np.abs(P0).max(initial=0), np.abs(P1).max(initial=0)) < 2 ** 29
        S += P0 + (((P1 - P0) * f) >> s)
    return S


def _stream(model, seed, row, t):
    F = NC._filtered(model, seed, row, t) + slow_values(model, seed, row, t)
    assert np.abs(F).max(initial=0) < 2 ** 29
    return F


def slow_noise_values(model, seed, ch, t):
    """noise(ch, t) for a contiguous ascending int64 array t"""
    t = np.asarray(t, dtype=np.int64)
    if len(t) == 0:
        return np.zeros(0, dtype=np.int64)
    assert np.all(np.diff(t) == 1)
    F = _stream(model, seed, ch, t)
    g = int(model['group'][ch])
    C = (int(model['mix_q'][ch]) * _stream(model, seed, model['n_channels'] + g, t)) >> 16 if g >= 0 else 0
    return (F + C + 32768) >> 16


def materialise_slow(rows, n_windows, model, seed, n_columns=None, pad=8):
    """As NC.materialise_colour, with the slow levels: (table int16[N][n_columns], ix_rand int64[n_windows]), one stretch of the table per
    window, table[ix_rand[g] + k, ch] = noise(ch, row_abs(g, ch) + k) for every row (window, channel, first absolute sample, length)."""
    n_columns = model['n_channels'] if n_columns is None else int(n_columns)
    longest = np.zeros(n_windows, dtype=np.int64)
    seen = set()
    for w, ch, first, length in rows:
        assert (w, ch) not in seen, 'one row per (window, channel)'
        seen.add((w, ch))
        longest[w] = max(longest[w], length)
    ix_rand = np.concatenate([[0], np.cumsum(longest + pad)])[:-1].astype(np.int64)
    table = np.zeros((max(int((longest + pad).sum()), 1), n_columns), dtype=np.int16)
    for w, ch, first, length in rows:
        if ch >= min(n_columns, model['n_channels']):
            continue
        table[ix_rand[w]:ix_rand[w] + length, ch] = slow_noise_values(model, seed, ch, first + np.arange(length, dtype=np.int64))
    return table, ix_rand


# ---------------------------------------------------------------------------------------------------- statistics
# The interpolated knots are cyclostationary with period N = 2^s; a sample autocovariance over many periods estimates the average over
# the phase.  level_autocov enumerates the phases: sample t = m N + f weighs knot m with (N - f) / N and knot m + 1 with f / N, the knots
# are independent with unit variance, and the covariance of two samples is the sum over the knots they share of the product of their
# weights.  (The floor of the arithmetic shift moves a value by less than one Q16 unit, 2^-16 of an amplitude of 1.0: left out.)
def level_autocov(shift, lag):
    """the phase-averaged autocovariance at ``lag`` of one level with unit-variance knots and amplitude 1, by enumeration of f"""
    N = 1 << shift
    lag = abs(int(lag))
    total = 0.0
    for f in range(N):
        wa = {0: (N - f) / N, 1: f / N}
        dm, f2 = divmod(f + lag, N)
        wb = {dm: (N - f2) / N, dm + 1: f2 / N}
        total += sum(wa[k] * wb[k] for k in wa if k in wb)
    return total / N


def pmf_variance(pmf_row, vmin):
    v = vmin + np.arange(len(pmf_row), dtype=np.float64)
    mean = float((pmf_row * v).sum())
    return float((pmf_row * (v - mean) ** 2).sum())
