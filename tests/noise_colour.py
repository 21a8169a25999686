"""The coloured noise model (config 'noise_model' with 'taps' / 'common', wfs_set_noise_colour, noise kind 4) restated in numpy; a helper,
not a test.  Philox, the alias cells and the white values come from tests/noise_model.py.

    w(r, t), r < n_channels   : NM.noise_values(cells[r], ..., channel = r, t)                 (Philox counter (q lo, q hi, r, 65))
    w(n_channels + g, t)      : the same under the counter (q lo, q hi, g, 66), cells[n_channels + g]
    F(r, t)  = sum_k taps_q[r][k] * w(r, t - k)
    C(ch, t) = group[ch] < 0 ? 0 : (mix_q[ch] * F(n_channels + group[ch], t)) >> 16             (arithmetic shift)
    noise(ch, t) = (F(ch, t) + C(ch, t) + 32768) >> 16

in int64 numpy arithmetic (every intermediate fits: |F| < 2^29 by the bound the host checks).  A ``model`` here is the dict that
``colour_model`` builds from what wfsim_amd.noise_model hands the engine.
"""
import numpy as np

from tests import noise_model as NM

SITE_NOISE_COMMON = 66


def colour_model(pmf, vmin, colour=None):
    """pmf[n_channels][n_values], vmin and the dict of wfsim_amd.noise_model.noise_colour (None: white, one unit tap) as one model:
    the cells of every stream as the host builds them, taps, groups and gains"""
    pmf = np.asarray(pmf, dtype=np.float64)
    n_ch = pmf.shape[0]
    if colour is None:
        colour = dict(taps_q=np.full((n_ch, 1), 65536), group=np.full(n_ch, -1), mix_q=np.zeros(n_ch), common_pmf=np.zeros((0, pmf.shape[1])))
    common = np.asarray(colour['common_pmf'], dtype=np.float64).reshape(-1, pmf.shape[1])
    thr, alias, shift = NM.build_cells(np.concatenate([pmf, common]))
    return dict(n_channels=n_ch, n_groups=len(common), vmin=int(vmin), thr=thr, alias=alias, shift=shift,
                taps_q=np.asarray(colour['taps_q'], dtype=np.int64), group=np.asarray(colour['group'], dtype=np.int64),
                mix_q=np.asarray(colour['mix_q'], dtype=np.int64))


def white_values(model, seed, row, t):
    """w(row, t) for every t of the int64 array t"""
    t = np.asarray(t, dtype=np.int64)
    cells = (model['thr'][row], model['alias'][row])
    if row < model['n_channels']:
        return NM.noise_values(cells, model['shift'], model['vmin'], seed, row, t)
    q = t >> 2
    uq, inv = np.unique(q, return_inverse=True)
    qu = uq.view(np.uint64)
    w = NM.philox4x32_10(qu & np.uint64(0xFFFFFFFF), qu >> np.uint64(32), np.uint64(row - model['n_channels']), np.uint64(SITE_NOISE_COMMON), seed)
    word = w[(t & 3).astype(np.int64), inv]
    return (model['vmin'] + NM.alias_sample(cells[0], cells[1], model['shift'], word)).astype(np.int64)


def _filtered(model, seed, row, t):
    """F(row, t) for a CONTIGUOUS ascending t (the whites of t[0] - L + 1 .. t[-1] are drawn once)"""
    taps = model['taps_q'][row]
    L = len(taps)
    w = white_values(model, seed, row, np.arange(int(t[0]) - (L - 1), int(t[-1]) + 1, dtype=np.int64))
    F = np.zeros(len(t), dtype=np.int64)
    for k in range(L):
        F += int(taps[k]) * w[L - 1 - k:L - 1 - k + len(t)]
    assert np.abs(F).max(initial=0) < 2 ** 29
    return F


def colour_values(model, seed, ch, t):
    """noise(ch, t) for a contiguous ascending int64 array t"""
    t = np.asarray(t, dtype=np.int64)
    if len(t) == 0:
        return np.zeros(0, dtype=np.int64)
    assert np.all(np.diff(t) == 1)
    F = _filtered(model, seed, ch, t)
    g = int(model['group'][ch])
    C = (int(model['mix_q'][ch]) * _filtered(model, seed, model['n_channels'] + g, t)) >> 16 if g >= 0 else 0
    return (F + C + 32768) >> 16


def materialise_colour(rows, n_windows, model, seed, n_columns=None, pad=8):
    """As NM.materialise, with the coloured values: (table int16[N][n_columns], ix_rand int64[n_windows]), one stretch of the table per
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
        table[ix_rand[w]:ix_rand[w] + length, ch] = colour_values(model, seed, ch, first + np.arange(length, dtype=np.int64))
    return table, ix_rand


# ---------------------------------------------------------------------------------------------------- statistics
# 2^20 restated samples under a fixed seed (tests/test_noise_colour_cpu.py).  The predictions: with r_h(lag) = sum_k h[k] h[k + lag],
# the filtered sequence has autocovariance r_h(lag) Var_w; rounding to integers adds 1/12 of white variance.
STAT_SEED = 20261019
STAT_N = 1 << 20
STAT_T0 = 987654321


def tap_autocorr(h, lag):
    h = np.asarray(h, dtype=np.float64)
    return float((h[lag:] * h[:len(h) - lag]).sum()) if lag < len(h) else 0.0


def bartlett_factor(rxx, ryy, rxy, k, n_lags=48):
    """Bartlett's variance factor B of the sample cross-correlation r_xy(k) of two jointly stationary series, n Var(r_xy(k)) ~ B (Bartlett
    1955; Box & Jenkins, Time Series Analysis, eq. 11.1.7):

        B = sum_v { rxx(v) ryy(v) + rxy(k + v) rxy(k - v) + rxy(k)^2 [rxy(v)^2 + rxx(v)^2 / 2 + ryy(v)^2 / 2]
                    - 2 rxy(k) [rxx(v) rxy(v + k) + rxy(-v) ryy(v + k)] }

    over all lags v; rxx, ryy, rxy: the predicted correlation functions, callables on signed lags that vanish beyond the filters.
    With x = y (rxy = rxx) it is his formula for an autocorrelation."""
    c = rxy(k)
    return sum(rxx(v) * ryy(v) + rxy(k + v) * rxy(k - v) + c * c * (rxy(v) ** 2 + 0.5 * rxx(v) ** 2 + 0.5 * ryy(v) ** 2)
               - 2.0 * c * (rxx(v) * rxy(v + k) + rxy(-v) * ryy(v + k)) for v in range(-n_lags, n_lags + 1))


def sample_autocorr(x, lag):
    x = np.asarray(x, dtype=np.float64)
    x = x - x.mean()
    return float((x[lag:] * x[:-lag]).mean() / (x * x).mean())


def sample_corr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))
