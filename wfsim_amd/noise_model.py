"""Digitiser noise drawn per sample on the device (config ``noise_model``; wfs_set_noise_model).

The reference replays a recorded noise array from a random offset per digitise window (rawdata.py:398-437).  With a model the
noise of a sample is a draw from the channel's distribution over integer ADC offsets, made from a counter-based random word of
(seed, channel, absolute sample index): no array, no period, the same value whichever window or batch holds the sample.  White
noise only: samples are independent of each other and of the other channels.

``config['noise_model']`` is one of

* ``None`` / absent: nothing changes, ``noise_data`` is replayed as before;
* ``{'sigma': float | array[n_channels]}``: a Gaussian of that standard deviation [ADC counts] per channel, discretised:
  ``half = max(1, ceil(6 * max sigma))``, values ``-half .. half``, the mass of value k is ``Phi((k + 1/2) / sigma) - Phi((k - 1/2) / sigma)``
  (the Gaussian rounded to the nearest integer) and the two tails beyond ``half + 1/2`` are folded into the end values, so every row
  sums to 1.  ``sigma == 0`` puts all mass on 0.  The variance of the discretised distribution is ``sigma^2 + 1/12`` (Sheppard) for
  sigma of about an ADC count or more.  A scalar covers ``len(config['gains'])`` channels; an array sets the channel count by its
  length -- 801 entries give the high-energy rows and the sum row noise, as an 801-column noise array does;
* ``{'pmf': array[n_channels][n_values], 'vmin': int}``: any distribution per channel over ``vmin .. vmin + n_values - 1``
  (see ``pmf_from_samples``).

The model only acts with ``enable_noise``; it takes precedence over ``noise_data``.

Colour (wfs_set_noise_colour).  Two optional keys turn the white sequences into coloured, channel-correlated noise while
keeping the value a function of (seed, channel, absolute sample index):

* ``'taps'``: FIR taps, a float array ``[L]`` for all channels or ``[n_channels][L]``, 1 <= L <= 16.  The channel's noise becomes
  ``sum_k h[k] w(ch, t - k)``.  The taps are used as given, quantised with ``round(h * 65536)``: no hidden normalisation, see
  ``unit_power`` and ``taps_from_psd``;
* ``'common'``: ``{'groups': int[n_channels] (-1: none), 'gain': number | [n_channels], 'sigma': number | [n_groups]}`` or, in place
  of ``'sigma'``, ``'pmf': [n_groups][n_values]`` on the model's ``vmin``; optional ``'taps'``: ``[L']`` or ``[n_groups][L']``.  Every
  group has one white common stream c(g, t); a channel of group g adds ``gain * sum_k h_c[k] c(g, t - k)``: the coherent part of the
  channels of one digitiser board.  With ``'sigma'`` for channels and groups the Gaussians are built together and share ``half``.

Tap rows shorter than the longest are zero-padded.  The sum is rounded to the nearest integer (half up), so the variance of a channel is

    Var ~ Var_w * sum h^2 + gain^2 * Var_c * sum h_c^2 + 1/12

with Var_w, Var_c the variances of the channel's and the group's distributions.  The arithmetic is exact in integers (Q16 taps); a
model is refused unless ``sum |h_q| * max |value| < 2^29`` for every row of taps.

Slow levels (wfs_set_noise_slow).  The taps reach 16 samples; baseline motion slower than that comes from the key

* ``'slow'``: ``{'shifts': int[n_levels], 'amplitude': [n_levels] | [n_channels][n_levels]}``, 1 <= n_levels <= 8, shifts strictly
  ascending in 4 .. 30.  Level j is a sequence of knots ``2^shifts[j]`` samples apart, each a draw from the channel's own distribution
  (its own counter-based word), joined by linear interpolation and scaled by the amplitude; the levels are added to the channel's
  filtered sequence before the rounding.  ``'period_ns'`` may stand in place of ``'shifts'``: knot periods in ns, each ``dt * 2^s``.
  Amplitudes are quantised with ``round(a * 65536)``, no hidden normalisation; averaged over the phase a level has the variance
  ``a^2 Var_w (2/3 + 1/(3 * 4^s))`` (``slow_levels`` picks amplitudes for a stated rms);
* ``noise_model['common']['slow']``: amplitudes ``[n_levels]`` or ``[n_groups][n_levels]`` of the same levels on the common streams: slow
  motion that is coherent over a group and adds linearly in a sum of its channels.

With slow levels the bound reads ``(sum |h_q| + sum |a_q|) * max |value| < 2^29`` per row (``sum |h_q| = 65536`` without taps).
"""
import math

import numpy as np

MAX_VALUES = 4096           # wfs_set_noise_model
MAX_TAPS = 16               # wfs_set_noise_colour
MAX_LEVELS, MIN_SHIFT, MAX_SHIFT = 8, 4, 30        # wfs_set_noise_slow
Q16 = 65536
SUM_TOLERANCE = 1e-9


def _phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def gaussian_pmf(sigma):
    """(pmf[n_channels][2 half + 1], vmin = -half) of the discretised Gaussians described in the module docstring"""
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    if sigma.ndim != 1 or len(sigma) == 0 or not np.all(np.isfinite(sigma)) or np.any(sigma < 0):
        raise ValueError("noise_model['sigma'] must be a non-negative number or a 1-D array of them")
    half = max(1, int(math.ceil(6.0 * float(sigma.max()))))
    if 2 * half + 1 > MAX_VALUES:
        raise ValueError(f"noise_model['sigma']: {2 * half + 1} values, more than {MAX_VALUES}")
    pmf = np.zeros((len(sigma), 2 * half + 1), dtype=np.float64)
    for c, s in enumerate(sigma):
        if s == 0:
            pmf[c, half] = 1.0
            continue
        # upper half from differences of the upper tail (no cancellation far out), mirrored: exactly symmetric
        tail = np.array([_phi(-(k - 0.5) / s) for k in range(1, half + 2)])        # P(X > k - 1/2), k = 1 .. half + 1
        up = tail[:-1] - tail[1:]
        up[-1] += tail[-1]                                                          # the tail beyond half + 1/2
        pmf[c, half + 1:] = up
        pmf[c, :half] = up[::-1]
        pmf[c, half] = 1.0 - 2.0 * tail[0]
    return pmf, -half


def check_pmf(pmf, vmin, n_rows=None):
    """validates what wfs_set_noise_model validates, with the argument named; returns (pmf as f64[n_channels][n_values], vmin)"""
    pmf = np.ascontiguousarray(pmf, dtype=np.float64)
    if pmf.ndim != 2 or pmf.shape[0] < 1:
        raise ValueError('noise model: pmf must be a 2-D array [n_channels][n_values]')
    n_ch, n_val = pmf.shape
    if n_rows is not None and n_ch > n_rows:
        raise ValueError(f'noise model: n_channels {n_ch} exceeds the {n_rows} rows of the digitiser array')
    if n_val < 1 or n_val > MAX_VALUES:
        raise ValueError(f'noise model: n_values {n_val} outside 1 .. {MAX_VALUES}')
    if int(vmin) != vmin:
        raise ValueError('noise model: vmin must be an integer')
    vmin = int(vmin)
    if vmin < -32768 or vmin + n_val - 1 > 32767:
        raise ValueError(f'noise model: values {vmin} .. {vmin + n_val - 1} leave the int16 range')
    if not np.all(pmf >= 0):            # (NaN fails too)
        raise ValueError('noise model: pmf has a negative entry')
    bad = np.where(np.abs(pmf.sum(axis=1) - 1.0) > SUM_TOLERANCE)[0]
    if len(bad):
        raise ValueError(f'noise model: pmf of channel {int(bad[0])} does not sum to 1')
    return pmf, vmin


def noise_pmf(config, n_rows):
    """(pmf[n_channels][n_values], vmin) from ``config['noise_model']``, or None without one"""
    m = config.get('noise_model')
    if m is None:
        return None
    if not isinstance(m, dict) or ('sigma' in m) == ('pmf' in m):
        raise ValueError("noise_model must be a dict with either 'sigma' or 'pmf' (and 'vmin')")
    if 'sigma' in m:
        sigma = np.asarray(m['sigma'], dtype=np.float64)
        if sigma.ndim == 0:
            sigma = np.full(len(config['gains']), float(sigma))
        common = m.get('common')
        if isinstance(common, dict) and 'sigma' in common and sigma.ndim == 1:
            # channels and common streams in one call: one half, one vmin (noise_colour takes the groups' rows from the same call)
            pmf, vmin = gaussian_pmf(np.concatenate([sigma, _group_sigmas(common, len(sigma))]))
            pmf = pmf[:len(sigma)]
        else:
            pmf, vmin = gaussian_pmf(sigma)
    else:
        if 'vmin' not in m:
            raise ValueError("noise_model: 'pmf' needs 'vmin'")
        pmf, vmin = m['pmf'], m['vmin']
    return check_pmf(pmf, vmin, n_rows)


def pmf_from_samples(noise_data):
    """The per-channel histogram of a recorded noise array [n_samples][n_channels] (integral values) as a ``noise_model``:
    ``{'pmf': ..., 'vmin': ...}`` -- the ADC distribution of the recording without its period."""
    a = np.asarray(noise_data)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('pmf_from_samples: noise_data must be [n_samples][n_channels]')
    if not np.array_equal(a, np.trunc(a)):
        raise ValueError('pmf_from_samples: noise_data must hold integral ADC values')
    a = a.astype(np.int64)
    vmin, vmax = int(a.min()), int(a.max())
    n_val = vmax - vmin + 1
    if n_val > MAX_VALUES:
        raise ValueError(f'pmf_from_samples: {n_val} values, more than {MAX_VALUES}')
    pmf = np.zeros((a.shape[1], n_val), dtype=np.float64)
    for c in range(a.shape[1]):
        pmf[c] = np.bincount(a[:, c] - vmin, minlength=n_val) / a.shape[0]
    check_pmf(pmf, vmin)
    return dict(pmf=pmf, vmin=vmin)


# ---------------------------------------------------------------------------------------------------- colour
def _n_groups(common, n_channels):
    if not isinstance(common, dict) or 'groups' not in common or 'gain' not in common or ('sigma' in common) == ('pmf' in common):
        raise ValueError("noise_model['common'] must be a dict with 'groups', 'gain' and either 'sigma' or 'pmf'")
    g = np.asarray(common['groups'])
    if g.ndim != 1 or len(g) != n_channels or g.dtype.kind not in 'iu':
        raise ValueError(f"noise_model['common']['groups'] must be an integer array [{n_channels}] (-1: no group)")
    if g.min() < -1:
        raise ValueError("noise_model['common']['groups']: entries below -1")
    return int(g.max()) + 1


def _group_sigmas(common, n_channels):
    n_groups = _n_groups(common, n_channels)
    s = np.asarray(common['sigma'], dtype=np.float64)
    if s.ndim == 0:
        s = np.full(n_groups, float(s))
    if s.ndim != 1 or len(s) != n_groups:
        raise ValueError(f"noise_model['common']['sigma'] must be a number or an array [{n_groups}] (one per group)")
    return s


def _tap_rows(taps, n_rows, name):
    t = np.asarray(taps, dtype=np.float64)
    if t.ndim == 1:
        t = np.tile(t, (n_rows, 1))
    if t.ndim != 2 or t.shape[0] != n_rows or t.shape[1] < 1:
        raise ValueError(f'{name} must be a float array [L] or [{n_rows}][L]')
    if t.shape[1] > MAX_TAPS:
        raise ValueError(f'{name}: {t.shape[1]} taps, more than {MAX_TAPS}')
    if not np.all(np.isfinite(t)):
        raise ValueError(f'{name} must be finite')
    return t


def quantise_taps(taps):
    """round(h * 65536) as int64 (the caller checks the range)"""
    return np.floor(np.asarray(taps, dtype=np.float64) * Q16 + 0.5).astype(np.int64)


def check_colour(taps_q, group, mix_q, common_pmf, n_channels, n_values, vmin):
    """validates what wfs_set_noise_colour validates, with the argument named; returns the arrays in the dtypes of the C ABI"""
    taps_q = np.asarray(taps_q, dtype=np.int64)
    group, mix_q = np.asarray(group, dtype=np.int64), np.asarray(mix_q, dtype=np.int64)
    common_pmf = np.asarray(common_pmf, dtype=np.float64).reshape(-1, n_values)
    n_groups = common_pmf.shape[0]
    if taps_q.ndim != 2 or taps_q.shape[0] != n_channels + n_groups:
        raise ValueError(f'noise colour: taps_q must be [{n_channels + n_groups}][n_taps] (channels, then common streams)')
    if taps_q.shape[1] < 1 or taps_q.shape[1] > MAX_TAPS:
        raise ValueError(f'noise colour: n_taps {taps_q.shape[1]} outside 1 .. {MAX_TAPS}')
    vmax = max(abs(int(vmin)), abs(int(vmin) + int(n_values) - 1))
    bound = np.abs(taps_q).sum(axis=1) * vmax
    bad = np.where(bound >= 2 ** 29)[0]
    if len(bad):
        raise ValueError(f'noise colour: taps_q of row {int(bad[0])}: sum |taps| * max |value| = {int(bound[bad[0]])} reaches 2^29')
    if group.shape != (n_channels,) or mix_q.shape != (n_channels,):
        raise ValueError(f'noise colour: group and mix_q must be [{n_channels}]')
    bad = np.where((group < -1) | (group >= n_groups))[0]
    if len(bad):
        raise ValueError(f'noise colour: group of channel {int(bad[0])} outside -1 .. {n_groups - 1}')
    bad = np.where(np.abs(mix_q) > Q16)[0]
    if len(bad):
        raise ValueError(f'noise colour: mix_q of channel {int(bad[0])} beyond {Q16} in magnitude (|gain| > 1)')
    if not np.all(common_pmf >= 0):
        raise ValueError('noise colour: common_pmf has a negative entry')
    bad = np.where(np.abs(common_pmf.sum(axis=1) - 1.0) > SUM_TOLERANCE)[0]
    if len(bad):
        raise ValueError(f'noise colour: common_pmf of group {int(bad[0])} does not sum to 1')
    return (np.ascontiguousarray(taps_q, dtype=np.int32), np.ascontiguousarray(group, dtype=np.int32),
            np.ascontiguousarray(mix_q, dtype=np.int32), np.ascontiguousarray(common_pmf))


def noise_colour(config, n_rows):
    """dict(taps_q int32[n_channels + n_groups][L], group int32[n_channels], mix_q int32[n_channels], common_pmf f64[n_groups][n_values])
    from the 'taps' and 'common' keys of ``config['noise_model']``, or None when it has neither (a white model, or no model)"""
    m = config.get('noise_model')
    if not isinstance(m, dict) or ('taps' not in m and 'common' not in m):
        return None
    pmf, vmin = noise_pmf(config, n_rows)
    n_ch, n_val = pmf.shape
    taps = _tap_rows(m['taps'], n_ch, "noise_model['taps']") if 'taps' in m else np.ones((n_ch, 1))
    group, mix_q, common_pmf, ctaps = np.full(n_ch, -1, dtype=np.int64), np.zeros(n_ch, dtype=np.int64), np.zeros((0, n_val)), np.zeros((0, 1))
    common = m.get('common')
    if common is not None:
        n_groups = _n_groups(common, n_ch)
        group = np.asarray(common['groups'], dtype=np.int64)
        gain = np.asarray(common['gain'], dtype=np.float64)
        gain = np.full(n_ch, float(gain)) if gain.ndim == 0 else gain
        if gain.shape != (n_ch,) or not np.all(np.isfinite(gain)):
            raise ValueError(f"noise_model['common']['gain'] must be a number or an array [{n_ch}]")
        mix_q = np.where(group >= 0, quantise_taps(gain), 0)
        if 'sigma' in common:
            if 'sigma' not in m:
                raise ValueError("noise_model['common']['sigma'] needs the channels given by 'sigma' too (with a 'pmf' give the groups a 'pmf')")
            sigma = np.asarray(m['sigma'], dtype=np.float64)
            sigma = np.full(n_ch, float(sigma)) if sigma.ndim == 0 else sigma
            both, vmin_c = gaussian_pmf(np.concatenate([sigma, _group_sigmas(common, n_ch)]))
            assert vmin_c == vmin and both.shape[1] == n_val
            common_pmf = both[n_ch:]
        else:
            common_pmf = np.asarray(common['pmf'], dtype=np.float64)
            if common_pmf.ndim != 2 or common_pmf.shape != (n_groups, n_val):
                raise ValueError(f"noise_model['common']['pmf'] must be [{n_groups}][{n_val}] (one row per group, on the model's values)")
        ctaps = _tap_rows(common['taps'], n_groups, "noise_model['common']['taps']") if 'taps' in common else np.ones((n_groups, 1))
    L = max(taps.shape[1], ctaps.shape[1])
    rows = np.zeros((n_ch + len(ctaps), L), dtype=np.float64)
    rows[:n_ch, :taps.shape[1]] = taps
    rows[n_ch:, :ctaps.shape[1]] = ctaps
    taps_q, group, mix_q, common_pmf = check_colour(quantise_taps(rows), group, mix_q, common_pmf, n_ch, n_val, vmin)
    return dict(taps_q=taps_q, group=group, mix_q=mix_q, common_pmf=common_pmf)


# ---------------------------------------------------------------------------------------------------- slow levels
def check_slow(shifts, slow_q, taps_q, n_channels, n_groups, n_values, vmin):
    """validates what wfs_set_noise_slow validates, with the argument named; taps_q: those of the colour, None without one (a unit tap per
    channel, no groups).  Returns (shifts int32[n_levels], slow_q int32[n_channels + n_groups][n_levels])"""
    shifts, slow_q = np.asarray(shifts, dtype=np.int64), np.asarray(slow_q, dtype=np.int64)
    if shifts.ndim != 1 or len(shifts) < 1 or len(shifts) > MAX_LEVELS:
        raise ValueError(f'noise slow: n_levels {shifts.size if shifts.ndim == 1 else shifts.shape} outside 1 .. {MAX_LEVELS}')
    bad = np.where((shifts < MIN_SHIFT) | (shifts > MAX_SHIFT))[0]
    if len(bad):
        raise ValueError(f'noise slow: shifts[{int(bad[0])}] = {int(shifts[bad[0]])} outside {MIN_SHIFT} .. {MAX_SHIFT}')
    bad = np.where(np.diff(shifts) <= 0)[0]
    if len(bad):
        raise ValueError(f'noise slow: shifts not strictly ascending at level {int(bad[0]) + 1}')
    n_rows = n_channels + (n_groups if taps_q is not None else 0)
    if slow_q.shape != (n_rows, len(shifts)):
        raise ValueError(f'noise slow: slow_q must be [{n_rows}][{len(shifts)}] (channels, then common streams)')
    tapsum = np.abs(np.asarray(taps_q, dtype=np.int64)).sum(axis=1) if taps_q is not None else np.full(n_rows, Q16, dtype=np.int64)
    vmax = max(abs(int(vmin)), abs(int(vmin) + int(n_values) - 1))
    bound = (tapsum + np.abs(slow_q).sum(axis=1)) * vmax
    bad = np.where(bound >= 2 ** 29)[0]
    if len(bad):
        raise ValueError(f'noise slow: slow_q of row {int(bad[0])}: (sum |taps| + sum |slow|) * max |value| = {int(bound[bad[0]])} reaches 2^29')
    return np.ascontiguousarray(shifts, dtype=np.int32), np.ascontiguousarray(slow_q, dtype=np.int32)


def _slow_shifts(slow, dt_ns):
    if not isinstance(slow, dict) or 'amplitude' not in slow or ('shifts' in slow) == ('period_ns' in slow):
        raise ValueError("noise_model['slow'] must be a dict with 'amplitude' and either 'shifts' or 'period_ns'")
    if 'shifts' in slow:
        sh = np.asarray(slow['shifts'])
        if sh.ndim != 1 or sh.dtype.kind not in 'iu':
            raise ValueError("noise_model['slow']['shifts'] must be a 1-D integer array")
        return sh.astype(np.int64)
    period = np.atleast_1d(np.asarray(slow['period_ns'], dtype=np.float64))
    if period.ndim != 1:
        raise ValueError("noise_model['slow']['period_ns'] must be a number or a 1-D array")
    sh = np.zeros(len(period), dtype=np.int64)
    for j, p in enumerate(period):
        s = int(round(math.log2(p / dt_ns))) if np.isfinite(p) and p > 0 else -1
        if s < 0 or dt_ns * 2 ** s != p:
            raise ValueError(f"noise_model['slow']['period_ns'][{j}] = {p:g} ns is not dt * 2^s (dt = {dt_ns:g} ns)")
        sh[j] = s
    return sh


def _amp_rows(amp, n_rows, n_levels, name):
    a = np.asarray(amp, dtype=np.float64)
    if a.ndim == 1:
        a = np.tile(a, (n_rows, 1))
    if a.ndim != 2 or a.shape != (n_rows, n_levels):
        raise ValueError(f'{name} must be a float array [{n_levels}] or [{n_rows}][{n_levels}]')
    if not np.all(np.isfinite(a)):
        raise ValueError(f'{name} must be finite')
    return a


def noise_slow(config, n_rows):
    """dict(shifts int32[n_levels], slow_q int32[n_channels + n_groups][n_levels]) from the 'slow' keys of ``config['noise_model']`` and
    of its 'common', or None when the model has no slow levels"""
    m = config.get('noise_model')
    if not isinstance(m, dict):
        return None
    common = m.get('common')
    if 'slow' not in m:
        if isinstance(common, dict) and 'slow' in common:
            raise ValueError("noise_model['common']['slow'] needs noise_model['slow'] (the shifts; its amplitudes may be zero)")
        return None
    pmf, vmin = noise_pmf(config, n_rows)
    n_ch, n_val = pmf.shape
    colour = noise_colour(config, n_rows)
    shifts = _slow_shifts(m['slow'], float(config.get('sample_duration', 10)))
    amp = _amp_rows(m['slow']['amplitude'], n_ch, len(shifts), "noise_model['slow']['amplitude']")
    n_groups = len(colour['common_pmf']) if colour is not None else 0
    camp = np.zeros((n_groups, len(shifts)))
    if isinstance(common, dict) and 'slow' in common:
        camp = _amp_rows(common['slow'], n_groups, len(shifts), "noise_model['common']['slow']")
    shifts, slow_q = check_slow(shifts, quantise_taps(np.concatenate([amp, camp])), None if colour is None else colour['taps_q'],
                                n_ch, n_groups, n_val, vmin)
    return dict(shifts=shifts, slow_q=slow_q)


def slow_level_variance(amplitude, shift, var_w):
    """the variance of one level averaged over the phase: a knot pair weighted (1 - u, u), u = f / 2^s, has (1 - u)^2 + u^2 of the knot
    variance, and the mean of that over f = 0 .. 2^s - 1 is 2/3 + 1/(3 * 4^s)"""
    return amplitude ** 2 * var_w * (2.0 / 3.0 + 1.0 / (3.0 * 4.0 ** shift))


def slow_levels(f_lo_hz, f_hi_hz, rms_adc, white_sigma, dt_ns=10):
    """A ``noise_model['slow']`` of one level per octave between two frequencies: a level whose knots are 2^s samples apart moves no
    faster than the Nyquist frequency of its knots, 1 / (2 * dt * 2^s), and the levels taken are those with that frequency inside
    [f_lo_hz, f_hi_hz].  Equal amplitudes, chosen so that the slow part has the stated rms [ADC counts] on a channel whose white
    distribution is the discretised Gaussian of ``white_sigma`` (variance sigma^2 + 1/12)."""
    if not (0 < f_lo_hz <= f_hi_hz) or not rms_adc >= 0 or not white_sigma > 0:
        raise ValueError('slow_levels: needs 0 < f_lo_hz <= f_hi_hz, rms_adc >= 0 and white_sigma > 0')
    shifts = [s for s in range(MIN_SHIFT, MAX_SHIFT + 1) if f_lo_hz <= 1.0 / (2.0 * dt_ns * 1e-9 * 2 ** s) <= f_hi_hz]
    if not 1 <= len(shifts) <= MAX_LEVELS:
        raise ValueError(f'slow_levels: {len(shifts)} octaves between {f_lo_hz:g} and {f_hi_hz:g} Hz, outside 1 .. {MAX_LEVELS} '
                         f'(knot periods are dt * 2^s, s = {MIN_SHIFT} .. {MAX_SHIFT})')
    var_w = float(white_sigma) ** 2 + 1.0 / 12.0
    unit = sum(slow_level_variance(1.0, s, var_w) for s in shifts)
    a = float(rms_adc) / math.sqrt(unit)
    return dict(shifts=shifts, amplitude=[a] * len(shifts))


def unit_power(taps):
    """the taps, every row scaled to sum h^2 = 1: the filtered sequence keeps the variance of the white one"""
    t = np.asarray(taps, dtype=np.float64)
    p = np.sqrt((t * t).sum(axis=-1, keepdims=True))
    if np.any(p == 0):
        raise ValueError('unit_power: a row of zeros')
    return t / p


def taps_from_psd(freqs_hz, psd, n_taps, dt_ns=10):
    """Linear-phase FIR taps whose power response follows a measured power spectral density (frequency sampling): sqrt(psd) is
    interpolated onto the n_taps-point rFFT grid k / (n_taps * dt), taken as a zero-phase amplitude response, inverted and rotated to
    the causal, symmetric form; the taps are scaled to unit power.  At the grid frequencies |H|^2 is the (scaled) psd exactly."""
    n_taps = int(n_taps)
    if n_taps < 1 or n_taps > MAX_TAPS:
        raise ValueError(f'taps_from_psd: n_taps outside 1 .. {MAX_TAPS}')
    f, p = np.asarray(freqs_hz, dtype=np.float64), np.asarray(psd, dtype=np.float64)
    if f.ndim != 1 or f.shape != p.shape or len(f) < 1 or np.any(np.diff(f) <= 0) or np.any(p < 0) or not np.all(np.isfinite(p)):
        raise ValueError('taps_from_psd: freqs_hz must be increasing, psd non-negative and of the same length')
    grid = np.fft.rfftfreq(n_taps, d=float(dt_ns) * 1e-9)
    amp = np.sqrt(np.interp(grid, f, p))
    h = np.fft.irfft(amp, n=n_taps)                 # zero phase: real, symmetric about index 0
    h = np.roll(h, (n_taps - 1) // 2)               # a circular shift: the same magnitudes at the grid frequencies
    return unit_power(h)
