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
"""
import math

import numpy as np

MAX_VALUES = 4096           # wfs_set_noise_model
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
