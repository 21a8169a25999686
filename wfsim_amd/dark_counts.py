"""PMT dark counts (config 'dark_count_rate', wfs_set_dark_counts): rates to the thresholds of a cell's Poisson count.

A cell is CELL = 64 samples of a channel's absolute sample axis; its dark photons are N ~ Poisson(mu), mu = rate * CELL * dt * 1e-9,
counted from one 32-bit word w as sum_{k = 1 .. 4} [w < T[k]] with T[k] = floor(2^32 P(N >= k)).  The tails are summed as the
series sum_{i >= k} from the smallest term up -- 1 - sum_{i < k} loses a small mu to cancellation.  mu <= MU_MAX = 1/8: the mass above
4 photons, below 2.6e-7, is folded into 4.  The library computes the same thresholds from the rates (wfs_dark.h); these are for
the restatement of the tests and for users who want the law.
"""
import math

import numpy as np

CELL = 64
MAX_PHOTONS = 4
MU_MAX = 0.125
SITE_COUNT, SITE_PHOTON = 112, 113


def mu_of(rate_hz, dt):
    """mean dark photons per cell"""
    return np.asarray(rate_hz, dtype=np.float64) * (CELL * float(dt) * 1e-9)


def max_rate(dt):
    """the largest rate [Hz] the setter takes at a sample duration of dt ns"""
    return MU_MAX / (CELL * float(dt) * 1e-9)


def tail(mu, k):
    """P(N >= k), N ~ Poisson(mu), as the series from the smallest term up"""
    mu = float(mu)
    t = math.exp(-mu)
    for i in range(1, k + 1):
        t *= mu / i
    terms = []
    i = k
    while t > 0 and len(terms) < 48:
        terms.append(t)
        t *= mu / (i + 1)
        i += 1
    s = 0.0
    for t in reversed(terms):
        s += t
    return s


def thresholds_of_mu(mu):
    """uint32[4]: floor(2^32 P(N >= k)), k = 1 .. 4"""
    mu = float(mu)
    if not (mu >= 0.0) or not math.isfinite(mu):
        raise ValueError('dark counts: a mean per cell that is negative or not finite')
    if mu > MU_MAX:
        raise ValueError(f'dark counts: {mu:.4g} photons per cell of {CELL} samples, more than 1/8')
    return np.array([int(math.floor(tail(mu, k) * 4294967296.0)) for k in range(1, MAX_PHOTONS + 1)], dtype=np.uint32)


def rates_array(rate, n_channels):
    """a number or one value per channel [Hz] -> float64[n_channels]; raises on a negative or non-finite rate or a wrong length"""
    r = np.asarray(rate, dtype=np.float64)
    if r.ndim == 0:
        r = np.full(int(n_channels), float(r))
    if r.ndim != 1 or len(r) > int(n_channels):
        raise ValueError(f'dark_count_rate: a number or at most {int(n_channels)} values, one per channel')
    if not np.all(np.isfinite(r)) or np.any(r < 0):
        raise ValueError('dark_count_rate: a rate that is negative or not finite')
    return np.ascontiguousarray(r)


def thresholds(rate, n_channels, dt):
    """uint32[n][4] of a rate or an array of rates [Hz]"""
    r = rates_array(rate, n_channels)
    return np.stack([thresholds_of_mu(m) for m in mu_of(r, dt)]) if len(r) else np.zeros((0, MAX_PHOTONS), dtype=np.uint32)


def rates_from(config, n_channels=None):
    """float64[n] of config['dark_count_rate'] (a number or one value per channel, Hz), or None when the key is absent, None or all
    zero; n_channels: the PMTs of the engine's array (default: len(config['gains']))"""
    rate = config.get('dark_count_rate')
    if rate is None:
        return None
    n = len(config['gains']) if n_channels is None else int(n_channels)
    r = rates_array(rate, n)
    dt = config['sample_duration']
    if np.any(mu_of(r, dt) > MU_MAX):
        raise ValueError(f'dark_count_rate: above {max_rate(dt):.4g} Hz, more than 1/8 photons per cell of {CELL} samples')
    return r if np.any(r > 0) else None
