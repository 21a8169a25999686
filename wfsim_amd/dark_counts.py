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


# ---- lone-hit rows (config 'dark_count_lone_hits', wfs_lone_hits)

def lone_gap(params):
    """G = tlen + 2 tw [samples]: lone photons of a channel whose starts are at most G apart share a row"""
    return int(params['tlen']) + 2 * int(params['trigger_window'])


def lone_min_rext(params):
    """the smallest right_raw_extension [ns] the lone-hit passes of RawData take: (2 G + 64) dt (wfs_lone.h, lone_min_rext)"""
    return (2 * lone_gap(params) + CELL) * int(params['dt'])


def lone_hits_from(config, params=None):
    """True when config['dark_count_lone_hits'] asks for lone-hit rows; raises ValueError when it does and they cannot be had"""
    if not config.get('dark_count_lone_hits', False):
        return False
    if rates_from(config, None if params is None else params['n_tpc']) is None:
        raise ValueError("dark_count_lone_hits: needs config['dark_count_rate'] (a rate above zero on some channel)")
    if params is None:
        from .config import kernel_params
        params = kernel_params(config)
    _lone_window_bounds('dark_count_lone_hits', params)
    return True


def noise_lone_hits_from(config, params=None):
    """True when config['noise_lone_hits'] asks for the noise-hit seeds of the lone-hit rows; raises ValueError when it
    does and they cannot be had: without config['noise_model'] (a drawn model: a noise table has no value at an absolute sample), with
    enable_noise off, or below the right_raw_extension bound of the lone-hit passes.  Independent of 'dark_count_lone_hits'."""
    if not config.get('noise_lone_hits', False):
        return False
    if config.get('noise_model') is None:
        raise ValueError("noise_lone_hits: needs config['noise_model'] (a noise table has no value between the rows)")
    if not config.get('enable_noise', True):
        raise ValueError('noise_lone_hits: enable_noise is off')
    if params is None:
        from .config import kernel_params
        params = kernel_params(config)
    _lone_window_bounds('noise_lone_hits', params)
    return True


def _lone_window_bounds(key, params):
    """the bounds a lone-hit pass of RawData puts on the configuration; key: the config key that asks for the pass"""
    # A new window begins where a cluster's first time lies more than right_raw_extension (rext) behind the end of the last pulse,
    # (a_hi - tw) dt for rows that end at sample a_hi.  A pulse begins `before` + samples_to_store_before samples ahead of its first
    # photon, a row tw ahead of that, and a window's left may go one sample down to an even one: the next window's rows begin at
    # b_lo >= a_hi + rext / dt - (2 tw + before + store_before + 2).  From rext >= (2 G + 64) dt = (2 tlen + 4 tw + 64) dt follows
    # b_lo - a_hi >= G + tlen + (64 - before - store_before - 2), which is more than G + tlen - 1 while before + store_before + 2 < 64:
    #  * a pulse (tlen samples) or a row's margins (G in all) cannot reach from the rows of one window into those of the next, so a
    #    lone row meets at most one window at either end -- what the single window look-up of k_lone_scan / k_lone_rows relies on
    #    (wfs_lone_hits checks the distance of the windows it is given);
    #  * a photon that starts within G samples behind a window ends in front of the next one's rows, so RawData can end a batch's
    #    pass G samples behind the batch's last window without knowing the next.
    # 64, a cell, is the slack that pays for `before` and samples_to_store_before.
    if int(params['samples_before']) + int(params['store_before']) + 2 >= CELL:
        raise ValueError(f'{key}: samples_to_store_before + samples_before_pulse_center + 2 must stay below 64 '
                         '(the bound on right_raw_extension assumes it)')
    need = lone_min_rext(params)
    if int(params['rext']) < need:
        raise ValueError(f"{key}: right_raw_extension {int(params['rext'])} ns below (2 G + 64) dt = {need} ns "
                         f"(G = tlen + 2 trigger_window = {lone_gap(params)} samples)")
