"""PMT dark counts (config 'dark_count_rate') without a device: the thresholds of wfsim_amd/dark_counts.py against scipy, the
mu limit and the error cases, the statistics of the restatement (tests/dark_counts.py) over a fixed seed, and the Philox sites.

The seed of the statistics, 20261020, was chosen here on the CPU before any device run; with it the chi-square test of the offsets
gives p = 0.66 (printed by the test).
"""
import os
import re

import numpy as np
import pytest

from tests import dark_counts as DK
from wfsim_amd import dark_counts as DC
from wfsim_amd.config import kernel_params, xenonnt_test_config

SEED = 20261020
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thresholds_against_scipy():
    """floor(2^32 P(N >= k)) within 2 words of scipy's survival function for mu from 1e-9 to 1/8 -- relative to the value too, so that
    a small mu lost to cancellation (1 - sum_{i < k} is 0 or 2^-53 steps there) would show"""
    from scipy.stats import poisson
    for mu in np.concatenate([10.0 ** np.arange(-9, 0), np.linspace(1e-3, 0.125, 40), [0.125]]):
        got = DC.thresholds_of_mu(mu).astype(np.float64)
        ref = np.array([poisson.sf(k - 1, mu) for k in range(1, 5)]) * 2.0 ** 32
        assert np.all(np.abs(got - np.floor(ref)) <= 2), (mu, got, ref)
        # the tail itself to 1e-12 of its value: 1 - cdf keeps no more than 2^-53 / mu of it at mu = 1e-9
        mine = np.array([DC.tail(mu, k) for k in range(1, 5)])
        exact = np.array([poisson.sf(k - 1, mu) for k in range(1, 5)])
        assert np.all(np.abs(mine - exact) <= 1e-12 * exact), (mu, mine, exact)
    assert DC.thresholds_of_mu(1e-9)[0] == 4 and not DC.thresholds_of_mu(0.0).any()
    t = DC.thresholds_of_mu(0.125)
    assert t[0] > t[1] > t[2] > t[3] > 0


def test_mass_above_four_is_small():
    from scipy.stats import poisson
    assert poisson.sf(4, DC.MU_MAX) < 2.6e-7


def test_limit_and_errors():
    assert DC.max_rate(10) == pytest.approx(0.125 / 640e-9)
    DC.thresholds_of_mu(DC.MU_MAX)
    for bad in (DC.MU_MAX * (1 + 1e-12), -1e-9, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            DC.thresholds_of_mu(bad)
    with pytest.raises(ValueError, match='negative or not finite'):
        DC.rates_array([1.0, -2.0], 494)
    with pytest.raises(ValueError, match='negative or not finite'):
        DC.rates_array(float('nan'), 494)
    with pytest.raises(ValueError, match='at most 494'):
        DC.rates_array(np.ones(495), 494)
    with pytest.raises(ValueError, match='at most 494'):
        DC.rates_array(np.ones((2, 3)), 494)
    assert DC.rates_array(150.0, 494).shape == (494,) and DC.thresholds(150.0, 494, 10).shape == (494, 4)
    cfg = xenonnt_test_config()
    assert DC.rates_from(cfg) is None and DC.rates_from(dict(cfg, dark_count_rate=0.0)) is None
    assert DC.rates_from(dict(cfg, dark_count_rate=np.zeros(494))) is None
    r = DC.rates_from(dict(cfg, dark_count_rate=[10.0, 0.0, 30.0]))
    assert r.tolist() == [10.0, 0.0, 30.0]
    assert len(DC.rates_from(dict(cfg, dark_count_rate=200.0))) == 494
    with pytest.raises(ValueError, match='more than 1/8'):
        DC.rates_from(dict(cfg, dark_count_rate=DC.max_rate(10) * 1.01))


def _dark(mu, n_channels=8):
    cfg = xenonnt_test_config(seed=SEED)
    return DK.Dark.of_config(cfg, np.tile(DC.thresholds_of_mu(mu), (n_channels, 1))), kernel_params(cfg)


@pytest.mark.parametrize('mu', [0.125, 0.01])
def test_count_of_a_million_cells(mu):
    """N cells hold Poisson(N mu) photons up to the fold at 4 (N * 2.6e-7 < 0.3 photons): within 5 sqrt(N mu) of N mu"""
    dark, p = _dark(mu)
    N = 10 ** 6
    n = dark.counts(5, np.arange(-N // 2, N - N // 2, dtype=np.int64))
    assert n.max() <= 4 and abs(int(n.sum()) - N * mu) <= 5 * np.sqrt(N * mu), (int(n.sum()), N * mu)
    hist = np.bincount(n, minlength=5)
    from scipy.stats import poisson
    exp = N * np.append(poisson.pmf(np.arange(4), mu), poisson.sf(3, mu))
    assert np.all(np.abs(hist - exp) <= 5 * np.sqrt(exp) + 1), (hist, exp)


def test_offsets_are_uniform_and_gains_follow_the_spe_row():
    from scipy.stats import chi2
    dark, p = _dark(0.125)
    ph = dark.photons(5, 0, 400000)
    off = ph['t_ns'] - ph['m'] * 64 * p['dt']
    assert off.min() >= 0 and off.max() < 64 * p['dt'] and len(off) > 40000
    obs = np.bincount(off, minlength=64 * p['dt']).astype(np.float64)
    e = len(off) / len(obs)
    pv = float(chi2.sf(((obs - e) ** 2 / e).sum(), len(obs) - 1))
    print(f'chi-square of {len(off)} offsets over {len(obs)} bins: p = {pv:.3g}')
    assert pv > 1e-4
    assert np.array_equal(ph['idx'], ph['m'] * 64 + off // p['dt']) and np.array_equal(ph['r'], off % p['dt'])
    # the gain: gains[ch] times a uniformly drawn entry 1 .. 2000 of the SPE row -- the mean within 5 standard errors of the row's
    row = dark.spe_row(5)[1:] * dark.gains[5]
    assert abs(ph['gain'].mean() - row.mean()) <= 5 * row.std() / np.sqrt(len(off))
    assert np.all(np.isin(ph['gain'], row))


def test_samples_are_the_sum_of_single_pulses():
    """D of a range is the sum of the photons' own rounded pulses, wherever the range is cut"""
    dark, p = _dark(0.125)
    whole = dark.samples(5, -3000, 9000)
    assert whole.min() < -15 and np.count_nonzero(whole) > 100          # single-PE pulses beyond the ZLE threshold of 15 counts
    for a, n in ((-3000, 1), (-2999, 255), (-1, 2), (0, 64), (63, 130), (5000, 1000)):
        assert np.array_equal(dark.samples(5, a, n), whole[a + 3000:a + 3000 + n])
    t, g = dark.photons_in(5, -3000, 9000)
    assert np.all(np.diff(t) >= 0) and len(t) == len(dark.photons(5, -3000 >> 6, 5999 >> 6)['t_ns'])
    k = int(np.argmax(np.diff(t) > 400))                    # a photon with nothing within 40 samples behind it
    idx, r = int(t[k] // p['dt']), int(t[k] % p['dt'])
    if k == 0 or t[k] - t[k - 1] > 400:
        own = -np.rint(g[k] * dark.templates[r] * dark.c2a).astype(np.int64)
        assert np.array_equal(dark.samples(5, idx - p['samples_before'], p['tlen']), own)


def test_sites_collide_with_nothing():
    """112 .. 115 are named by no other stream of DESIGN 4 and of the device's site list"""
    src = open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_device.h')).read()
    enum = src[src.index('enum WfsSite'):src.index('};', src.index('enum WfsSite'))]
    enum = re.sub(r'//[^\n]*', '', enum)
    sites = {name: int(v) for name, v in re.findall(r'(SITE_\w+)\s*=\s*(\d+)', enum)}
    spans = {'SITE_AP': 8, 'SITE_AP_SCREEN': 2, 'SITE_AP_X': 8, 'SITE_NOISE_SLOW': 8, 'SITE_NOISE_SLOW_COMMON': 8}      # sites that are the first of a run
    taken = set()
    for name, v in sites.items():
        taken |= set(range(v, v + spans.get(name, 1)))
    assert len(sites) >= 20 and max(taken) == 103
    assert not taken & {112, 113, 114, 115}
    assert (DC.SITE_COUNT, DC.SITE_PHOTON) == (112, 113) == (DK.SITE_COUNT, DK.SITE_PHOTON)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'112.{0,200}dark', design, re.S) and '3e' in design
