"""The coloured noise model on the CPU: what wfsim_amd.noise_model makes of config['noise_model'] ('taps', 'common'), its refusals, and the
statistics of the numpy restatement (tests/noise_colour.py) that the device is compared with sample by sample in
tests/test_gpu_noise_colour.py.

The statistical bounds are 5 sqrt(B / n), B Bartlett's variance factor of the sample correlation computed from the PREDICTED correlation
functions (NC.bartlett_factor): five standard deviations of the estimator, not a figure taken from the samples.  On the 2^20 samples
under NC.STAT_SEED the largest deviation is 2.3 of these standard deviations (the autocorrelation at lag 8, printed by the test).
"""
import numpy as np
import pytest

from tests import noise_colour as NC
from tests import noise_model as NM
from wfsim_amd.noise_model import (Q16, check_colour, gaussian_pmf, noise_colour, noise_pmf, quantise_taps, taps_from_psd, unit_power)

N_CH = 6
GAINS = [1.0] * N_CH


def _cfg(**model):
    return {'gains': GAINS, 'noise_model': model}


# ---------------------------------------------------------------------------------------------------- parsing
def test_white_models_have_no_colour():
    assert noise_colour({'gains': GAINS}, 801) is None
    assert noise_colour(_cfg(sigma=2.0), 801) is None
    assert noise_colour(_cfg(pmf=np.full((2, 4), 0.25), vmin=-1), 801) is None


def test_taps_for_all_channels_and_per_channel():
    h = [0.25, -0.5, 1.0 / 3.0]
    c = noise_colour(_cfg(sigma=2.0, taps=h), 801)
    assert c['taps_q'].dtype == np.int32 and c['taps_q'].shape == (N_CH, 3)
    assert np.array_equal(c['taps_q'], np.tile([16384, -32768, 21845], (N_CH, 1)))          # round(h * 65536)
    assert np.all(c['group'] == -1) and np.all(c['mix_q'] == 0) and c['common_pmf'].shape == (0, 25)
    per = np.arange(N_CH * 2).reshape(N_CH, 2) / 16.0
    c = noise_colour(_cfg(sigma=2.0, taps=per), 801)
    assert np.array_equal(c['taps_q'], (per * Q16).astype(np.int64))
    assert np.array_equal(quantise_taps([0.5 / Q16, 1.5 / Q16, -0.5 / Q16, -1.5 / Q16, 0.49 / Q16]), [1, 2, 0, -1, 0])       # half up


def test_common_forms_and_zero_padding():
    groups = np.array([0, 0, 1, -1, 1, 0])
    c = noise_colour(_cfg(sigma=2.0, taps=[1.0, 0.5], common=dict(groups=groups, gain=0.5, sigma=3.0, taps=[0.5, 0.25, 0.125, 1.0])), 801)
    assert c['taps_q'].shape == (N_CH + 2, 4)                                      # the longer of the two, the shorter rows zero-padded
    assert np.array_equal(c['taps_q'][:N_CH], np.tile([65536, 32768, 0, 0], (N_CH, 1)))
    assert np.array_equal(c['taps_q'][N_CH:], np.tile([32768, 16384, 8192, 65536], (2, 1)))
    assert np.array_equal(c['group'], groups) and np.array_equal(c['mix_q'], np.where(groups >= 0, 32768, 0))
    # one gaussian_pmf call for channels and groups: the same half (6 * 3.0 = 18), and the white model's pmf is on it too
    pmf, vmin = noise_pmf(_cfg(sigma=2.0, common=dict(groups=groups, gain=0.5, sigma=3.0)), 801)
    both, vmin_b = gaussian_pmf([2.0] * N_CH + [3.0, 3.0])
    assert vmin == vmin_b == -18 and np.array_equal(pmf, both[:N_CH]) and np.array_equal(c['common_pmf'], both[N_CH:])
    # per-group sigma, per-channel gain, per-group taps, a common part without channel taps (one unit tap, padded)
    gain = np.array([0.5, -1.0, 0.25, 0.9, 1.0, 0.0])
    c = noise_colour(_cfg(sigma=[2.0] * N_CH, common=dict(groups=groups, gain=gain, sigma=[1.0, 3.0], taps=[[1.0, 0.5], [0.25, 0.0]])), 801)
    assert np.array_equal(c['taps_q'], [[65536, 0]] * N_CH + [[65536, 32768], [16384, 0]])
    assert np.array_equal(c['mix_q'], [32768, -65536, 16384, 0, 65536, 0])          # no group: no gain
    assert np.array_equal(c['common_pmf'], gaussian_pmf([2.0] * N_CH + [1.0, 3.0])[0][N_CH:])
    # the 'pmf' form on the model's values
    pmf = np.full((N_CH, 5), 0.2)
    cp = np.array([[0.0, 0.25, 0.5, 0.25, 0.0], [0.5, 0.0, 0.0, 0.0, 0.5]])
    c = noise_colour(_cfg(pmf=pmf, vmin=-2, common=dict(groups=groups, gain=1.0, pmf=cp)), 801)
    assert np.array_equal(c['common_pmf'], cp) and np.array_equal(c['taps_q'], [[65536]] * (N_CH + 2))


@pytest.mark.parametrize('model,match', [
    (dict(sigma=2.0, taps=np.ones(17)), 'more than 16'),
    (dict(sigma=2.0, taps=np.ones((5, 2))), r"noise_model\['taps'\] must be"),
    (dict(sigma=2.0, taps=[1.0, np.nan]), 'finite'),
    (dict(sigma=2.0, taps=[[]] * N_CH), r"noise_model\['taps'\] must be"),
    (dict(sigma=2.0, common=dict(groups=[0] * N_CH, gain=1.0)), "either 'sigma' or 'pmf'"),
    (dict(sigma=2.0, common=dict(groups=[0] * N_CH, gain=1.0, sigma=1.0, pmf=[[1.0]])), "either 'sigma' or 'pmf'"),
    (dict(sigma=2.0, common=dict(gain=1.0, sigma=1.0)), "'groups', 'gain'"),
    (dict(sigma=2.0, common=dict(groups=[0] * 5, gain=1.0, sigma=1.0)), r"\['groups'\] must be an integer array \[6\]"),
    (dict(sigma=2.0, common=dict(groups=[0.0] * N_CH, gain=1.0, sigma=1.0)), r"\['groups'\] must be an integer array"),
    (dict(sigma=2.0, common=dict(groups=[0, -2, 0, 0, 0, 0], gain=1.0, sigma=1.0)), 'below -1'),
    (dict(sigma=2.0, common=dict(groups=[0] * N_CH, gain=[1.0] * 5, sigma=1.0)), r"\['gain'\] must be"),
    (dict(sigma=2.0, common=dict(groups=[0] * N_CH, gain=1.5, sigma=1.0)), r'mix_q of channel 0 beyond 65536'),
    (dict(sigma=2.0, common=dict(groups=[0, 1, 0, 0, 0, 0], gain=1.0, sigma=[1.0, 1.0, 1.0])), r"\['sigma'\] must be a number or an array \[2\]"),
    (dict(sigma=2.0, common=dict(groups=[0] * N_CH, gain=1.0, sigma=1.0, taps=np.ones((2, 3)))), r"\['common'\]\['taps'\] must be"),
    (dict(sigma=2.0, common=dict(groups=[0] * N_CH, gain=1.0, pmf=np.full((1, 3), 1 / 3))), r"\['pmf'\] must be \[1\]\[25\]"),
    (dict(pmf=np.full((N_CH, 4), 0.25), vmin=0, common=dict(groups=[0] * N_CH, gain=1.0, sigma=1.0)), "needs the channels given by 'sigma'"),
    (dict(pmf=np.full((N_CH, 4), 0.25), vmin=0, common=dict(groups=[0] * N_CH, gain=1.0, pmf=np.full((1, 5), 0.2))), r"\['pmf'\] must be \[1\]\[4\]"),
    (dict(pmf=np.full((N_CH, 4), 0.25), vmin=0, common=dict(groups=[0] * N_CH, gain=1.0, pmf=[[0.5, 0.6, -0.1, 0.0]])), 'common_pmf has a negative'),
    (dict(pmf=np.full((N_CH, 4), 0.25), vmin=0, common=dict(groups=[0, 1, 0, 0, 0, 0], gain=1.0, pmf=[[0.25] * 4, [0.25, 0.25, 0.25, 0.25 + 1e-8]])),
     'common_pmf of group 1 does not sum to 1'),
    (dict(sigma=100.0, taps=[14.0]), r'taps_q of row 0: sum \|taps\| \* max \|value\|'),
])
def test_refusals(model, match):
    with pytest.raises(ValueError, match=match):
        noise_colour(_cfg(**model), 801)


def test_overflow_bound_at_its_edge():
    # values -1 .. 1: max |value| = 1, so the bound is on sum |taps_q| itself
    cp, grp, mix = np.zeros((0, 3)), np.full(2, -1), np.zeros(2)
    row = np.full(16, 2 ** 25, dtype=np.int64)                 # sum = 2^29
    row[3] = -row[3]
    edge = row.copy()
    edge[7] -= 1                                               # 2^29 - 1
    t, g, m, c = check_colour(np.stack([edge, edge]), grp, mix, cp, 2, 3, -1)
    assert t.dtype == np.int32 and np.array_equal(t[0], edge) and int(np.abs(t[0]).sum()) == 2 ** 29 - 1
    with pytest.raises(ValueError, match=r'taps_q of row 1: sum \|taps\| \* max \|value\| = 536870912 reaches 2\^29'):
        check_colour(np.stack([edge, row]), grp, mix, cp, 2, 3, -1)
    # and with max |value| = 12 the same figure bounds the product
    at = (2 ** 29 - 1) // 12
    check_colour([[at], [-at]], grp, mix, np.zeros((0, 25)), 2, 25, -12)
    with pytest.raises(ValueError, match='taps_q of row 1'):
        check_colour([[at], [-at - 1]], grp, mix, np.zeros((0, 25)), 2, 25, -12)
    with pytest.raises(ValueError, match='n_taps 17 outside'):
        check_colour(np.ones((2, 17)), grp, mix, cp, 2, 3, -1)
    with pytest.raises(ValueError, match='group of channel 1 outside -1 .. -1'):
        check_colour(np.ones((2, 1)), [-1, 0], mix, cp, 2, 3, -1)
    with pytest.raises(ValueError, match='mix_q of channel 0'):
        check_colour(np.ones((3, 1)), [0, 0], [-65537, 0], [[0.5, 0.0, 0.5]], 2, 3, -1)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_unit_tap_is_the_white_restatement():
    pmf, vmin = gaussian_pmf([2.2, 0.0, 5.1])
    model = NC.colour_model(pmf, vmin, noise_colour({'gains': [1.0] * 3, 'noise_model': {'sigma': [2.2, 0.0, 5.1], 'taps': [1.0]}}, 801))
    thr, alias, shift = NM.build_cells(pmf)
    for t0 in (0, -7, 2 ** 34 - 5):
        t = t0 + np.arange(1000, dtype=np.int64)
        for ch in range(3):
            white = NM.noise_values((thr[ch], alias[ch]), shift, vmin, 77, ch, t)
            assert np.array_equal(NC.colour_values(model, 77, ch, t), white) and np.array_equal(NC.white_values(model, 77, ch, t), white)
    assert np.array_equal(NC.colour_values(NC.colour_model(pmf, vmin), 77, 2, t), white)          # no colour at all: the same model


def test_restatement_by_hand():
    """the definition term by term on a few samples, common stream and negative t included"""
    groups = np.array([0, -1, 0])
    cfg = {'gains': [1.0] * 3, 'noise_model': {'sigma': [2.0, 3.0, 1.0], 'taps': [[0.5, 0.25, -0.125], [1.0, 0.0, 0.0], [0.3, 0.3, 0.3]],
                                               'common': dict(groups=groups, gain=[0.5, 0.0, -1.0], sigma=2.5, taps=[0.6, 0.4])}}
    pmf, vmin = noise_pmf(cfg, 801)
    col = noise_colour(cfg, 801)
    model = NC.colour_model(pmf, vmin, col)
    seed = 5
    for ch in range(3):
        for t in (-5, 0, 3, 2 ** 34):
            F = sum(int(col['taps_q'][ch][k]) * int(NC.white_values(model, seed, ch, [t - k])[0]) for k in range(3))
            C = 0
            if groups[ch] >= 0:
                Fc = sum(int(col['taps_q'][3][k]) * int(NC.white_values(model, seed, 3, [t - k])[0]) for k in range(3))
                C = (int(col['mix_q'][ch]) * Fc) >> 16
            assert int(NC.colour_values(model, seed, ch, np.array([t]))[0]) == (F + C + 32768) >> 16
    a = NC.colour_values(model, seed, 0, np.arange(-40, 40, dtype=np.int64))
    assert np.array_equal(a[10:50], NC.colour_values(model, seed, 0, np.arange(-30, 10, dtype=np.int64)))         # a function of t alone


# ---------------------------------------------------------------------------------------------------- statistics of the restatement
# (taps without a short common denominator: with h = 0.5, 0.8, ... the sum is a multiple of 0.1, its rounding error takes ten values that
# follow the whites, and the "1/12 of white variance" of the prediction is off by more than the bound resolves -- 12 sd at lag 1)
STAT_TAPS = [0.4871, 0.8123, 0.3057, -0.4219, 0.1993]
STAT_COMMON_TAPS = [0.6137, 0.5871, 0.4923]
STAT_GAIN = [0.7431, -0.5129, 0.7431, 0.0]
STAT_GROUPS = [0, 0, 1, -1]


@pytest.fixture(scope='module')
def stat():
    cfg = {'gains': [1.0] * 4, 'noise_model': {'sigma': [3.0, 2.0, 3.0, 3.0], 'taps': STAT_TAPS,
                                               'common': dict(groups=STAT_GROUPS, gain=STAT_GAIN, sigma=[2.5, 2.5], taps=STAT_COMMON_TAPS)}}
    pmf, vmin = noise_pmf(cfg, 801)
    col = noise_colour(cfg, 801)
    model = NC.colour_model(pmf, vmin, col)
    t = NC.STAT_T0 + np.arange(NC.STAT_N, dtype=np.int64)
    x = [NC.colour_values(model, NC.STAT_SEED, ch, t) for ch in range(4)]
    values = vmin + np.arange(pmf.shape[1])
    var = lambda row: float((row * values ** 2).sum() - (row * values).sum() ** 2)
    var_w, var_c = [var(r) for r in pmf], [var(r) for r in col['common_pmf']]
    hq, hc = col['taps_q'][0] / Q16, col['taps_q'][4] / Q16              # the taps as quantised

    def gamma(a, b):
        """predicted covariance function of channels a and b on signed lags"""
        def g(v):
            v = abs(int(v))
            own = var_w[a] * NC.tap_autocorr(hq, v) + (1.0 / 12.0 if v == 0 else 0.0) if a == b else 0.0
            ga, gb = STAT_GROUPS[a], STAT_GROUPS[b]
            mix = col['mix_q'][a] / Q16 * col['mix_q'][b] / Q16
            return own + (mix * var_c[ga] * NC.tap_autocorr(hc, v) if ga >= 0 and ga == gb else 0.0)
        return g

    def rho(a, b):
        ga, gb, gab = gamma(a, a), gamma(b, b), gamma(a, b)
        return lambda v: gab(v) / np.sqrt(ga(0) * gb(0))
    return x, rho, gamma, var_w, var_c


def test_autocorrelation_follows_the_taps(stat):
    x, rho, gamma, var_w, var_c = stat
    L, n = len(STAT_TAPS), NC.STAT_N
    worst = 0.0
    for ch in (3, 0):                                          # without a group: r_h(lag) Var_w / (r_h(0) Var_w + 1/12); with one: the sum of both parts
        r = rho(ch, ch)
        if ch == 3:
            for lag in range(1, L + 5):
                assert r(lag) == pytest.approx(NC.tap_autocorr(STAT_TAPS, lag) * var_w[3] / (NC.tap_autocorr(STAT_TAPS, 0) * var_w[3] + 1 / 12), abs=1e-4)
        for lag in range(1, L + 5):
            got, B = NC.sample_autocorr(x[ch], lag), NC.bartlett_factor(r, r, r, lag)
            bound = 5.0 * np.sqrt(B / n)
            print(f'channel {ch} lag {lag}: {got:+.5f} predicted {r(lag):+.5f} bound {bound:.5f} ({abs(got - r(lag)) / np.sqrt(B / n):.2f} sd)')
            worst = max(worst, abs(got - r(lag)) / np.sqrt(B / n))
            assert abs(got - r(lag)) <= bound, (ch, lag)
        assert abs(r(1)) > 0.3 and r(L + 1) == 0.0             # coloured inside the filter, nothing beyond it
    print(f'worst {worst:.2f} sd')


def test_channel_correlations(stat):
    x, rho, gamma, var_w, var_c = stat
    n = NC.STAT_N
    for a, b in ((0, 1), (0, 2), (0, 3), (2, 3)):             # one group (gains of opposite sign) / different groups / a channel with none
        rab = rho(a, b)
        got, B = NC.sample_corr(x[a], x[b]), NC.bartlett_factor(rho(a, a), rho(b, b), rab, 0)
        bound = 5.0 * np.sqrt(B / n)
        print(f'channels {a}, {b}: {got:+.5f} predicted {rab(0):+.5f} bound {bound:.5f}')
        assert abs(got - rab(0)) <= bound, (a, b)
        assert (rab(0) < -0.1) if (a, b) == (0, 1) else (rab(0) == 0.0)
    # the variance of a channel: Var_w sum h^2 + gain^2 Var_c sum h_c^2 + 1/12 (the taps as quantised: 2^-17 apart from those given);
    # bound: five standard errors of the variance estimate of a Gaussian series with the predicted correlation function
    for ch in (0, 3):
        g0, r = gamma(ch, ch)(0), rho(ch, ch)
        doc = var_w[ch] * sum(np.square(STAT_TAPS)) + (STAT_GAIN[ch] ** 2 * var_c[0] * sum(np.square(STAT_COMMON_TAPS)) if ch == 0 else 0.0) + 1 / 12
        assert g0 == pytest.approx(doc, rel=1e-4)
        se = g0 * np.sqrt(2.0 * sum(r(v) ** 2 for v in range(-20, 21)) / n)
        print(f'channel {ch}: variance {np.var(x[ch]):.4f} predicted {g0:.4f} bound {5 * se:.4f}')
        assert abs(np.var(x[ch]) - g0) <= 5 * se, (ch, np.var(x[ch]), g0)


# ---------------------------------------------------------------------------------------------------- helpers for users
def test_unit_power():
    assert np.allclose((unit_power([3.0, 4.0]) ** 2).sum(), 1.0) and np.allclose(unit_power([3.0, 4.0]), [0.6, 0.8])
    u = unit_power([[1.0, 1.0], [2.0, 0.0]])
    assert np.allclose((u ** 2).sum(axis=1), 1.0)
    with pytest.raises(ValueError, match='zeros'):
        unit_power([[0.0, 0.0]])


def test_taps_from_psd_recovers_known_taps():
    h = unit_power([0.1, 0.35, 0.6, 0.35, 0.1])                # symmetric, unit power
    dt_ns = 10
    grid = np.fft.rfftfreq(5, d=dt_ns * 1e-9)
    psd = np.abs(np.fft.rfft(h)) ** 2
    got = taps_from_psd(grid, psd, 5, dt_ns)
    assert got.shape == (5,) and (got ** 2).sum() == pytest.approx(1.0, abs=1e-12)
    assert np.allclose(np.abs(np.fft.rfft(got)) ** 2, psd, rtol=1e-9, atol=0)
    assert np.allclose(got, got[::-1], atol=1e-12)             # linear phase
    assert np.allclose(got, h, atol=1e-9)                      # (the zero-phase response of these taps is positive on the grid: the taps themselves return)
    # a scaled psd on a finer frequency axis gives the same taps: unit power
    fine = np.linspace(0, grid[-1], 201)
    assert np.allclose(taps_from_psd(fine, 7.0 * np.interp(fine, grid, psd), 5, dt_ns), got, atol=1e-9)
    flat = taps_from_psd([0.0, 5e7], [2.0, 2.0], 8, dt_ns)      # a white spectrum: one tap
    assert np.allclose(np.sort(np.abs(flat)), [0] * 7 + [1.0], atol=1e-12)
    with pytest.raises(ValueError, match='n_taps'):
        taps_from_psd([0.0, 1.0], [1.0, 1.0], 17)
    with pytest.raises(ValueError, match='increasing'):
        taps_from_psd([1.0, 0.0], [1.0, 1.0], 4)
