"""The slow levels of the noise model on the CPU: what wfsim_amd.noise_model makes of config['noise_model']['slow'] (and of 'slow' under
'common'), its refusals, and the statistics of the numpy restatement (tests/noise_slow.py) that the device is compared with sample by
sample in tests/test_gpu_noise_slow.py.

The statistical bounds are 5 sqrt(B / n), B Bartlett's variance factor (NC.bartlett_factor) computed from the PREDICTED correlation
functions; the predictions come from NS.level_autocov, an enumeration of the interpolation weights over the phase, not a closed form.
The seeds are fixed; the figures the restatement gives under them are printed by each test.
"""
import numpy as np
import pytest

from tests import noise_colour as NC
from tests import noise_model as NM
from tests import noise_slow as NS
from wfsim_amd.noise_model import (Q16, check_slow, gaussian_pmf, noise_colour, noise_pmf, noise_slow, slow_level_variance, slow_levels)

N_CH = 6
GAINS = [1.0] * N_CH


def _cfg(**model):
    return {'gains': GAINS, 'noise_model': model}


def _model(cfg):
    pmf, vmin = noise_pmf(cfg, 801)
    return NS.slow_model(pmf, vmin, noise_colour(cfg, 801), noise_slow(cfg, 801))


# ---------------------------------------------------------------------------------------------------- parsing
def test_models_without_the_key_have_no_levels():
    assert noise_slow({'gains': GAINS}, 801) is None
    assert noise_slow(_cfg(sigma=2.0), 801) is None
    assert noise_slow(_cfg(sigma=2.0, taps=[0.5, 0.5]), 801) is None


def test_forms_and_quantisation():
    s = noise_slow(_cfg(sigma=2.0, slow=dict(shifts=[4, 6, 10], amplitude=[0.25, -0.5, 1.0 / 3.0])), 801)
    assert s['shifts'].dtype == np.int32 and np.array_equal(s['shifts'], [4, 6, 10])
    assert s['slow_q'].dtype == np.int32 and np.array_equal(s['slow_q'], np.tile([16384, -32768, 21845], (N_CH, 1)))         # round(a * 65536)
    assert noise_colour(_cfg(sigma=2.0, slow=dict(shifts=[4], amplitude=[1.0])), 801) is None                                  # levels are no colour
    per = np.arange(N_CH * 2).reshape(N_CH, 2) / 16.0
    s = noise_slow(_cfg(sigma=2.0, slow=dict(shifts=[5, 30], amplitude=per)), 801)
    assert np.array_equal(s['slow_q'], (per * Q16).astype(np.int64))
    # periods in ns: dt * 2^s, with the configured sample duration
    s = noise_slow(_cfg(sigma=2.0, slow=dict(period_ns=[160, 640, 10240], amplitude=[1.0, 1.0, 1.0])), 801)
    assert np.array_equal(s['shifts'], [4, 6, 10])
    s = noise_slow(dict(_cfg(sigma=2.0, slow=dict(period_ns=128, amplitude=[1.0])), sample_duration=2), 801)
    assert np.array_equal(s['shifts'], [6])
    # common streams: rows behind the channels', zero unless given
    groups = np.array([0, 0, 1, -1, 1, 0])
    common = dict(groups=groups, gain=0.5, sigma=3.0)
    s = noise_slow(_cfg(sigma=2.0, slow=dict(shifts=[4, 8], amplitude=[0.5, 0.0]), common=common), 801)
    assert s['slow_q'].shape == (N_CH + 2, 2) and np.all(s['slow_q'][N_CH:] == 0) and np.all(s['slow_q'][:N_CH] == [32768, 0])
    s = noise_slow(_cfg(sigma=2.0, slow=dict(shifts=[4, 8], amplitude=[0.0, 0.0]), common=dict(common, slow=[1.0, 0.25])), 801)
    assert np.array_equal(s['slow_q'][N_CH:], [[65536, 16384]] * 2) and np.all(s['slow_q'][:N_CH] == 0)
    s = noise_slow(_cfg(sigma=2.0, slow=dict(shifts=[4, 8], amplitude=[0.0, 0.0]), common=dict(common, slow=[[1.0, 0.25], [0.0, -1.0]])), 801)
    assert np.array_equal(s['slow_q'][N_CH:], [[65536, 16384], [0, -65536]])


@pytest.mark.parametrize('model,match', [
    (dict(sigma=2.0, slow=dict(shifts=[4])), "'amplitude' and either 'shifts' or 'period_ns'"),
    (dict(sigma=2.0, slow=dict(amplitude=[1.0])), "'amplitude' and either 'shifts' or 'period_ns'"),
    (dict(sigma=2.0, slow=dict(shifts=[4], period_ns=[160], amplitude=[1.0])), "'amplitude' and either 'shifts' or 'period_ns'"),
    (dict(sigma=2.0, slow=[4]), "'amplitude' and either 'shifts' or 'period_ns'"),
    (dict(sigma=2.0, slow=dict(shifts=[4.0], amplitude=[1.0])), r"\['shifts'\] must be a 1-D integer array"),
    (dict(sigma=2.0, slow=dict(shifts=[[4]], amplitude=[1.0])), r"\['shifts'\] must be a 1-D integer array"),
    (dict(sigma=2.0, slow=dict(shifts=np.zeros(0, dtype=np.int64), amplitude=[])), r'n_levels 0 outside 1 \.\. 8'),
    (dict(sigma=2.0, slow=dict(shifts=list(range(4, 13)), amplitude=[0.0] * 9)), r'n_levels 9 outside 1 \.\. 8'),
    (dict(sigma=2.0, slow=dict(shifts=[3, 5], amplitude=[1.0, 1.0])), r'shifts\[0\] = 3 outside 4 \.\. 30'),
    (dict(sigma=2.0, slow=dict(shifts=[5, 31], amplitude=[1.0, 1.0])), r'shifts\[1\] = 31 outside 4 \.\. 30'),
    (dict(sigma=2.0, slow=dict(shifts=[5, 5], amplitude=[1.0, 1.0])), 'not strictly ascending at level 1'),
    (dict(sigma=2.0, slow=dict(shifts=[5, 8, 7], amplitude=[1.0] * 3)), 'not strictly ascending at level 2'),
    (dict(sigma=2.0, slow=dict(period_ns=[150], amplitude=[1.0])), r"\['period_ns'\]\[0\] = 150 ns is not dt \* 2\^s \(dt = 10 ns\)"),
    (dict(sigma=2.0, slow=dict(period_ns=[160, -160], amplitude=[1.0, 1.0])), r"\['period_ns'\]\[1\] = -160 ns is not dt \* 2\^s"),
    (dict(sigma=2.0, slow=dict(period_ns=[5], amplitude=[1.0])), r"\['period_ns'\]\[0\] = 5 ns is not dt \* 2\^s"),
    (dict(sigma=2.0, slow=dict(period_ns=[80], amplitude=[1.0])), r'shifts\[0\] = 3 outside 4 \.\. 30'),
    (dict(sigma=2.0, slow=dict(period_ns=[[160]], amplitude=[1.0])), r"\['period_ns'\] must be a number or a 1-D array"),
    (dict(sigma=2.0, slow=dict(shifts=[4, 6], amplitude=[1.0])), r"\['amplitude'\] must be a float array \[2\] or \[6\]\[2\]"),
    (dict(sigma=2.0, slow=dict(shifts=[4], amplitude=np.ones((5, 1)))), r"\['amplitude'\] must be a float array \[1\] or \[6\]\[1\]"),
    (dict(sigma=2.0, slow=dict(shifts=[4], amplitude=[np.inf])), r"\['amplitude'\] must be finite"),
    (dict(sigma=2.0, common=dict(groups=[0] * N_CH, gain=1.0, sigma=1.0, slow=[1.0])), r"\['common'\]\['slow'\] needs noise_model\['slow'\]"),
    (dict(sigma=2.0, slow=dict(shifts=[4], amplitude=[0.0]), common=dict(groups=[0] * N_CH, gain=1.0, sigma=1.0, slow=[1.0, 1.0])),
     r"\['common'\]\['slow'\] must be a float array \[1\] or \[1\]\[1\]"),
    (dict(sigma=100.0, slow=dict(shifts=[4], amplitude=[13.0])), r'slow_q of row 0: \(sum \|taps\| \+ sum \|slow\|\) \* max \|value\|'),
])
def test_refusals(model, match):
    with pytest.raises(ValueError, match=match):
        noise_slow(_cfg(**model), 801)


def test_overflow_bound_at_its_edge():
    # values -1 .. 1: max |value| = 1, so the bound is on sum |taps_q| + sum |slow_q| itself
    taps = np.full((2, 16), 2 ** 24, dtype=np.int64)            # sum |taps| = 2^28
    taps[:, 3] = -taps[:, 3]
    full = np.full(8, 2 ** 25, dtype=np.int64)                  # sum |slow| = 2^28: together 2^29
    full[2] = -full[2]
    edge = full.copy()
    edge[5] -= 1                                                # 2^29 - 1
    sh = np.arange(4, 12)
    s, q = check_slow(sh, np.stack([edge, edge]), taps, 2, 0, 3, -1)
    assert s.dtype == np.int32 and q.dtype == np.int32 and np.array_equal(q[1], edge)
    assert int(np.abs(taps[0]).sum() + np.abs(q[0]).sum()) == 2 ** 29 - 1
    with pytest.raises(ValueError, match=r'slow_q of row 1: \(sum \|taps\| \+ sum \|slow\|\) \* max \|value\| = 536870912 reaches 2\^29'):
        check_slow(sh, np.stack([edge, full]), taps, 2, 0, 3, -1)
    # without a colour the taps count as one unit tap: 65536
    at = 2 ** 29 - 1 - 65536
    check_slow([4], [[at], [-at]], None, 2, 0, 3, -1)
    with pytest.raises(ValueError, match='slow_q of row 1'):
        check_slow([4], [[at], [-at - 1]], None, 2, 0, 3, -1)
    # and with max |value| = 12 the same figure bounds the product
    at = (2 ** 29 - 1) // 12 - 65536
    check_slow([4], [[at], [-at]], None, 2, 0, 25, -12)
    with pytest.raises(ValueError, match='slow_q of row 0'):
        check_slow([4], [[at + 1], [-at]], None, 2, 0, 25, -12)
    # rows: channels, then the common streams of the colour
    with pytest.raises(ValueError, match=r'slow_q must be \[3\]\[1\]'):
        check_slow([4], [[1], [1]], np.ones((3, 1)), 2, 1, 3, -1)
    with pytest.raises(ValueError, match=r'slow_q must be \[2\]\[1\]'):
        check_slow([4], [[1], [1], [1]], None, 2, 0, 3, -1)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_zero_amplitudes_are_the_colour_and_the_white_restatement():
    pmf, vmin = gaussian_pmf([2.2, 0.0, 5.1])
    thr, alias, shift = NM.build_cells(pmf)
    base = {'gains': [1.0] * 3, 'noise_model': {'sigma': [2.2, 0.0, 5.1]}}
    zero = dict(shifts=[4, 9, 30], amplitude=[0.0, 0.0, 0.0])
    plain = dict(base, noise_model=dict(base['noise_model'], slow=zero))
    col = dict(taps=[0.5, -0.25, 0.7], common=dict(groups=np.array([0, -1, 0]), gain=[0.5, 0.0, -1.0], sigma=2.5, taps=[0.6, 0.4]))
    coloured = dict(base, noise_model=dict(base['noise_model'], slow=zero, **col))
    cm = NC.colour_model(*noise_pmf(coloured, 801), noise_colour(coloured, 801))
    for t0 in (0, -7, 2 ** 34 - 5):
        t = t0 + np.arange(1000, dtype=np.int64)
        for ch in range(3):
            white = NM.noise_values((thr[ch], alias[ch]), shift, vmin, 77, ch, t)
            assert np.array_equal(NS.slow_noise_values(_model(plain), 77, ch, t), white)
            assert np.array_equal(NS.slow_noise_values(_model(coloured), 77, ch, t), NC.colour_values(cm, 77, ch, t))
            assert not np.any(NS.slow_values(_model(coloured), 77, ch, t))
    assert np.array_equal(NS.slow_noise_values(NS.slow_model(pmf, vmin), 77, 2, t), white)          # no levels at all: the same model


def test_restatement_by_hand():
    """the definition term by term on a few samples: two levels, a common stream with a level of its own, negative t, a knot on t"""
    groups = np.array([0, -1, 0])
    cfg = {'gains': [1.0] * 3, 'noise_model': {'sigma': [2.0, 3.0, 1.0], 'taps': [[0.5, 0.25], [1.0, 0.0], [0.3, 0.3]],
                                               'slow': dict(shifts=[4, 7], amplitude=[[0.5, 1.5], [0.0, -2.0], [1.0, 0.0]]),
                                               'common': dict(groups=groups, gain=[0.5, 0.0, -1.0], sigma=2.5, taps=[0.6], slow=[0.0, 0.75])}}
    model, seed = _model(cfg), 5
    assert np.array_equal(model['slow_q'], [[32768, 98304], [0, -131072], [65536, 0], [0, 49152]])

    def knot(row, j, m):
        return int(NS.knot_values(model, seed, row, j, np.array([m]))[0])

    def S(row, t):
        total = 0
        for j, s in enumerate((4, 7)):
            m, f = t >> s, t & ((1 << s) - 1)                  # python's >> and & on negative ints are arithmetic / two's complement
            P0, P1 = int(model['slow_q'][row][j]) * knot(row, j, m), int(model['slow_q'][row][j]) * knot(row, j, m + 1)
            total += P0 + (((P1 - P0) * f) >> s)
        return total

    def F(row, t):
        w = NC.white_values(model, seed, row, np.array([t, t - 1]))
        return int(model['taps_q'][row][0]) * int(w[0]) + int(model['taps_q'][row][1]) * int(w[1]) + S(row, t)

    for t in (-130, -129, -128, -17, -16, -1, 0, 15, 16, 127, 128, 2 ** 34 - 1, 2 ** 34):
        for ch in range(3):
            g = int(groups[ch])
            c = (int(model['mix_q'][ch]) * F(3 + g, t)) >> 16 if g >= 0 else 0
            assert int(NS.slow_noise_values(model, seed, ch, np.array([t]))[0]) == (F(ch, t) + c + 32768) >> 16, (ch, t)
        assert int(NS.slow_values(model, seed, 3, np.array([t]))[0]) == S(3, t)
    # on a knot the value is the knot's; between two knots it moves monotonically from one to the other
    t = np.arange(-32, 33, dtype=np.int64)
    one = NS.slow_model(*noise_pmf(cfg, 801), None, dict(shifts=[4], slow_q=[[65536]] * 3))
    s = NS.slow_values(one, seed, 0, t)
    k = NS.knot_values(one, seed, 0, 0, np.arange(-2, 3))
    assert np.array_equal(s[::16], 65536 * k)
    for a in range(4):
        d = np.diff(s[16 * a:16 * a + 17])
        assert np.all(d >= 0) or np.all(d <= 0)
    # knots of different levels, rows and kinds of row are different draws
    m = np.arange(64)
    draws = [NS.knot_values(model, seed, r, j, m) for r, j in ((0, 0), (0, 1), (2, 0), (3, 0), (3, 1))]
    assert all(not np.array_equal(a, b) for i, a in enumerate(draws) for b in draws[i + 1:])


def test_level_autocov_enumeration():
    for s in (4, 6):
        N = 1 << s
        assert NS.level_autocov(s, 0) == pytest.approx(2.0 / 3.0 + 1.0 / (3.0 * 4.0 ** s), rel=1e-12)       # the variance quoted in noise_model.py
        assert NS.level_autocov(s, 2 * N - 1) == 0.0 and NS.level_autocov(s, 2 * N - 2) > 0.0       # (f = 1 and f = N - 1 share one knot, with weight 1 / N each)
        assert NS.level_autocov(s, -3) == NS.level_autocov(s, 3)
        assert slow_level_variance(0.5, s, 4.0) == pytest.approx(0.25 * 4.0 * NS.level_autocov(s, 0), rel=1e-12)


# ---------------------------------------------------------------------------------------------------- statistics
STAT_SEED = 20261020
STAT_N = 1 << 20
STAT_T0 = 987654321


def _within(name, got, exp, B, n=STAT_N):
    sd = np.sqrt(B / n)
    print(f'{name}: sample {got:+.5f} predicted {exp:+.5f} deviation {(got - exp) / sd:+.2f} sd (bound 5)')
    assert abs(got - exp) <= 5.0 * sd, (name, got, exp, sd)


def _variance_within(name, x, cov, span):
    """the sample variance of a series with the predicted autocovariance cov (zero beyond span): its own variance is 2 sum_v cov(v)^2 / n
    for a Gaussian series"""
    sd = np.sqrt(2.0 * sum(cov(v) ** 2 for v in range(-span, span + 1)) / len(x))
    print(f'{name}: sample variance {np.var(x):.4f} predicted {cov(0):.4f} deviation {(np.var(x) - cov(0)) / sd:+.2f} sd (bound 5)')
    assert abs(np.var(x) - cov(0)) <= 5.0 * sd, (name, np.var(x), cov(0), sd)


@pytest.mark.parametrize('shift', [4, 6])
def test_autocorrelation_of_one_level(shift):
    """S(r, t) of a single level: the sample autocorrelation follows the enumeration at lags inside, at and beyond the knot spacing"""
    N = 1 << shift
    pmf, vmin = gaussian_pmf([2.2])
    model = NS.slow_model(pmf, vmin, None, dict(shifts=[shift], slow_q=[[65536]]))
    x = NS.slow_values(model, STAT_SEED, 0, STAT_T0 + np.arange(STAT_N, dtype=np.int64)) / 65536.0
    var = NS.pmf_variance(pmf[0], vmin)
    assert var * NS.level_autocov(shift, 0) == pytest.approx(slow_level_variance(1.0, shift, var), rel=1e-12)
    _variance_within(f's = {shift} variance', x, lambda v: var * NS.level_autocov(shift, v), 2 * N)
    r = lambda v: NS.level_autocov(shift, v) / NS.level_autocov(shift, 0)
    for lag in (1, N // 2, N, 2 * N - 1, 2 * N + 3):
        B = NC.bartlett_factor(r, r, r, lag, n_lags=4 * N)
        _within(f's = {shift} lag {lag}', NC.sample_autocorr(x, lag), r(lag), B)
    assert r(2 * N + 3) == 0.0 and r(2 * N - 1) == 0.0 and r(N) > 0.1


def test_common_slow_level_correlates_channels():
    """two channels of one group with gains of opposite sign share the group's slow level: anticorrelated as predicted; a channel of another
    group is not correlated with either.

    Rounding: the own part of a channel is an integer here, so the fractions of a and b are those of +g X and -g X of the one common value
    X and their rounding errors are each other's negative: -1/12 in the covariance of a and b (less at ties), 1/12 in each variance.  A
    rounding error also correlates with the value it rounds when that value lives on a coarse lattice (on a knot X is an integer and g X a
    multiple of 1/2): with sigma 2 that moved the variances by 0.7 %, five standard deviations of this test.  sigma 20 makes every
    distribution wide against that lattice -- the fraction is independent of the magnitude -- and all of rounding 2e-4 of the variance."""
    groups = np.array([0, 0, 1])
    g = 0.5
    cfg = {'gains': [1.0] * 3, 'noise_model': {'sigma': [20.0, 20.0, 20.0], 'slow': dict(shifts=[4], amplitude=[0.0]),
                                               'common': dict(groups=groups, gain=[g, -g, g], sigma=20.0, slow=[1.0])}}
    model = _model(cfg)
    pmf, vmin = noise_pmf(cfg, 801)
    vw, vc = NS.pmf_variance(pmf[0], vmin), NS.pmf_variance(noise_colour(cfg, 801)['common_pmf'][0], vmin)
    t = STAT_T0 + np.arange(STAT_N, dtype=np.int64)
    a, b, c = (NS.slow_noise_values(model, STAT_SEED, ch, t) for ch in range(3))
    # covariance functions: own white + rounding at lag 0; the common stream's white at lag 0 and its level over 2 N lags
    common = lambda v: g * g * vc * ((1.0 if v == 0 else 0.0) + NS.level_autocov(4, v))
    total = vw + 1.0 / 12.0 + common(0)
    rxx = lambda v: ((vw + 1.0 / 12.0 if v == 0 else 0.0) + common(v)) / total
    rxy = lambda v: -(common(v) + (1.0 / 12.0 if v == 0 else 0.0)) / total
    zero = lambda v: 0.0
    for name, x in (('a', a), ('b', b), ('c', c)):
        _variance_within(f'variance of {name}', x, lambda v: total * rxx(v), 32)
    _within('corr(a, b)', NC.sample_corr(a, b), rxy(0), NC.bartlett_factor(rxx, rxx, rxy, 0, n_lags=64))
    _within('corr(a, c)', NC.sample_corr(a, c), 0.0, NC.bartlett_factor(rxx, rxx, zero, 0, n_lags=64))
    _within('corr(b, c)', NC.sample_corr(b, c), 0.0, NC.bartlett_factor(rxx, rxx, zero, 0, n_lags=64))
    assert rxy(0) < -0.25


def test_slow_levels_helper():
    sl = slow_levels(1e4, 1e6, 1.5, 2.2)
    assert sl['shifts'] == [6, 7, 8, 9, 10, 11, 12] and len(set(sl['amplitude'])) == 1          # 1 / (2 * 10 ns * 2^6) = 781 kHz .. 2^12: 12.2 kHz
    assert slow_levels(1e6, 4e6, 1.0, 2.0)['shifts'] == [4, 5]                                   # 3.1 MHz and 1.6 MHz
    with pytest.raises(ValueError, match='0 octaves between'):
        slow_levels(4e6, 1e7, 1.0, 2.0)
    with pytest.raises(ValueError, match='9 octaves between'):
        slow_levels(1e4, 3.2e6, 1.0, 2.0)
    with pytest.raises(ValueError, match='needs 0 < f_lo_hz <= f_hi_hz'):
        slow_levels(1e6, 1e4, 1.0, 2.0)
    with pytest.raises(ValueError, match='needs 0 < f_lo_hz <= f_hi_hz'):
        slow_levels(1e4, 1e6, 1.0, 0.0)
    # the stated rms, on the restatement: three levels, S alone
    sl = slow_levels(1.9e5, 1e6, 1.5, 2.2)
    assert sl['shifts'] == [6, 7, 8]
    cfg = {'gains': [1.0], 'noise_model': {'sigma': 2.2, 'slow': sl}}
    model = _model(cfg)
    x = NS.slow_values(model, STAT_SEED, 0, STAT_T0 + np.arange(STAT_N, dtype=np.int64)) / 65536.0
    pmf, vmin = noise_pmf(cfg, 801)
    var = NS.pmf_variance(pmf[0], vmin)
    assert var == pytest.approx(2.2 ** 2 + 1.0 / 12.0, rel=1e-3)                                 # Sheppard: what the helper assumes
    a = sl['amplitude'][0]
    cov = lambda v: sum(a * a * var * NS.level_autocov(s, v) for s in sl['shifts'])
    assert cov(0) == pytest.approx(1.5 ** 2, rel=1e-3)
    _variance_within('slow_levels rms', x, cov, 512)
