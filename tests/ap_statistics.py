"""Statistics shared by the CPU and GPU tests of the PMT-afterpulse generator against draws of the reference's
PMT_Afterpulse.photon_afterpulse (tests/golden/pmt_ap_draws.npz, made by make_golden.py pmt_ap_draws).

Both sides are reduced to COUNTS (`ap_counts`): parents per channel (single / double PE), afterpulses per channel, histograms over
the delay bin and the amplitude bin, for He the joint table.  `compare` gives one p-value per table (two-sample chi-square on the
2 x K contingency table; columns with fewer than 20 pooled entries are merged into their neighbour, never dropped) and z-scores
for the total rate and the mean delay bin.  ACCEPT: every p > P_MIN = 1e-3 and every |z| < Z_MAX = 4: with some 50 figures over
all cases a correct generator fails by chance less than once in twenty re-seedings, while the wrong laws of the power check
(tests/test_pmt_afterpulse_cpu.py) land many orders of magnitude beyond.  The thresholds are conditions, not measurements."""
import numpy as np
from scipy.stats import chi2

from tests.helpers import golden
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype

P_MIN, Z_MAX = 1e-3, 4.0
N_CH = 494
ELEMENTS = ('He', 'Xe', 'Uniform')


def scaled_tables(name, only=True):
    """pmt_ap_tables.npz with the probability column of element `name` ('He', 'Xe', 'Uniform', 'Uniform_hi') scaled as in the
    draw fixture (the factors are stored there); the other elements switched off (probability 0) -- or, only=False, all three
    elements scaled (the fixture's all-elements case)"""
    tab, fx = golden('pmt_ap_tables.npz'), golden('pmt_ap_draws.npz')
    out = {}
    for el in ELEMENTS:
        key = name if (only and name.split('_')[0] == el) else el
        on = (not only) or name.split('_')[0] == el
        out[el] = dict(delaytime_cdf=tab[f'{el}_delaytime_cdf'] * (float(fx[f'scale_{key}']) if on else 0.0),
                       amplitude_cdf=tab[f'{el}_amplitude_cdf'], delaytime_bin_size=float(tab[f'{el}_delaytime_bin_size']),
                       amplitude_bin_size=float(tab[f'{el}_amplitude_bin_size']))
    return out


def fixture_counts(case):
    fx = golden('pmt_ap_draws.npz')
    return {k[len(case) + 1:]: fx[k] for k in fx.files if k.startswith(case + '_')}


def ap_counts(element, par_ch, par_dpe, ap_ch, delay_bin=None, amp_bin=None):
    """counts of one sample.  delay_bin: index of the delay bin (Uniform: delay in whole ns); amp_bin: index of the amplitude bin"""
    par_dpe = np.asarray(par_dpe).astype(bool)
    c = dict(par_single=np.bincount(par_ch[~par_dpe], minlength=N_CH), par_double=np.bincount(par_ch[par_dpe], minlength=N_CH),
             ap_ch=np.bincount(ap_ch, minlength=N_CH))
    uni = element.startswith('Uniform')
    if delay_bin is not None:
        assert delay_bin.min() >= 0 and delay_bin.max() < (512 if uni else 200), (delay_bin.min(), delay_bin.max())
        c['delay'] = np.bincount(delay_bin, minlength=512 if uni else 200)
    if amp_bin is not None:
        assert amp_bin.min() >= 0 and amp_bin.max() < (4 if uni else 100)
        c['amp'] = np.bincount(amp_bin, minlength=4 if uni else 100)
    if element == 'He' and delay_bin is not None and amp_bin is not None:
        c['joint'] = np.zeros((20, 20), np.int64)
        np.add.at(c['joint'], (delay_bin // 10, amp_bin // 5), 1)
    return c


def _merge_sparse(a, b, least=20):
    """merge every column whose pooled count is below `least` into its right neighbour (the last one into its left): the mass stays"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    oa, ob = [], []
    ca = cb = 0
    for x, y in zip(a, b):
        ca += x; cb += y
        if ca + cb >= least:
            oa.append(ca); ob.append(cb); ca = cb = 0
    if ca + cb > 0:
        if oa:
            oa[-1] += ca; ob[-1] += cb
        else:
            oa.append(ca); ob.append(cb)
    return np.array(oa, float), np.array(ob, float)


def two_sample_chi2(a, b):
    """p-value of the 2 x K contingency table of two count vectors (same law?), sparse columns merged"""
    assert np.sum(a) > 0 and np.sum(b) > 0
    a, b = np.ravel(a), np.ravel(b)
    n = max(len(a), len(b))
    a, b = _merge_sparse(np.pad(a, (0, n - len(a))), np.pad(b, (0, n - len(b))))
    if len(a) < 2:
        return 1.0
    na, nb = a.sum(), b.sum()
    ea, eb = (a + b) * na / (na + nb), (a + b) * nb / (na + nb)
    stat = ((a - ea) ** 2 / ea).sum() + ((b - eb) ** 2 / eb).sum()
    return float(chi2.sf(stat, len(a) - 1))


def rate_tests(x, y, n_elements=1):
    """afterpulses per channel relative to the parents' weight w = singles + 2 * doubles (afterpulse.py:200-204; the samples have
    different parents, so rates are compared).  With the pooled rate per unit weight r = (a_x + a_y) / (w_x + w_y) of a channel, the
    residual a_x - w_x r has variance (w_y^2 V_x + w_x^2 V_y) / (w_x + w_y)^2, V = singles r (1 - r) + doubles q (1 - q), q = min(2 r, 1):
    binomial counts, not Poisson ones -- at P * modifier ~ 0.3 the Poisson variance would be a third too large and hide a rate error.
    n_elements > 1 (several elements in one call: a parent makes a sum of n_elements Bernoulli afterpulses of total mean r): the variance per
    parent is r - sum p_e^2 <= r (1 - r / n_elements), the bound is used (conservative).
    Returns (p of the chi-square over the channels, z of the summed residual = the total rate).  Where a double-PE parent saturates
    (P * modifier * 2 > 1) the weight is not exact, but both samples have the same double-PE fraction and only the ratio enters."""
    wx, wy = x['par_single'] + 2.0 * x['par_double'], y['par_single'] + 2.0 * y['par_double']
    assert wx.min() > 0 and wy.min() > 0
    n = (x['ap_ch'] + y['ap_ch']).astype(float)
    r = n / (wx + wy)
    n_el = float(n_elements)
    q = np.minimum(2 * r, n_el)
    vx = x['par_single'] * r * (1 - r / n_el) + x['par_double'] * q * (1 - q / n_el)
    vy = y['par_single'] * r * (1 - r / n_el) + y['par_double'] * q * (1 - q / n_el)
    resid, var = x['ap_ch'] - wx * r, (wy ** 2 * vx + wx ** 2 * vy) / (wx + wy) ** 2
    # channels with few pooled afterpulses are merged with their neighbour
    g_res, g_var, rs, vs, m = [], [], 0.0, 0.0, 0.0
    for c in range(len(n)):
        rs += resid[c]; vs += var[c]; m += n[c]
        if m >= 20:
            g_res.append(rs); g_var.append(vs); rs = vs = m = 0.0
    if m > 0 and g_res:
        g_res[-1] += rs; g_var[-1] += vs
    g_res, g_var = np.array(g_res), np.array(g_var)
    return float(chi2.sf((g_res ** 2 / g_var).sum(), len(g_res))), float(resid.sum() / np.sqrt(var.sum()))


def mean_z(a, b):
    """z of the difference of the mean bin index of two histograms"""
    n = max(len(a), len(b))
    a, b = np.pad(a, (0, n - len(a))).astype(float), np.pad(b, (0, n - len(b))).astype(float)
    k = np.arange(n, dtype=float)
    na, nb = a.sum(), b.sum()
    ma, mb = (a * k).sum() / na, (b * k).sum() / nb
    va, vb = (a * (k - ma) ** 2).sum() / na, (b * (k - mb) ** 2).sum() / nb
    return float((ma - mb) / np.sqrt(va / na + vb / nb))


def blur(hist, f, seed):
    """every entry of a histogram moved up one bin with probability f (seeded): what parents that sit on two adjacent nanoseconds,
    a fraction f on the later one, do to a delay measured from the earlier one"""
    up = np.random.default_rng(seed).binomial(np.asarray(hist, np.int64), f)
    out = np.zeros(len(hist) + 1, np.int64)
    out[:-1] += hist - up
    out[1:] += up
    return out


def compare(x, fx, tables=('delay', 'amp', 'joint', 'rate'), late_fraction=None):
    """x: counts of the sample under test, fx: the fixture's.  dict of p-values ('p_*') and z-scores ('z_*').  late_fraction: the
    delay histogram of x is in whole ns measured from the earlier of two adjacent parent times (Uniform element), the fixture's is
    blurred accordingly"""
    out = {}
    if 'rate' in tables:
        out['p_rate'], out['z_total'] = rate_tests(x, fx)
    if 'delay' in tables and 'delay' in x:
        ref = fx['delay'] if late_fraction is None else blur(fx['delay'], late_fraction, 7)
        out['p_delay'] = two_sample_chi2(x['delay'], ref)
        out['z_mean_delay'] = mean_z(x['delay'], ref)
    if 'amp' in tables and 'amp' in x and len(x['amp']) > 4:          # (Uniform: the amplitude is 1, checked exactly by the callers)
        out['p_amp'] = two_sample_chi2(x['amp'], fx['amp'])
    if 'joint' in tables and 'joint' in x:
        out['p_joint'] = two_sample_chi2(x['joint'], fx['joint'])
    return out


def accepted(res):
    return all((v > P_MIN) if k.startswith('p_') else (abs(v) < Z_MAX) for k, v in res.items())


def fmt(res):
    return ' '.join(f'{k}={v:.3g}' for k, v in sorted(res.items()))


def photon_counts(element, tables, gains, t_modifier, par_t, par_ch, par_dpe, ap_t, ap_ch, ap_gain, period=1_000_000, exact_delays=True):
    """counts of a simulated sample: parents and afterpulses of instructions `period` ns apart (times relative to the instruction =
    t - period * round(t / period)).  exact_delays: the parents must sit on two adjacent nanoseconds t0, t0 + 1 (asserted) -- then
    the delay BIN of an afterpulse at 10 k - t_modifier (+0 / +1) behind t0 is k, exactly; for the Uniform element the delay in whole
    ns measured from t0 (returned with the fraction of parents on t0 + 1, for `compare`).  Without: no delay histogram."""
    el = element.split('_')[0]
    T = tables[el]
    rel = lambda t: np.asarray(t, np.int64) - period * np.rint(np.asarray(t, np.float64) / period).astype(np.int64)
    abin = np.rint(ap_gain / np.asarray(gains)[ap_ch] / T['amplitude_bin_size']).astype(np.int64)
    assert np.allclose(abin * T['amplitude_bin_size'] * np.asarray(gains)[ap_ch], ap_gain, rtol=1e-9)          # amplitudes sit on the table's bins
    if not exact_delays:
        return ap_counts(element, par_ch, par_dpe, ap_ch, None, abin), None
    rp, ra = rel(par_t), rel(ap_t)
    t0 = int(rp.min())
    assert rp.max() - t0 <= 1, f'parents spread over {t0} .. {int(rp.max())} ns: the delay bins would blur'
    late = float(np.mean(rp == t0 + 1))
    if el == 'Uniform':
        return ap_counts(element, par_ch, par_dpe, ap_ch, ra - t0, abin), late
    d = ra - t0 + int(t_modifier)
    step = int(T['delaytime_bin_size'])
    assert step == T['delaytime_bin_size'] and np.all(d % step <= 1), 'afterpulse times off the delay grid'
    return ap_counts(element, par_ch, par_dpe, ap_ch, d // step, abin), None


# ------------------------------------------------------------------------------------------------ inputs of the simulated samples
MS = 1_000_000
DRAW_CASES = [(el, m) for el in ELEMENTS for m in (0.6, 1.0, 1.8)] + [('Uniform_hi', 1.8)]
MIN_AFTERPULSES = 200_000


def case_name(element, modifier):
    return f'{element}_m{int(round(modifier * 10)):02d}'


def draw_config(modifier, seed, **kw):
    """the config of the afterpulse-draw tests: S1 photons without spread (every parent photon 45 or 46 ns behind its instruction),
    the fixture's pmt_ap_t_modifier and non-uniform gains"""
    fx = golden('pmt_ap_draws.npz')
    return xenonnt_test_config(seed=seed, pmt_ap_modifier=modifier, pmt_ap_t_modifier=int(fx['t_modifier']), gains=fx['gains'],
                               s1_model_type='simple', s1_decay_time=1e-9, s1_decay_spread=0.0, pmt_transit_time_spread=1e-9, **kw)


def s1_instructions_for(element, modifier, cfg, amp=600_000, detected=0.095):
    """enough S1s of `amp` photons for MIN_AFTERPULSES afterpulses: per parent the tables promise mean(P) * modifier * (1 + p_dpe)
    of them (singles P * modifier, doubles twice that, both capped at 1), and about `detected` of the photons of a test-config S1
    become parents; 10 % margin"""
    P = scaled_tables(element)[element.split('_')[0]]['delaytime_cdf'][:, -1]
    p_dpe = cfg['p_double_pe_emision']
    per_parent = np.mean((1 - p_dpe) * np.minimum(P * modifier, 1) + p_dpe * np.minimum(2 * P * modifier, 1))
    n = int(np.ceil(1.1 * MIN_AFTERPULSES / (per_parent * amp * detected)))
    ins = np.zeros(n, dtype=instruction_dtype)
    ins['type'], ins['amp'], ins['z'], ins['recoil'] = 1, amp, -30.0, 7
    ins['time'], ins['event_number'] = MS * (1 + np.arange(n)), np.arange(n)
    return ins


def afterpulses_per_parent(element, modifier, p_dpe):
    P = scaled_tables(element)[element.split('_')[0]]['delaytime_cdf'][:, -1]
    return float(np.mean((1 - p_dpe) * np.minimum(P * modifier, 1) + p_dpe * np.minimum(2 * P * modifier, 1)))


def s2_instructions_for(element, modifier, cfg, amp=4000, photons=285_000):
    """S2s of `amp` electrons at z = -10 cm (s2_secondary_sc_gain 100: about `photons` parents each), enough for MIN_AFTERPULSES"""
    n = int(np.ceil(1.15 * MIN_AFTERPULSES / (afterpulses_per_parent(element, modifier, cfg['p_double_pe_emision']) * photons)))
    ins = np.zeros(n, dtype=instruction_dtype)
    ins['type'], ins['amp'], ins['z'], ins['recoil'] = 2, amp, -10.0, 7
    ins['time'], ins['event_number'] = MS * (1 + np.arange(n)), np.arange(n)
    return ins


# ------------------------------------------------------------------------------------------------ numpy draws (power check)
def numpy_draws(element, tables, modifier, p_dpe, n_parents, seed, law='reference'):
    """afterpulses of `n_parents` parents on uniformly drawn channels, in numpy, under the law of afterpulse.py:172-249 ('reference': the
    parent fires when rU0 / modifier (/ 2 for a double-PE parent) <= P(channel); delay = the bin of the unnormalised delay cdf nearest
    to that scaled uniform; amplitude = the bin of the amplitude cdf nearest to an independent rU1) or under a plausible wrong one:
      'first_above' : the delay bin is the first bin whose cdf is >= u (searchsorted) instead of the nearest bin
      'no_dpe'      : the uniform of a double-PE parent is not halved
      'one_uniform' : the amplitude is looked up with the (normalised) delay uniform instead of an independent one
    returns counts (ap_counts)"""
    el = element.split('_')[0]
    T = tables[el]
    rng = np.random.default_rng(seed)
    ch = rng.integers(0, N_CH, n_parents)
    dpe = rng.random(n_parents) < p_dpe
    u0 = (1 - rng.random(n_parents)) / modifier
    if law != 'no_dpe':
        u0[dpe] /= 2
    dc = T['delaytime_cdf']
    sel = np.flatnonzero(u0 <= dc[ch, -1])
    sch, su0 = ch[sel], u0[sel]
    u1 = 1 - rng.random(len(sel))
    if law == 'one_uniform':
        u1 = su0 / dc[sch, -1]
    if el == 'Uniform':
        delay = np.floor(rng.uniform(dc[sch, 0], dc[sch, 1]) * T['delaytime_bin_size']).astype(np.int64)
        return ap_counts(element, ch, dpe, sch, delay, np.ones(len(sel), np.int64))
    dbin, abin = np.zeros(len(sel), np.int64), np.zeros(len(sel), np.int64)
    ac = T['amplitude_cdf']
    for a in range(0, len(sel), 100_000):
        s = slice(a, a + 100_000)
        rows = dc[sch[s]]
        if law == 'first_above':
            dbin[s] = np.minimum((rows < su0[s][:, None]).sum(axis=1), rows.shape[1] - 1)
        else:
            dbin[s] = np.argmin(np.abs(rows - su0[s][:, None]), axis=-1)
        arows = ac[sch[s]] if ac.ndim == 2 else ac[None, :]
        abin[s] = np.argmin(np.abs(arows - u1[s][:, None]), axis=-1)
    return ap_counts(element, ch, dpe, sch, dbin, abin)
