"""The yardstick of PMT afterpulses behind supplied photons (tests/optical_afterpulse.py), pinned on the CPU: the numpy restatement
of the afterpulse call equals the oracle's own, the call-by-call driver equals the oracle's optical scheduler, and the fixture of the
reference's RawDataOptical with afterpulses on (tests/golden/chain_optical_ap.npz) replays on the oracle and has the structure the
driver assumes.  These pass without the device feature: they pin what the GPU tests (tests/test_gpu_optical_afterpulse.py) compare to."""
import numpy as np

from tests import optical_afterpulse as OA
from tests.helpers import ap_tables_from_golden, golden, make_oracle, replay_chain_on_oracle, with_fma
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.workloads import nveto_config, optical_instructions


def scaled_tables(factor, rows=None):
    """the golden afterpulse tables with every cumulative delay row (its last entry is the probability) times ``factor``; ``rows``: the
    first so many channels only"""
    out = {}
    for name, d in ap_tables_from_golden().items():
        dc, ac = d['delaytime_cdf'] * factor, d['amplitude_cdf']
        if rows is not None:
            dc, ac = dc[:rows], (ac[:rows] if ac.ndim == 2 else ac)
        out[name] = dict(d, delaytime_cdf=np.ascontiguousarray(dc), amplitude_cdf=np.ascontiguousarray(ac))
    return out


def test_restated_afterpulse_call_equals_the_oracles():
    """one tile-generated S2 (photon q of channel ch draws at counter (ch, gid, q, site)): afterpulses_of on the parents of the kind-2
    call gives the kind-3 call's photons exactly -- time, channel and gain, in order"""
    ap = scaled_tables(4)
    cfg = xenonnt_test_config(seed=77, enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap, pmt_ap_modifier=1.3, pmt_ap_t_modifier=3,
                              enable_electron_afterpulses=False)
    ins = np.zeros(1, dtype=instruction_dtype)
    ins['type'], ins['amp'], ins['z'], ins['recoil'], ins['time'] = 2, 2500, -5.0, 7, 1_000_000
    orc = make_oracle(cfg, ap)
    orc.simulate(ins, np.array([5], dtype=np.uint32), instruction_params(ins, cfg, Resource(cfg)))
    o = orc.results()
    assert o['call_kind'].tolist() == [2, 3]
    a, b, c = o['call_ph_off']
    ch = o['ph_ch'][a:b]
    assert np.all(np.diff(ch) >= 0)
    pos = np.arange(b - a) - np.searchsorted(ch, ch, side='left')           # position inside the channel
    p = kernel_params(cfg)
    t, c3, g = OA.afterpulses_of(p['seed'], ap, cfg['gains'], p['pmt_ap_modifier'], p['pmt_ap_t_modifier'],
                                 (o['ph_t'][a:b], ch, o['ph_dpe'][a:b], ch.astype(np.int64), np.full(b - a, 5), pos))
    print('parents', b - a, 'afterpulses', c - b, 'restated', len(t))
    assert b - a > 20000 and c - b > 4000
    assert np.array_equal(t, o['ph_t'][b:c]) and np.array_equal(c3, o['ph_ch'][b:c]) and np.array_equal(g, o['ph_gain'][b:c])


def test_driver_equals_the_oracles_optical_scheduler():
    """afterpulses off: the records of the driven oracle are simulate_optical's, byte for byte, and so are the windows"""
    cfg = nveto_config(seed=31)
    ins, channels, timings = optical_instructions(400, 1000.0, 3)
    ref = make_oracle(cfg)
    ref.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, int(1e6))
    orc, aps, order = OA.drive_optical(cfg, ins, channels, timings, int(1e6))
    assert all(x is None for x in aps) and np.array_equal(order, np.arange(len(ins)))
    o, r = orc.results(), ref.results()
    print('windows', len(r['dg_left']))
    assert len(r['dg_left']) > 10
    for f in ('dg_left', 'dg_right', 'dg_first_pulse', 'dg_n_pulses', 'pl_ch', 'pl_left', 'pl_right'):
        assert np.array_equal(o[f], r[f]), f
    assert orc.pack_records().tobytes() == ref.pack_records().tobytes()


# ------------------------------------------------------------------------------------------------ the reference's run
def optical_ap_chain_config(**overrides):
    """the config of tests/golden/chain_optical_ap.npz (make_golden_optical_ap.py: overrides): 494 channels, three turned-off PMTs,
    right_raw_extension 2 us, the golden afterpulse tables times ap_scale, modifier 1.3, t_modifier 3"""
    import json
    import os
    from tests.helpers import GOLDEN
    ov = json.load(open(os.path.join(GOLDEN, 'chain_optical_ap_config.json')))
    scale = ov.pop('ap_scale')
    ov['gains'] = np.asarray(ov['gains'], dtype=np.float64)
    ov['turned_off_pmts'] = np.asarray(ov['turned_off_pmts'])
    c = xenonnt_test_config(enable_pmt_afterpulses=True, uniform_to_pmt_ap=scaled_tables(scale), **ov)
    c.update(overrides)
    return c


def test_fixture_holds_the_cases_it_is_for():
    d = golden('chain_optical_ap.npz')
    ins, t, ch, cutoff = d['instructions'], d['timings'], d['channels'], int(d['cutoff'])
    cfg = optical_ap_chain_config()
    kept = (t >= 0) & (t < cutoff)
    nph = ins['_last'] - ins['_first']
    assert len(cfg['gains']) == 494 and len(ins) == 80 and nph.max() <= 40 and np.all(np.diff(ins['time']) >= 0)
    assert (nph == 0).any() and (np.diff(ins['time']) == 0).sum() == 1
    assert any(b > a and not kept[a:b].any() for a, b in zip(ins['_first'], ins['_last']))
    assert (kept & (cfg['gains'][ch] == 0)).sum() >= 3 and (t[kept] > 1500).sum() >= 3
    assert (d['call_kind'] == 3).sum() > 50 and np.diff(d['call_ph_off'])[d['call_kind'] == 3].sum() > 200


def test_fixture_replays_on_the_oracle_and_has_the_drivers_structure():
    d = golden('chain_optical_ap.npz')
    cfg = optical_ap_chain_config()
    # ---- injected-photon replay: windows, rows, ZLE tuples, integer truth (the comparison of tests/test_optical_chain_reference.py)
    for fma in (True, False):
        orc = make_oracle(with_fma(cfg, fma))
        r = replay_chain_on_oracle(orc, d)
        for a, b in [('pl_ch', 'pl_ch'), ('pl_left', 'pl_left'), ('pl_right', 'pl_right'), ('pl_nph', 'pl_photons'),
                     ('dg_left', 'dg_left'), ('dg_right', 'dg_right'), ('dg_row_off', 'dg_row_off'), ('row_ch', 'row_ch'),
                     ('row_left', 'row_left'), ('row_right', 'row_right'), ('row_data_off', 'row_data_off'), ('row_data', 'row_data')]:
            assert np.array_equal(r[a], d[b]), (a, fma)
        for k in ['ch', 'left', 'right', 'data_off', 'data', 'digit']:
            assert np.array_equal(r['zl_' + k], d['zle_' + k]), (k, fma)
    tr = r['truth'].reshape(-1, 12)
    for j, f in enumerate(['n_photon', 'n_pe', 'n_photon_trigger', 'n_pe_trigger']):
        assert np.array_equal(tr[:, j], d['call_truth_' + f].astype(np.float64)), f
        assert np.array_equal(tr[:, 6 + j], d['call_truth_' + f + '_bottom'].astype(np.float64)), f + '_bottom'
    # ---- structure: one afterpulse call (kind 3, channels sorted) right behind every primary call that holds a photon, in the same
    # window; none behind a primary call without photons; one truth row per instruction
    kind, nph, npl = d['call_kind'], np.diff(d['call_ph_off']), np.diff(d['call_pulse_off'])
    assert set(kind.tolist()) == {0, 3} and (kind == 0).sum() == len(d['instructions']) == len(d['truth'])
    win_of_pulse = np.repeat(np.arange(len(d['dg_left'])), d['dg_n_pulses'])
    assert np.array_equal(d['dg_first_pulse'], np.cumsum(d['dg_n_pulses']) - d['dg_n_pulses'])

    def window(k):
        p = d['call_pulse_off'][k]
        return int(win_of_pulse[p]) if npl[k] else None
    for k in np.flatnonzero(kind == 0):
        follows = k + 1 < len(kind) and kind[k + 1] == 3
        assert follows == (nph[k] > 0), k
        if follows:
            a, b = d['call_ph_off'][k + 1], d['call_ph_off'][k + 2]
            assert np.all(np.diff(d['ph_ch'][a:b]) >= 0) and d['call_has_gains'][k + 1]
            assert not (k + 2 < len(kind) and kind[k + 2] == 3)
            if npl[k] and npl[k + 1]:
                assert window(k) == window(k + 1), k
    # ---- the driver's window rule on the recorded calls, in place of dg_first_pulse
    ins = d['instructions']
    proc = np.argsort(ins['time'], kind='stable')
    orc = make_oracle(cfg)
    rule = OA.WindowRule(orc, cfg['right_raw_extension'], cfg['sample_duration'])
    q = -1
    for k in range(len(kind)):
        if kind[k] == 0:
            q += 1
            rule.before_instruction(int(ins['time'][proc[q]]))
        a, b = d['call_ph_off'][k], d['call_ph_off'][k + 1]
        orc.pulse_call(int(kind[k]), q, d['ph_t'][a:b], d['ph_ch'][a:b], d['ph_dpe'][a:b], d['ph_gain'][a:b], bool(d['call_has_gains'][k]))
    orc.digitize_and_zle(0)
    assert np.array_equal(orc.get('dg_left'), d['dg_left']) and np.array_equal(orc.get('dg_right'), d['dg_right'])
    assert len(d['dg_left']) > 5
