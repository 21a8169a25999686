"""RawDataOptical on runs of the reference (golden chains J: tests/golden/chain_optical.npz, chain_optical_cutoff.npz).

The fixtures hold what the reference's RawDataOptical (rawdata.py:461-495) did with ~200 / 40 optical instructions on the 120-channel
nVeto configuration: the photon list on entry to every Pulse.__call__ (what sim_primary itself decides: the _first:_last slices, the
[0, nveto_time_max_cutoff) window, the channel sort, timings + event time, one call per run set) and, downstream of the reference's
own random draws, pulses, digitise windows, rows, ZLE tuples and truth.  CPU only: the oracle's optical scheduler against the
former (EQUAL), the injected-photon replay against the latter (bit-exact, as for the other chains).
"""
import numpy as np
import pytest

from tests.helpers import (OPTICAL_CHAINS, golden, make_oracle, optical_chain_config,
                           photons_by_call_and_channel, replay_chain_on_oracle, with_fma)

CASES = sorted(OPTICAL_CHAINS)


def test_fixture_holds_the_cases_it_is_for():
    """the edges the chains exist for are in the stored inputs (a regenerated fixture that lost one fails here, not silently)"""
    d = golden(OPTICAL_CHAINS['main'])
    ins, t, ch, cutoff = d['instructions'], d['timings'], d['channels'], int(d['cutoff'])
    cfg = optical_chain_config('main')
    assert 'nveto_time_max_cutoff' not in cfg and cutoff == int(1e6) and cfg['gains'][7] == 0 and len(cfg['gains']) == 120
    assert len(ins) == 200 and len(d['dg_left']) > 20 and len(d['call_kind']) == len(ins)
    nph = ins['_last'] - ins['_first']
    order = np.argsort(ins['time'], kind='stable')
    new_cluster = np.concatenate([[True], np.diff(ins['time'][order]) > cfg['right_raw_extension']])
    empty = nph[order] == 0
    assert empty.sum() >= 3 and empty[-1] and (empty & new_cluster).any() and nph.max() == 8
    assert (np.diff(np.flatnonzero(new_cluster)) > 1).any() and new_cluster.sum() > 30      # clusters of several instructions
    assert (np.diff(ins['time'][order]) == 0).sum() == 1
    assert {0, cutoff - 1, cutoff}.issubset(set(t.tolist())) and (t < 0).sum() >= 3 and (t >= cutoff).sum() >= 3
    assert (ch == 7).sum() >= 3 and ((ch == 7) & (t >= 0) & (t < cutoff)).any()
    kept = (t >= 0) & (t < cutoff)
    all_cut = [not kept[a:b].any() for a, b in zip(ins['_first'], ins['_last']) if b > a]
    assert any(all_cut)
    c = golden(OPTICAL_CHAINS['cutoff'])
    assert int(c['cutoff']) == optical_chain_config('cutoff')['nveto_time_max_cutoff'] == 5000
    tc = c['timings']
    assert ((tc >= 0) & (tc < 5000)).sum() > 30 and (tc >= 5000).sum() > 30 and {4999, 5000}.issubset(set(tc.tolist()))


@pytest.mark.parametrize('case', CASES)
def test_sim_primary_photon_lists_equal_the_reference(case):
    """orc.simulate_optical on the stored inputs against the photon lists the reference's sim_primary handed to Pulse.__call__:
    number of calls, which instruction each call is (save_full_truth: one instruction per run set, in the reference's processing
    order), photons per call, and per call and channel the sorted entry times -- all EQUAL"""
    d = golden(OPTICAL_CHAINS[case])
    cfg = optical_chain_config(case)
    ins = d['instructions']
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), d['channels'], d['timings'], cfg.get('nveto_time_max_cutoff', int(1e6)))
    r = orc.results()
    assert len(r['call_kind']) == len(d['call_kind']) == len(ins)
    assert np.array_equal(r['call_ph_off'], d['call_in_off'])
    assert len(r['opt_in_t']) == len(d['in_t']) == r['call_ph_off'][-1]
    got = photons_by_call_and_channel(r['call_ph_off'], r['opt_in_t'], r['opt_in_ch'])
    want = photons_by_call_and_channel(d['call_in_off'], d['in_t'], d['in_ch'])
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'call {k}'
    # which instruction a call is: the reference writes one truth row per call, in call order, with the instruction's fields
    tr = d['truth']
    assert len(tr) == len(ins)
    proc = np.argsort(ins['time'], kind='stable')
    assert np.array_equal(tr['event_number'], ins['event_number'][proc])
    kept = (d['timings'] >= 0) & (d['timings'] < int(d['cutoff']))
    n_kept = np.array([kept[a:b].sum() for a, b in zip(ins['_first'][proc], ins['_last'][proc])])
    assert np.array_equal(np.diff(d['call_in_off']), n_kept)
    # the stored entry lists are channel sorted and nothing outside the window got through
    for a, b, i in zip(d['call_in_off'][:-1], d['call_in_off'][1:], proc):
        assert np.all(np.diff(d['in_ch'][a:b]) >= 0)
        rel = d['in_t'][a:b] - ins['time'][i]
        assert np.all((rel >= 0) & (rel < int(d['cutoff'])))
    # photons on the dead PMT enter the call (sim_primary does not know the gains) and leave no truth: n_photon counts live ones
    live = cfg['gains'][d['ph_ch']] > 0
    assert np.array_equal(tr['n_photon'], [live[a:b].sum() for a, b in zip(d['call_ph_off'][:-1], d['call_ph_off'][1:])])


@pytest.mark.parametrize('case', CASES)
def test_optical_chain_replay_bit_exact(case):
    """the reference's photons after its transit-time draw, with its gains, injected call by call (replay_chain_on_oracle) on the
    nVeto configuration: pulse list, digitise windows, rows, masks, ZLE tuples and all truth accumulators bit-exact; with fused
    multiply-adds rows and ZLE tuples equal"""
    d = golden(OPTICAL_CHAINS[case])
    cfg = optical_chain_config(case)
    for fma in (True, False):
        orc = make_oracle(with_fma(cfg, fma))
        r = replay_chain_on_oracle(orc, d)
        for a, b in [('pl_ch', 'pl_ch'), ('pl_left', 'pl_left'), ('pl_right', 'pl_right'), ('pl_nph', 'pl_photons'),
                     ('dg_left', 'dg_left'), ('dg_right', 'dg_right'), ('dg_row_off', 'dg_row_off'), ('row_ch', 'row_ch'),
                     ('row_left', 'row_left'), ('row_right', 'row_right'), ('row_data_off', 'row_data_off'), ('row_data', 'row_data')]:
            assert np.array_equal(r[a], d[b]), (a, fma)
        for k in ['ch', 'left', 'right', 'data_off', 'data', 'digit']:
            assert np.array_equal(r['zl_' + k], d['zle_' + k]), (k, fma)
    assert 7 not in d['pl_ch'] and len(d['pl_ch']) > 30
    tr = r['truth'].reshape(-1, 12)
    names = ['n_photon', 'n_pe', 'n_photon_trigger', 'n_pe_trigger', 'raw_area', 'raw_area_trigger']
    for j, f in enumerate(names):
        assert np.array_equal(tr[:, j], d['call_truth_' + f].astype(np.float64)), f
        assert np.array_equal(tr[:, 6 + j], d['call_truth_' + f + '_bottom'].astype(np.float64)), f + '_bottom'
    assert np.array_equal(tr[:, 0], d['truth']['n_photon'])
