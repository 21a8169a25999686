"""Optical-input path (RawDataOptical / nVeto, BASELINE config[4] shape) on the GPU against the CPU oracle."""
import numpy as np
import pytest

import wfsim_amd
from tests.helpers import (OPTICAL_CHAINS, assert_tiles_in_oracle_order, golden, make_engine, make_oracle, optical_chain_config, photons_by_call_and_channel)
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype, truth_extra_dtype

pytestmark = pytest.mark.gpu


from wfsim_amd.workloads import nveto_config, optical_instructions      # noqa: E402  (the builders of BASELINE configs[4])


def test_nveto_high_rate_against_oracle():
    cfg = nveto_config(seed=31)
    ins, channels, timings = optical_instructions(3000, 1000.0, 3)       # ~1 MHz instruction rate
    keep = channels != 7                                                  # photons on the dead PMT make no pulse (pulse.py:89)
    rd = wfsim_amd.RawDataOptical(cfg, channels=channels, timings=timings)
    windows = list(rd.iter_windows(ins))
    rec = np.concatenate([w['records'] for w in windows])
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, int(1e6))
    o = orc.results()
    assert len(windows) == len(o['dg_left'])
    assert np.array_equal([w['left'] for w in windows], o['dg_left'])
    assert np.array_equal([w['right'] for w in windows], o['dg_right'])
    assert rec.tobytes() == orc.pack_records().tobytes()
    assert len(rec) > 1000 and rec['channel'].max() < 120 and 7 not in rec['channel']


def test_nveto_chunker_output():
    cfg = nveto_config(seed=32, chunk_size=0.0005)
    ins, channels, timings = optical_instructions(2000, 1000.0, 4)
    sim = wfsim_amd.ChunkRawRecords(cfg, rawdata_generator=wfsim_amd.RawDataOptical, channels=channels, timings=timings)
    sim.truth_buffer = np.zeros(10000, dtype=instruction_dtype + optical_extra_dtype + sim.truth_dtype + [('fill', bool)])
    chunks = list(sim(ins))
    assert len(chunks) >= 3 and set(chunks[0].keys()) == {'raw_records', 'truth'}
    rr = np.concatenate([c['raw_records'] for c in chunks])
    truth = np.concatenate([c['truth'] for c in chunks])
    # the chunks are instruction_dtype + truth fields (strax_interface.py:478), without the buffer's _first / _last columns
    assert len(truth) == len(ins) and truth.dtype == np.dtype(instruction_dtype + sim.truth_dtype)
    assert np.all(np.diff(rr['time']) >= 0) and rr['data'].sum() > 0
    ok = (timings >= 0) & (timings < 1e6) & (channels != 7)
    assert truth['n_photon'].sum() == ok.sum()


def test_nveto_plugin():
    from wfsim_amd import ministrax
    ins, channels, timings = optical_instructions(1500, 1000.0, 5)
    cfg = nveto_config(seed=33, chunk_size=0.0005, instructions=ins, channels=channels, timings=timings)
    plugin = wfsim_amd.RawRecordsFromFaxnVeto(cfg)
    out = ministrax.run_plugin(plugin)
    rr = np.concatenate([c.data for c in out['raw_records_nv']])
    truth = np.concatenate([c.data for c in out['truth_nv']])
    assert len(out['raw_records_nv']) >= 2 and len(rr) > 500
    assert rr['channel'].min() >= 2000 and rr['channel'].max() <= 2119
    assert len(truth) == len(ins) and np.all(np.diff(rr['time']) >= 0)


def test_mc_chain_plugin_tpc_and_nveto():
    """RawRecordsFromMcChain (strax_interface.py:753-1005) with supplied instructions: both detectors follow the same
    event times; chunks of all six data types share the plugin's chunk boundaries"""
    from wfsim_amd import ministrax
    from wfsim_amd.dtypes import instruction_dtype
    n_ev = 40
    rng = np.random.default_rng(8)
    tpc = np.zeros(2 * n_ev, dtype=instruction_dtype)
    tpc['g4id'] = np.repeat(np.arange(n_ev), 2)
    tpc['type'] = np.tile([1, 2], n_ev)
    tpc['amp'] = np.tile([800, 40], n_ev)
    tpc['z'], tpc['recoil'] = -rng.uniform(1, 90, 2 * n_ev), 7
    tpc['time'] = np.tile([0, 200], n_ev)
    tpc['event_number'] = tpc['g4id']
    nv, channels, timings = optical_instructions(n_ev, 1000.0, 6)
    nv['time'], nv['g4id'] = 0, np.arange(n_ev)
    ncfg = nveto_config()
    nveto_keys = {k: ncfg[k] for k in ('gains', 'n_tpc_pmts', 'n_top_pmts', 'channel_map', 'photon_area_distribution', 'right_raw_extension')}
    cfg = xenonnt_test_config(seed=4, chunk_size=0.01, event_rate=1000.0, targets=('tpc', 'nveto'), instructions_epix=tpc,
                              instructions_nveto=nv, nveto_channels=channels, nveto_timings=timings, fax_config_nveto=nveto_keys)
    cfg['channel_map'] = dict(cfg['channel_map'], nveto=(2000, 2119))          # straxen's map holds all detectors
    plugin = wfsim_amd.RawRecordsFromMcChain(cfg)
    out = ministrax.run_plugin(plugin)
    rr = np.concatenate([c.data for c in out['raw_records']])
    rr_nv = np.concatenate([c.data for c in out['raw_records_nv']])
    truth = np.concatenate([c.data for c in out['truth']])
    truth_nv = np.concatenate([c.data for c in out['truth_nv']])
    assert len(rr) > 100 and len(rr_nv) > 50 and len(truth) == 2 * n_ev and len(truth_nv) == n_ev
    assert rr['channel'].max() < 494 and rr_nv['channel'].min() >= 2000 and rr_nv['channel'].max() <= 2119
    assert np.all(np.diff(rr['time']) >= 0) and np.all(np.diff(rr_nv['time']) >= 0)
    # both detectors saw event g at the same time (the nVeto photons arrive within ~100 ns, S1 photons within ~200 ns)
    ev_t = plugin.event_times
    for g in (0, 7, 39):
        assert np.abs(rr['time'] - ev_t[g]).min() < 2000 and np.abs(rr_nv['time'] - ev_t[g]).min() < 2000
    # ---- the records of both detectors are the oracle's for the synchronised instructions (a chunk is sorted by time, ties by channel)
    from wfsim_amd.dtypes import raw_record_dtype
    from wfsim_amd.physics import instruction_params
    from wfsim_amd.resource import Resource
    from wfsim_amd.scheduler import schedule

    def by_time(x):
        return x[np.lexsort((x['channel'], x['time']))]
    epix = plugin.instructions_epix
    order, key, cluster = schedule(epix, plugin.config)
    orc = make_oracle(plugin.config)
    orc.simulate(epix[order], order.astype(np.uint32), instruction_params(epix[order], plugin.config, Resource(plugin.config)))
    ref = np.frombuffer(orc.pack_records(), dtype=raw_record_dtype())
    assert by_time(rr).tobytes() == by_time(ref).tobytes()
    nvi = plugin.instructions_nveto
    assert np.array_equal(nvi['time'], ev_t[nvi['g4id'] - plugin.config['entry_start']])       # the event time replaces the (zero) nVeto instruction time
    orc_nv = make_oracle(plugin.config_nveto)
    orc_nv.simulate_optical(nvi, np.arange(len(nvi), dtype=np.uint32), plugin.nveto_channels, plugin.nveto_timings, int(1e6))
    ref_nv = np.frombuffer(orc_nv.pack_records(), dtype=raw_record_dtype()).copy()
    ref_nv['channel'] += 2000
    assert by_time(rr_nv).tobytes() == by_time(ref_nv).tobytes()
    # TPC only
    plugin = wfsim_amd.RawRecordsFromMcChain(dict(cfg, targets=('tpc',), entry_stop=None))
    out2 = ministrax.run_plugin(plugin)
    assert sum(len(c.data) for c in out2['raw_records_nv']) == 0 and sum(len(c.data) for c in out2['raw_records']) > 100


# ------------------------------------------------------------------------------------------------ golden chains J
# tests/golden/chain_optical.npz, chain_optical_cutoff.npz: runs of the reference's RawDataOptical (tests/test_optical_chain_reference.py
# pins the oracle on them; here the device)
TRUTH_COUNTS = ['n_photon', 'n_pe', 'n_photon_trigger', 'n_pe_trigger']


def _assert_truth_of_fixture(eng, d):
    acc, ts = eng.truth()
    assert len(acc) == len(d['call_kind'])
    for j, f in enumerate(TRUTH_COUNTS):
        assert np.array_equal(acc[:, j], d['call_truth_' + f]), f
        assert np.array_equal(acc[:, 6 + j], d['call_truth_' + f + '_bottom']), f
    assert np.array_equal(acc[:, 0], d['truth']['n_photon'])
    for j, f in [(4, 'raw_area'), (5, 'raw_area_trigger')]:
        assert np.allclose(acc[:, j], d['call_truth_' + f], rtol=1e-12, atol=0), f


@pytest.mark.parametrize('case', sorted(OPTICAL_CHAINS))
def test_optical_chain_replay_vs_reference(case):
    """the reference's photons (after its transit-time draw, with its gains; photons on the dead PMT dropped as Pulse.__call__ drops
    them) injected per Pulse call on the nVeto configuration, with the debug copies on -- which keeps the rows in the HBM accumulators
    (k_zle / k_pack; the resident kernel keeps no copies of currents or rows) -- in both arithmetic modes: pulses, windows, rows, ZLE
    intervals and record heads equal the fixture, the integer truth accumulators too.  The resident path:
    test_optical_chain_records_on_both_digitisation_paths"""
    from tests.test_gpu_parity import _check_chain
    d, eng = _check_chain(OPTICAL_CHAINS[case], optical_chain_config(case, row_resident=False))
    _assert_truth_of_fixture(eng, d)


@pytest.mark.parametrize('fma', [True, False])
@pytest.mark.parametrize('row_resident', [True, False])
@pytest.mark.parametrize('case', sorted(OPTICAL_CHAINS))
def test_optical_chain_records_on_both_digitisation_paths(case, row_resident, fma):
    """the same replay without debug copies, so that config row_resident selects the path: on -- every (window, channel) row made,
    finished and zero-suppressed by k_row_pulse -- and off (accumulators, k_zle, k_pack); which kernel ran is asserted from the kernel
    timers.  Either way, in both arithmetic modes, the records are the fixture's ZLE tuples fragment by fragment (time, channel,
    pulse_length, record_i, length and every data sample, in the reference's yield order) and the integer truth is the fixture's."""
    from tests.helpers import replay_chain_on_engine, with_fma
    from wfsim_amd.dtypes import raw_record_dtype
    d = golden(OPTICAL_CHAINS[case])
    cfg = with_fma(optical_chain_config(case, row_resident=row_resident), fma)
    eng = make_engine(cfg)
    replay_chain_on_engine(eng, d, cfg, debug=False)
    rec = eng.records()
    spr = np.dtype(raw_record_dtype())['data'].shape[0]
    plen = d['zle_right'] - d['zle_left'] + 1
    nfrag = -(-plen // spr)
    assert len(rec) == nfrag.sum() and len(plen) > 50
    iv = np.repeat(np.arange(len(plen)), nfrag)                                   # interval of every fragment
    frag = np.arange(len(rec)) - np.repeat(np.cumsum(nfrag) - nfrag, nfrag)       # its number inside the interval
    assert np.array_equal(rec['record_i'], frag)
    assert np.array_equal(rec['channel'], d['zle_ch'][iv])
    assert np.array_equal(rec['time'], 10 * (d['zle_left'][iv] + spr * frag))
    assert np.array_equal(rec['pulse_length'], plen[iv])
    assert np.array_equal(rec['length'], np.minimum(spr, plen[iv] - spr * frag))
    assert np.all(rec['dt'] == 10) and np.all(rec['baseline'] == 0)
    data = np.concatenate([rec['data'][k][:rec['length'][k]] for k in range(len(rec))])
    assert np.array_equal(data, d['zle_data'])
    assert all(not rec['data'][k][rec['length'][k]:].any() for k in range(len(rec)))          # the tail of a last fragment is zero
    _assert_truth_of_fixture(eng, d)
    g = eng.groups()
    keep = g['right'] >= g['left']
    assert np.array_equal(g['left'][keep], d['dg_left']) and np.array_equal(g['right'][keep], d['dg_right'])
    # which path made the rows: the same batch once more with the kernel timers on
    eng.set_profiling(True)
    eng.run()
    kt = eng.kernel_times()
    assert ('k_row_pulse' in kt) == row_resident, sorted(kt)
    assert eng.records().tobytes() == rec.tobytes()


@pytest.mark.parametrize('case', sorted(OPTICAL_CHAINS))
def test_raw_data_optical_on_the_reference_inputs(case):
    """wfsim_amd.RawDataOptical.iter_windows on the stored instructions / channels / timings (case 'cutoff': a non-default
    nveto_time_max_cutoff through load_optical).  Calls, photons per call and channel and n_photon of the truth rows equal the
    fixture; the entry times cannot be read off the device (it adds its own transit-time draw), so the device's photons equal the
    oracle's photon by photon and the oracle's entry times equal the fixture's (as in tests/test_optical_chain_reference.py)"""
    d = golden(OPTICAL_CHAINS[case])
    cfg = optical_chain_config(case, seed=61)
    ins, channels, timings = d['instructions'], d['channels'], d['timings']
    cutoff = cfg.get('nveto_time_max_cutoff', int(1e6))
    assert cutoff == int(d['cutoff']) and np.all(np.diff(ins['time']) >= 0)
    rd = wfsim_amd.RawDataOptical(cfg, channels=channels, timings=timings)
    rd.engine.keep_photons = True
    tb = np.zeros(2 * len(ins), dtype=instruction_dtype + optical_extra_dtype + truth_extra_dtype + [('fill', bool)])
    windows = list(rd.iter_windows(ins, truth_buffer=tb))
    truth = tb[tb['fill']]
    # ---- against the fixture: one call per instruction in the reference's order, live photons per call
    assert len(truth) == len(d['truth']) == len(ins)
    assert np.array_equal(truth['event_number'], d['truth']['event_number'])
    assert np.array_equal(truth['n_photon'], d['truth']['n_photon'])
    assert np.array_equal(truth['_first'], d['truth']['_first']) and np.array_equal(truth['_last'], d['truth']['_last'])
    # ---- against the oracle, photon by photon (one batch: the engine still holds it)
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, cutoff)
    o = orc.results()
    ph = rd.engine.photons()
    live = np.asarray(cfg['gains']) > 0
    assert len(ph['set_off']) - 1 == len(o['call_ph_off']) - 1 == len(ins)
    for k in range(len(ins)):
        a, b = o['call_ph_off'][k], o['call_ph_off'][k + 1]
        c, e = ph['set_off'][k], ph['set_off'][k + 1]
        mo, mg = live[o['ph_ch'][a:b]], live[ph['ch'][c:e]]
        ko = np.lexsort((o['ph_gain'][a:b][mo], o['ph_t'][a:b][mo], o['ph_ch'][a:b][mo]))
        kg = np.lexsort((ph['gain'][c:e][mg], ph['t'][c:e][mg], ph['ch'][c:e][mg]))
        assert mo.sum() == mg.sum() == d['truth']['n_photon'][k], k
        for f, g in [('ph_ch', 'ch'), ('ph_t', 't'), ('ph_gain', 'gain'), ('ph_dpe', 'dpe')]:
            assert np.array_equal(o[f][a:b][mo][ko], ph[g][c:e][mg][kg]), (k, f)
    # DESIGN.md 4 leaves the order of supplied photons inside a channel unpinned against the REFERENCE (numpy's unstable argsort); device and
    # oracle both keep the input's order, so between them the tiles are compared in order
    assert_tiles_in_oracle_order(rd.engine, o, list(range(len(ins))), live=live)
    # ---- photons per call and channel as the reference's sim_primary left them
    chan_of = lambda off, ch: [np.bincount(np.asarray(ch[a:b])[live[ch[a:b]]], minlength=120).tolist() for a, b in zip(off[:-1], off[1:])]
    assert chan_of(ph['set_off'], ph['ch']) == chan_of(d['call_in_off'], d['in_ch'])
    assert photons_by_call_and_channel(o['call_ph_off'], o['opt_in_t'], o['opt_in_ch']) == \
        photons_by_call_and_channel(d['call_in_off'], d['in_t'], d['in_ch'])
    # ---- windows and records: the oracle's for the same streams
    assert np.array_equal([w['left'] for w in windows], o['dg_left']) and np.array_equal([w['right'] for w in windows], o['dg_right'])
    assert np.concatenate([w['records'] for w in windows]).tobytes() == orc.pack_records().tobytes()


def test_optical_batch_after_a_run_set_batch_on_the_same_engine():
    """Engine.load_optical after a batch with run sets (save_full_truth off: S1s that share Pulse calls, sets numbered by their first
    instruction -- rows 0, 3, 5 of 6): truth(), photons() and electron_stats() of the optical batch are its own rows, not a remap
    through the earlier batch's sets; the truth is the fixture's"""
    from wfsim_amd.physics import instruction_params
    from wfsim_amd.resource import Resource
    from wfsim_amd.scheduler import schedule, run_sets
    d = golden(OPTICAL_CHAINS['main'])
    dummy = ['constant dummy', 1, [120]]
    cfg = optical_chain_config('main', seed=62, save_full_truth=False, s1_pattern_map=dummy, s2_pattern_map=dummy)
    eng = make_engine(cfg)
    s1 = np.zeros(6, dtype=instruction_dtype)
    s1['type'], s1['amp'], s1['z'], s1['recoil'] = 1, 400, -10, 7
    s1['time'] = [1_000_000, 1_000_050, 1_000_090, 1_003_000, 1_003_020, 1_009_000]
    order, key, cluster = schedule(s1, cfg)
    rs, n_sets = run_sets(s1[order], key, cluster, cfg)
    assert rs.tolist() == [0, 0, 0, 1, 1, 2]
    eng.load_instructions(s1[order], order.astype(np.uint32), cluster, key, instruction_params(s1[order], cfg, Resource(cfg)), run_set=rs)
    counts = eng.run()
    acc, _ = eng.truth()
    assert counts['n_pulse_sets'] == len(acc) == 3 and np.all(acc[:, 0] > 0)
    # ---- the optical chain on the same engine
    ins = d['instructions']
    order, key, cluster = schedule(ins, cfg)
    assert np.array_equal(order, np.arange(len(ins)))
    eng.load_optical(ins, order.astype(np.uint32), cluster, key, d['channels'], d['timings'], int(d['cutoff']))
    counts = eng.run()
    acc, ts = eng.truth()
    assert counts['n_pulse_sets'] == len(acc) == len(ins)
    assert np.array_equal(acc[:, 0], d['truth']['n_photon'])
    ph = eng.photons()
    live = np.asarray(cfg['gains']) > 0
    assert len(ph['set_off']) == len(ins) + 1
    assert [int(live[ph['ch'][a:b]].sum()) for a, b in zip(ph['set_off'][:-1], ph['set_off'][1:])] == d['truth']['n_photon'].tolist()
    assert len(eng.electron_stats()) == len(ins)
    # and the same truth as a fresh engine
    fresh = make_engine(cfg)
    fresh.load_optical(ins, order.astype(np.uint32), cluster, key, d['channels'], d['timings'], int(d['cutoff']))
    fresh.run()
    assert np.array_equal(fresh.truth()[0], acc) and np.array_equal(fresh.truth()[1], ts, equal_nan=True)
