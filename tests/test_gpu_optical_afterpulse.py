"""PMT afterpulses behind supplied photons on the GPU (RawDataOptical with enable_pmt_afterpulses, rawdata.py:166-190: the afterpulse
Pulse call runs behind EVERY primary call, the optical ones included).  The expectation is tests/optical_afterpulse.py: the oracle's
primaries, the restated afterpulse call (afterpulses_of) and the call-by-call driver (drive_optical), all three pinned on the CPU in
tests/test_optical_afterpulse_cpu.py.  Everything is compared exactly: photon times, channels and gains, windows, record bytes."""
import functools

import numpy as np
import pytest

import wfsim_amd
from tests import optical_afterpulse as OA
from tests.helpers import assert_tiles_in_oracle_order, make_engine, make_oracle, with_fma
from tests.test_optical_afterpulse_cpu import scaled_tables
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype, raw_record_dtype, truth_extra_dtype
from wfsim_amd.engine import WfsError
from wfsim_amd.scheduler import schedule
from wfsim_amd.workloads import nveto_config

pytestmark = pytest.mark.gpu

CUTOFF = int(1e6)
AP_KERNELS = ('k_optical_ap_screen', 'k_ap_finish', 'k_ap_count', 'k_ap_place', 'k_tile_order_scan', 'k_tile_order', 'k_tile_order_big',
              'k_tile_order_huge')


# ------------------------------------------------------------------------------------------------ shared inputs and expectations
def nveto_ap_config(on=True, **kw):
    """the 120-channel nVeto configuration with the first 120 rows of the golden afterpulse tables attached by hand (the reference
    loads none for this detector), every probability times 4 and modifier 1.3: about a quarter of the parents fire"""
    return nveto_config(seed=41, enable_pmt_afterpulses=on, uniform_to_pmt_ap=scaled_tables(4, rows=120), pmt_ap_modifier=1.3,
                        pmt_ap_t_modifier=3, **kw)


@functools.lru_cache(maxsize=None)
def nveto_input():
    return OA.edge_input(300, 120, seed=17, max_photons=8, dead_channel=7)


@functools.lru_cache(maxsize=None)
def nveto_expected(fma=True):
    """(windows left, right, record bytes, afterpulses per call) of the driver on the nVeto-shaped input; computed once"""
    cfg = with_fma(nveto_ap_config(), fma)
    ins, channels, timings = nveto_input()
    orc, aps, order = OA.drive_optical(cfg, ins, channels, timings, CUTOFF, ap_tables=cfg['uniform_to_pmt_ap'])
    assert np.array_equal(order, np.arange(len(ins)))
    o = orc.results()
    return o['dg_left'], o['dg_right'], orc.pack_records().tobytes(), aps


def run_windows(cfg, ins, channels, timings, max_batch_quanta=None, truth=False, profiling=False):
    rd = wfsim_amd.RawDataOptical(cfg, channels=channels, timings=timings)
    rd.engine.keep_photons = True
    if max_batch_quanta is not None:
        rd.max_batch_quanta = max_batch_quanta
    if profiling:
        rd.engine.set_profiling(True)
    tb = np.zeros(2 * len(ins), dtype=instruction_dtype + optical_extra_dtype + truth_extra_dtype + [('fill', bool)]) if truth else None
    windows = list(rd.iter_windows(ins, truth_buffer=tb))
    rec = np.concatenate([w['records'] for w in windows]) if windows else np.zeros(0, dtype=raw_record_dtype())
    return rd, windows, rec, (tb[tb['fill']] if truth else None)


def assert_photons(cfg, eng, ins, channels, timings, tables):
    """Engine.photons() of one optical batch with afterpulses: primary set k = the oracle's call k; afterpulse set n + k =
    afterpulses_of for call k, in order (parents on a turned-off PMT are dropped at bucketing: their afterpulses would land on the
    same dead channel and leave the reference's Pulse call at once)"""
    n = len(ins)
    _, o, order, items = OA.optical_primaries(cfg, ins, channels, timings, CUTOFF, make_oracle)
    assert np.array_equal(order, np.arange(n))
    ph = eng.photons()
    live = np.asarray(cfg['gains']) > 0
    assert len(ph['set_off']) - 1 == 2 * n
    n_ap, sizes = 0, []
    for k in range(n):
        a, b = o['call_ph_off'][k], o['call_ph_off'][k + 1]
        c, e = ph['set_off'][k], ph['set_off'][k + 1]
        mo = live[o['ph_ch'][a:b]]
        ko = np.lexsort((o['ph_gain'][a:b][mo], o['ph_t'][a:b][mo], o['ph_ch'][a:b][mo]))
        kg = np.lexsort((ph['gain'][c:e], ph['t'][c:e], ph['ch'][c:e]))
        assert mo.sum() == e - c, k
        for f, g in [('ph_ch', 'ch'), ('ph_t', 't'), ('ph_gain', 'gain'), ('ph_dpe', 'dpe')]:
            assert np.array_equal(o[f][a:b][mo][ko], ph[g][c:e][kg]), (k, f)
        t, ch, gain = OA.afterpulses_of_call(cfg, tables, o, k, k, items[k]) if b > a else (np.zeros(0, np.int64),) * 3
        keep = live[ch] if len(ch) else np.zeros(0, bool)
        c, e = ph['set_off'][n + k], ph['set_off'][n + k + 1]
        assert e - c == keep.sum(), (k, e - c, keep.sum())
        assert np.array_equal(ph['t'][c:e], t[keep]) and np.array_equal(ph['ch'][c:e], ch[keep]) and np.array_equal(ph['gain'][c:e], gain[keep]), k
        n_ap += e - c
        sizes += np.bincount(ch[keep]).tolist() if keep.any() else []
    # DESIGN.md 4 leaves the order of supplied photons inside a channel unpinned against the REFERENCE; device and oracle both keep the input's
    # order, so the parents' tiles are compared in order too (the afterpulse sets were, above)
    assert_tiles_in_oracle_order(eng, o, list(range(n)), live=live)
    return o['call_ph_off'][-1], n_ap, np.asarray(sizes)


# ------------------------------------------------------------------------------------------------ (a) photon by photon
def test_photons_nveto_shape():
    cfg = nveto_ap_config()
    ins, channels, timings = nveto_input()
    nph = ins['_last'] - ins['_first']
    kept = (timings >= 0) & (timings < CUTOFF)
    assert nph[3] == 0 and not kept[ins['_first'][5]:ins['_last'][5]].any() and nph[5] > 0 and ins['time'][10] == ins['time'][11]
    assert ((channels == 7) & kept).sum() >= 3 and (timings[kept] > 1500).sum() >= 3
    rd, windows, rec, _ = run_windows(cfg, ins, channels, timings)
    n_par, n_ap, _ = assert_photons(cfg, rd.engine, ins, channels, timings, cfg['uniform_to_pmt_ap'])
    print('parents', n_par, 'afterpulses', n_ap)
    assert n_ap > 150


def tpc_order_input():
    """four instructions on 494 channels whose afterpulse tiles fall into every class of the order pass: photons spread thin (tiles of
    up to 12), then 100, 2 000 and 12 000 photons on one channel (13 .. 64, 65 .. 4096, above 4096 with about half the parents firing)"""
    rng = np.random.default_rng(23)
    nph = np.array([400, 100, 2000, 12000])
    ins = np.zeros(4, dtype=instruction_dtype + optical_extra_dtype)
    ins['type'], ins['time'], ins['event_number'], ins['amp'] = 1, 1_000_000 + 20_000 * np.arange(4), np.arange(4), nph
    ins['_last'] = np.cumsum(nph)
    ins['_first'] = ins['_last'] - nph
    channels = np.concatenate([rng.integers(0, 494, 400), np.full(100, 31), np.full(2000, 300), np.full(12000, 77)])
    timings = rng.exponential(200, int(nph.sum())).astype(np.int64)
    return ins, channels, timings


def test_photons_tpc_shape_every_order_class():
    tables = scaled_tables(8)
    cfg = xenonnt_test_config(seed=43, enable_pmt_afterpulses=True, uniform_to_pmt_ap=tables, pmt_ap_modifier=1.3, pmt_ap_t_modifier=3)
    ins, channels, timings = tpc_order_input()
    rd, windows, rec, _ = run_windows(cfg, ins, channels, timings, profiling=True)
    kt = rd.engine.kernel_times()
    n_par, n_ap, sizes = assert_photons(cfg, rd.engine, ins, channels, timings, tables)
    print('parents', n_par, 'afterpulses', n_ap, 'largest afterpulse tiles', np.sort(sizes)[-4:], {k: kt[k] for k in AP_KERNELS if k in kt})
    assert n_par <= 20000
    assert (sizes <= 12).any() and ((sizes > 12) & (sizes <= 64)).any() and ((sizes > 64) & (sizes <= 4096)).any() and (sizes > 4096).any()
    for k in ('k_optical_ap_screen', 'k_tile_order', 'k_tile_order_big', 'k_tile_order_huge'):
        assert k in kt, (k, sorted(kt))


# ------------------------------------------------------------------------------------------------ (b) records end to end
@pytest.mark.parametrize('max_batch_quanta', [200, 5000, 2_000_000_000])
@pytest.mark.parametrize('fma', [True, False])
@pytest.mark.parametrize('row_resident', [True, False])
def test_records_end_to_end(row_resident, fma, max_batch_quanta):
    left, right, rec_bytes, aps = nveto_expected(fma)
    cfg = with_fma(nveto_ap_config(row_resident=row_resident), fma)
    ins, channels, timings = nveto_input()
    rd, windows, rec, _ = run_windows(cfg, ins, channels, timings, max_batch_quanta=max_batch_quanta, profiling=True)
    kt = rd.engine.kernel_times()                   # (of the last batch: its last instruction holds photons)
    assert np.array_equal([w['left'] for w in windows], left) and np.array_equal([w['right'] for w in windows], right)
    assert rec.tobytes() == rec_bytes
    assert ('k_row_pulse' in kt) == row_resident, sorted(kt)
    assert 'k_optical_ap_screen' in kt


def test_the_input_discriminates():
    """the afterpulses change windows and records of the nVeto-shaped input: the comparison above cannot pass without them"""
    left, right, rec_bytes, aps = nveto_expected(True)
    cfg = nveto_ap_config(on=False)
    ins, channels, timings = nveto_input()
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, CUTOFF)
    off_bytes = orc.pack_records().tobytes()
    n_ap = sum(len(x[0]) for x in aps if x is not None)
    print('afterpulses', n_ap, 'windows', len(orc.get('dg_left')), '->', len(left), 'records', len(off_bytes) // 244, '->', len(rec_bytes) // 244)
    assert n_ap > 150 and len(rec_bytes) > len(off_bytes) and len(left) < len(orc.get('dg_left'))


# ------------------------------------------------------------------------------------------------ (c) truth
def test_afterpulses_enter_no_truth_row():
    ins, channels, timings = nveto_input()
    _, _, _, t_on = run_windows(nveto_ap_config(), ins, channels, timings, truth=True)
    _, _, _, t_off = run_windows(nveto_ap_config(on=False), ins, channels, timings, truth=True)
    assert len(t_on) == len(t_off) == len(ins)
    for f in t_on.dtype.names:
        assert np.array_equal(t_on[f], t_off[f], equal_nan=t_on[f].dtype.kind == 'f'), f


# ------------------------------------------------------------------------------------------------ (d) second run
def test_second_run_of_a_loaded_batch():
    cfg = nveto_ap_config()
    ins, channels, timings = nveto_input()
    rd, windows, rec, _ = run_windows(cfg, ins, channels, timings)
    eng = rd.engine
    rec1, ph1 = eng.records().tobytes(), eng.photons()
    assert len(ph1['set_off']) - 1 == 2 * len(ins) and ph1['set_off'][-1] > ph1['set_off'][len(ins)]
    eng.run()
    ph2 = eng.photons()
    assert eng.records().tobytes() == rec1
    for f in ph1:
        assert np.array_equal(ph1[f], ph2[f]), f
    assert rec1 == nveto_expected(True)[2]


# ------------------------------------------------------------------------------------------------ (e) plugin
def test_optical_tpc_plugin():
    from wfsim_amd import ministrax
    tables = scaled_tables(4)
    ins, channels, timings = OA.edge_input(200, 494, seed=29, max_photons=12)
    kw = dict(seed=47, enable_pmt_afterpulses=True, uniform_to_pmt_ap=tables, pmt_ap_modifier=1.3, pmt_ap_t_modifier=3, right_raw_extension=2000)
    cfg = xenonnt_test_config(chunk_size=0.0002, instructions=ins, channels=channels, timings=timings, **kw)
    plugin = wfsim_amd.RawRecordsFromFaxOpticalNT(cfg)
    out = ministrax.run_plugin(plugin)
    rr = np.concatenate([c.data for c in out['raw_records']])
    truth = np.concatenate([c.data for c in out['truth']])
    assert len(out['raw_records']) >= 2 and len(truth) == len(ins)
    assert np.all(np.diff(rr['time']) >= 0) and rr['channel'].max() < 494

    def by_time(x):
        return x[np.lexsort((x['channel'], x['time']))]
    pcfg = plugin.config
    orc, aps, order = OA.drive_optical(pcfg, plugin.instructions, plugin.channels, plugin.timings, CUTOFF, ap_tables=tables)
    ref = np.frombuffer(orc.pack_records(), dtype=raw_record_dtype())
    print('records', len(rr), 'afterpulses', sum(len(x[0]) for x in aps if x is not None), 'chunks', len(out['raw_records']))
    assert sum(len(x[0]) for x in aps if x is not None) > 100
    assert by_time(rr).tobytes() == by_time(ref).tobytes()


# ------------------------------------------------------------------------------------------------ (f) fixture replay on the device
@pytest.mark.parametrize('row_resident', [False, True])
def test_fixture_replay_on_the_device(row_resident):
    """the reference's RawDataOptical run with afterpulses on (tests/golden/chain_optical_ap.npz), its photons injected call by call"""
    from tests.helpers import golden, replay_chain_on_engine
    from tests.test_gpu_parity import _check_chain
    from tests.test_optical_afterpulse_cpu import optical_ap_chain_config
    cfg = optical_ap_chain_config(row_resident=row_resident)
    if not row_resident:
        _check_chain('chain_optical_ap.npz', cfg)
        return
    d = golden('chain_optical_ap.npz')
    for fma in (True, False):
        eng = make_engine(with_fma(cfg, fma))
        replay_chain_on_engine(eng, d, cfg, debug=False)
        rec = eng.records()
        spr = np.dtype(raw_record_dtype())['data'].shape[0]
        plen = d['zle_right'] - d['zle_left'] + 1
        nfrag = -(-plen // spr)
        iv = np.repeat(np.arange(len(plen)), nfrag)
        frag = np.arange(len(rec)) - np.repeat(np.cumsum(nfrag) - nfrag, nfrag)
        assert len(rec) == nfrag.sum() and len(plen) > 50
        assert np.array_equal(rec['channel'], d['zle_ch'][iv]) and np.array_equal(rec['time'], 10 * (d['zle_left'][iv] + spr * frag))
        assert np.array_equal(rec['pulse_length'], plen[iv]) and np.array_equal(rec['record_i'], frag)
        data = np.concatenate([rec['data'][k][:rec['length'][k]] for k in range(len(rec))])
        assert np.array_equal(data, d['zle_data'])
        g = eng.groups()
        keep = g['right'] >= g['left']
        assert np.array_equal(g['left'][keep], d['dg_left']) and np.array_equal(g['right'][keep], d['dg_right'])
        eng.set_profiling(True)
        eng.run()
        assert 'k_row_pulse' in eng.kernel_times()


# ------------------------------------------------------------------------------------------------ (g) capacity
def test_capacity_error_and_the_batch_after_it():
    """more candidates than P / 8 + 65536: the engine's capacity error (every write of the lists is guarded by their capacity); the
    next batch on the same engine runs and gives the bytes of a fresh engine"""
    tables = scaled_tables(12, rows=120)           # modifier 1.3: about three parents in four are candidates
    cfg = nveto_config(seed=53, enable_pmt_afterpulses=True, uniform_to_pmt_ap=tables, pmt_ap_modifier=1.3)
    rng = np.random.default_rng(5)
    n, per = 100, 2000
    ins = np.zeros(n, dtype=instruction_dtype + optical_extra_dtype)
    ins['type'], ins['time'], ins['event_number'] = 1, 1_000_000 + 1000 * np.arange(n), np.arange(n)
    ins['_last'] = per * (1 + np.arange(n))
    ins['_first'] = ins['_last'] - per
    channels = rng.integers(0, 120, n * per)
    channels[channels == 7] = 8
    timings = rng.exponential(60, n * per).astype(np.int64)
    eng = make_engine(cfg)
    order, key, cluster = schedule(ins, cfg)
    eng.load_optical(ins[order], order.astype(np.uint32), cluster, key, channels, timings, CUTOFF)
    with pytest.raises(WfsError, match='afterpulse probability unreasonably high'):
        eng.run()
    small, sch, st = OA.edge_input(40, 120, seed=3, dead_channel=7)
    order, key, cluster = schedule(small, cfg)
    fresh = make_engine(cfg)
    out = []
    for e in (eng, fresh):
        e.load_optical(small[order], order.astype(np.uint32), cluster, key, sch, st, CUTOFF)
        counts = e.run()
        out.append((e.records().tobytes(), counts['n_photons']))
    assert out[0] == out[1] and len(out[0][0]) > 0
    n_prim = ((st >= 0) & (st < CUTOFF) & (sch != 7)).sum()
    assert out[0][1] > n_prim                      # (afterpulse photons on top of the primaries)


# ------------------------------------------------------------------------------------------------ (h) off is off
def test_off_is_off():
    cfg = nveto_ap_config(on=False)
    ins, channels, timings = nveto_input()
    rd, windows, rec, _ = run_windows(cfg, ins, channels, timings, profiling=True)
    kt = rd.engine.kernel_times()
    assert 'k_optical_finish' in kt and not [k for k in kt if k in AP_KERNELS or k.startswith('k_ap_')], sorted(kt)
    assert len(rd.engine.photons()['set_off']) - 1 == len(ins)
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, CUTOFF)
    assert np.array_equal([w['left'] for w in windows], orc.get('dg_left'))
    assert rec.tobytes() == orc.pack_records().tobytes()
