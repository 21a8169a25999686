"""Random instruction mixes under peaked hit patterns on the GPU (MI355X only): the cases of tests/hot_patterns.py, whose tiles run from
nothing to several 10^4 photons, so that k_s2_bright and its passes, k_s2_tile_gen, the fit rule, k_tile_add of bright tiles, the dense
pulse kernel and the large order classes behind the block generator meet run sets, resident rows, noise, HE rows, the sum row, batch
cuts, shards and an engine that is used again (tests/test_hot_patterns_cpu.py counts which seam each seed reaches).

Every comparison is one the suite already makes: device against the CPU oracle on the same Philox streams -- photons per pulse set, digitise
windows, record bytes, n_pe, the 12 truth columns, the per-PMT truth of the brightest tiles, the sum rows -- or device against device.  With
the map on the device the oracle is fed the device's rows (Engine.cdf_rows()), which must agree with the host map at rtol 1e-6.
Which kernel made a tile (Engine.tile_kernels()) is checked against rules that do not restate the fit rule.  Every launch is checked."""
import contextlib
import functools
import os

import numpy as np
import pytest

from tests import hot_patterns as H
from tests.helpers import assert_tiles_in_oracle_order, make_engine
from tests.sum_signal import SUM_CHANNEL, assert_sum_rows, expected_sum_rows
from tests.test_gpu_bright_tiles import _oracle_truth_per_pmt
from wfsim_amd import workloads as W
from wfsim_amd.config import kernel_params
from wfsim_amd.dtypes import instruction_dtype
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu
INT_TRUTH, FLOAT_TRUTH = [0, 1, 2, 3, 6, 7, 8, 9], [4, 5, 10, 11]          # n_photon, n_pe, n_photon_trigger, n_pe_trigger | raw_area, raw_area_trigger (all, bottom)


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')          # every launch checked on the spot
    monkeypatch.delenv('WFS_BRIGHT_MAX_BINS', raising=False)


def _set_knobs(monkeypatch, knobs):
    """the engine reads its environment when it is made"""
    monkeypatch.delenv('WFS_BRIGHT_MAX_BINS', raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@contextlib.contextmanager
def _knob_env(knobs):
    """the same for results that are computed once and shared"""
    old = os.environ.pop('WFS_BRIGHT_MAX_BINS', None)
    os.environ.update(knobs)
    try:
        yield
    finally:
        os.environ.pop('WFS_BRIGHT_MAX_BINS', None)
        if old is not None:
            os.environ['WFS_BRIGHT_MAX_BINS'] = old


def _run_device(cfg, ins, profiling=False, eng=None):
    """(engine, counts, scheduled batch): rows from the device map where the engine holds it, host rows otherwise"""
    res = H.resource_of(cfg)
    eng = eng or make_engine(cfg, resource=res)
    if profiling:
        eng.set_profiling(True)
    s = H.scheduled(cfg, ins, res, device_maps=eng.device_maps)
    eng.load_instructions(s['s_ins'], s['gid'], s['cluster'], s['key'], s['ip'], run_set=s['run_set'])
    return eng, eng.run(), s, res


def _oracle_on_device_rows(cfg, ap, eng, s, res):
    """the oracle on the rows the generator used: (oracle, results, batch with those rows)"""
    if eng.device_maps:
        row, table = eng.cdf_rows()
        s = dict(s, ip=dict(s['ip'], cdf_row=row, cdf_table=table))
    orc, o = H.run_oracle(cfg, ap, res, s)
    return orc, o, s


def _device_sets(o, s):
    """(device pulse set of every oracle call, device set of every primary call, primary sets of the device): the oracle's calls come in
    processing order, each followed by its PMT-afterpulse call if it has photons; the device numbers the primary sets by instruction (or
    by the caller's run set) and the afterpulse set of set i is n + i"""
    if s['run_set'] is None:
        of_call = np.array([np.flatnonzero(s['call'] == q)[0] for q in range(s['n_calls'])], dtype=np.int64)
        n_prim = len(s['s_ins'])
    else:
        of_call, n_prim = np.arange(s['n_calls']), s['n_calls']
    sets, q = [], -1
    for kind in o['call_kind']:
        q += kind != 3
        sets.append(of_call[q] if kind != 3 else n_prim + of_call[q])
    assert q == s['n_calls'] - 1
    return np.asarray(sets, dtype=np.int64), of_call, n_prim


def _compare(cfg, noise, orc, o, eng, counts, s):
    """the comparison of tests/test_gpu_generation.py::_compare with run sets and the sum row allowed for: photons per pulse set, every tile in
    the oracle's order (tests/helpers.py: assert_tiles_in_oracle_order), digitise windows, record bytes, n_pe; then the 12 truth columns of every call, set by set"""
    ph = eng.photons()
    assert counts['n_photons'] == len(o['ph_t'])
    sets, of_call, n_prim = _device_sets(o, s)
    if 3 in o['call_kind']:
        assert counts['n_pulse_sets'] == 2 * n_prim
    assert len(ph['set_off']) == counts['n_pulse_sets'] + 1 and counts['n_pulse_sets'] in (n_prim, 2 * n_prim)
    for k, i in enumerate(sets):
        a, b = o['call_ph_off'][k], o['call_ph_off'][k + 1]
        c, e = ph['set_off'][i], ph['set_off'][i + 1]
        assert b - a == e - c, f'call {k}, set {i}: {b - a} vs {e - c} photons'
    assert_tiles_in_oracle_order(eng, o, sets)
    g = eng.groups()
    keep = g['right'] >= g['left']
    assert np.array_equal(g['left'][keep], o['dg_left']) and np.array_equal(g['right'][keep], o['dg_right'])
    if eng.emits_sum_records:          # the sum row: the restatement of tests/sum_signal.py on the oracle's pulses; every other channel as the oracle packs it
        rec = assert_sum_rows(eng, expected_sum_rows(o, kernel_params(cfg), orc.tables['thr_zle'], noise=noise))
        assert rec[rec['channel'] != SUM_CHANNEL].tobytes() == orc.pack_records().tobytes()
    else:
        assert eng.records().tobytes() == orc.pack_records().tobytes()
    assert counts['n_pe'] == orc.n_pe
    # truth rows (tests/test_gpu_bright_tiles.py::_assert_truth_rows, rtol 1e-9), paired by set identity; sets without a call hold nothing
    acc, ts = eng.truth()
    tr = o['truth'].reshape(-1, 12)
    assert len(tr) == len(sets) and len(acc) == counts['n_pulse_sets']
    for k, i in enumerate(sets):
        assert np.allclose(acc[i], tr[k], rtol=1e-9), (k, i, acc[i], tr[k])
    rest = np.setdiff1d(np.arange(len(acc)), sets)
    assert not acc[rest].any()
    return sets, of_call, n_prim


def _check_tile_kernels(cfg, knobs, eng, o, s, of_call, n_prim):
    """Engine.tile_kernels() against what needs no restatement of the fit rule; returns the kinds"""
    kind = eng.tile_kernels()
    n = np.zeros((n_prim, H.NCH), dtype=np.int64)
    tg = np.zeros(n_prim, dtype=bool)
    bright, tg_call, first = H.bright_tiles(cfg, s, o)
    n[of_call] = H.tile_sizes(o)[H.primary_calls(o)]
    tg[of_call] = tg_call
    assert kind.shape == n.shape and kind.dtype == np.int8
    made = tg[:, None] & (n > 0)
    assert np.all(kind[~made] == 0)                                           # no photons, or not tile-generated
    assert np.array_equal(kind == 1, made & (n <= H.BRIGHT))                  # k_s2_tile exactly up to 2048 photons
    assert np.all(np.isin(kind[made & (n > H.BRIGHT)], (2, 3)))
    if not cfg.get('tile_local_bright', True) or knobs.get('WFS_BRIGHT_MAX_BINS') == '0':
        assert not (kind == 3).any()
    passes = -(-n // H.PASS)
    for i in np.flatnonzero((kind == 3).any(axis=1)):                        # one delay table per instruction here: a tile that fits lets every
        fits = made[i] & (n[i] > H.BRIGHT) & (passes[i] <= passes[i][kind[i] == 3].max())      # bright tile with no more passes fit
        assert np.all(kind[i][fits] == 3), (i, n[i][fits], kind[i][fits])
    return kind, n, bright


# ------------------------------------------------------------------------------------------------------- 1: every seed against the oracle
@pytest.mark.parametrize('seed', range(H.N_SEEDS))
def test_hot_mix_matches_oracle(seed, monkeypatch):
    cfg, ins, ap, noise, knobs = H.hot_case(seed)
    _set_knobs(monkeypatch, knobs)
    eng, counts, s, res = _run_device(cfg, ins)
    assert eng.device_maps == ({'s2'} if seed % 2 == 0 else set())
    orc, o, s = _oracle_on_device_rows(cfg, ap, eng, s, res)
    if eng.device_maps:          # the device's rows against the host map (tests/test_gpu_pattern_maps.py)
        host = instruction_params(s['s_ins'], cfg, res)
        p_host = np.diff(host['cdf_table'][host['cdf_row']], axis=1, prepend=0.0)
        p_dev = np.diff(s['ip']['cdf_table'][s['ip']['cdf_row']], axis=1, prepend=0.0)
        s2 = s['s_ins']['type'] == 2
        assert np.allclose(p_dev[s2], p_host[s2], rtol=1e-6, atol=1e-12)
    sets, of_call, n_prim = _compare(cfg, noise, orc, o, eng, counts, s)
    kind, n, bright = _check_tile_kernels(cfg, knobs, eng, o, s, of_call, n_prim)
    print(f'seed {seed}: {counts["n_photons"]} photons, largest tile {int(n.max()) if n.size else 0}, tiles of k_s2_tile / k_s2_tile_gen / k_s2_bright: '
          f'{int((kind == 1).sum())} / {int((kind == 2).sum())} / {int((kind == 3).sum())}')
    # per-PMT truth of the brightest tile of every instruction that has a bright one (n_pe_trigger: the ballots of every pass)
    per_pmt = eng.truth_per_pmt()
    prim = H.primary_calls(o)
    sizes = H.tile_sizes(o)[prim]
    for q in np.flatnonzero(bright.any(axis=1)):
        ch = int(np.argmax(np.where(bright[q], sizes[q], 0)))
        ref = _oracle_truth_per_pmt(eng.config, o, int(prim[q]), ch)
        assert np.allclose(per_pmt[of_call[q], ch], ref, rtol=1e-9), (q, ch, per_pmt[of_call[q], ch], ref)


def test_long_block_segments_keep_generation_order():
    """Regression case of what the odd seeds found (1, 3, 5, 7, 9, 11, 13, 19, 21 failed in n_pe_trigger, run to run differently): the
    block generator's fast path (k_photon_fill, a block of 2048 photons of ONE instruction) put the photons of a (block, channel)
    segment into photon order only up to 64 photons and left longer ones "to k_tile_order", which never looks at the block ranges of a
    single-instruction set -- under a flat pattern no segment is that long, under a peaked one the hot channel's are, and the tile
    stayed in the order of the LDS atomics.  n_pe_trigger counts the photons above threshold among the FIRST n_dpe of the tile
    (pulse.py:255), so it depends on that order.  Three instructions of the block generator with 30 - 40 % of their light on one channel:
    an S1 that is alone in a partial block (480 photons), an S1 of ~70 blocks, an S2 with the tile-local generator off.  The hot tiles
    are in the oracle's order photon by photon, and everything _compare checks holds."""
    from wfsim_amd.config import xenonnt_test_config
    ins = np.zeros(3, dtype=instruction_dtype)
    ins['type'], ins['amp'], ins['z'] = [1, 1, 2], [5000, 1_500_000, 400], [-20.0, -40.0, -8.0]
    ins['time'] = [1_000_000, 3_000_000, 5_000_000]
    ins['x'], ins['y'] = [0.0, 10.0, -10.0], [0.0, 5.0, 5.0]
    ins['recoil'], ins['event_number'] = 7, np.arange(3)
    hot, share = [212, 91, 300], [0.3, 0.4, 0.35]
    p = np.zeros((3, H.NCH))
    for i in range(3):
        p[i], p[i, hot[i]] = (1.0 - share[i]) / (H.NCH - 1), share[i]
    cfg = xenonnt_test_config(seed=311, s2_secondary_sc_gain=100.0, tile_local_generation=False,
                              hot_rows=dict(xy=np.array([ins['x'], ins['y']], dtype=np.float64).T, p=p))
    eng, counts, s, res = _run_device(cfg, ins)
    orc, o, s = _oracle_on_device_rows(cfg, None, eng, s, res)
    sets, of_call, n_prim = _compare(cfg, None, orc, o, eng, counts, s)
    assert not eng.tile_kernels().any()
    ph = eng.photons()
    sizes = H.tile_sizes(o)
    for k, i in enumerate(sets):
        ch = int(np.argmax(sizes[k]))
        assert sizes[k, ch] > 64 and ch in hot
        a, b, c, e = o['call_ph_off'][k], o['call_ph_off'][k + 1], ph['set_off'][i], ph['set_off'][i + 1]
        so, sd = o['ph_ch'][a:b] == ch, ph['ch'][c:e] == ch
        assert np.array_equal(o['ph_t'][a:b][so], ph['t'][c:e][sd]) and np.array_equal(o['ph_gain'][a:b][so], ph['gain'][c:e][sd]), (k, ch)
    assert sizes.max() > 2048 * 8          # (segments of many blocks, each far above 64 photons)


# ------------------------------------------------------------------------------------------------------- 2: the knobs change no byte
@pytest.mark.parametrize('seed', H.KNOB_SEEDS)
def test_hot_mix_knobs_do_not_change_bytes(seed, monkeypatch):
    """tile_local_bright on / off x WFS_BRIGHT_MAX_BINS unset / 1400 / 0 x row_resident on / off: which kernel makes a bright tile and
    where a row lives change nothing -- record bytes identical, integer truth columns equal, the float ones at rtol 1e-12 (sums over
    the photons of a tile in another order).  No oracle."""
    cfg, ins, ap, noise, _ = H.hot_case(seed)
    first, side_by_side = None, False
    for bright in (True, False):
        for bins in (None, '1400', '0'):
            for resident in (True, False):
                _set_knobs(monkeypatch, {} if bins is None else {'WFS_BRIGHT_MAX_BINS': bins})
                eng, counts, s, res = _run_device(dict(cfg, tile_local_bright=bright, row_resident=resident), ins)
                kind = eng.tile_kernels()
                assert (kind >= 2).any() and ((kind == 3).any() <= (bright and bins != '0'))
                side_by_side |= bool((kind == 2).any() and (kind == 3).any())
                got = dict(records=eng.records().tobytes(), acc=eng.truth()[0], n_pe=counts['n_pe'], bright=kind >= 2)
                if first is None:
                    first = got
                    continue
                what = (bright, bins, resident)
                assert got['records'] == first['records'], what
                assert got['n_pe'] == first['n_pe'] and np.array_equal(got['bright'], first['bright']), what
                assert np.array_equal(got['acc'][:, INT_TRUTH], first['acc'][:, INT_TRUTH]), what
                assert np.allclose(got['acc'][:, FLOAT_TRUTH], first['acc'][:, FLOAT_TRUTH], rtol=1e-12, atol=0.0), what
    assert side_by_side and len(first['records']) > 0


# ------------------------------------------------------------------------------------------------------- 3: batch cuts
@functools.lru_cache(maxsize=None)
def _cut_runs(seed):
    """a case through RawData.iter_windows uncut and with max_batch_quanta 500, 5000 and 60000: [(windows, truth rows, held)], computed once.
    A window that is still open at the end of a batch is held back and simulated again with the next batch; `held` lists the windows
    (their left edge) in which that happened to an instruction with a bright tile."""
    import wfsim_amd
    from wfsim_amd.dtypes import truth_extra_dtype
    cfg, ins, ap, noise, knobs = H.batch_case(seed)

    def run(mbq):
        rd = wfsim_amd.RawData(cfg)
        rd.max_batch_quanta = mbq
        held, launch = [], rd._launch

        def logged(*a):
            L = launch(*a)
            kind = rd.engine.tile_kernels()
            rs = getattr(rd, '_run_set', None)
            is_bright = (kind >= 2).any(axis=1)[np.arange(len(L['ins'])) if rs is None else np.asarray(rs)]
            again = is_bright & (L['ins_group'] >= L['n_emit'])            # (n_emit < windows of the batch: the last one is held back)
            held.extend(int(x) for x in np.unique(L['groups']['left'][L['ins_group'][again]]))
            return L
        rd._launch = logged
        truth = np.zeros(4 * len(ins) + 10, dtype=instruction_dtype + truth_extra_dtype + [('fill', bool)])
        w = [(x['left'], x['right'], x['records'].tobytes()) for x in rd.iter_windows(ins, truth_buffer=truth)]
        return w, truth[truth['fill']], sorted(set(held))
    with _knob_env(knobs):
        return [run(mbq) for mbq in (2_000_000_000, 500, 5_000, 60_000)]


@pytest.mark.parametrize('seed', H.BATCH_SEEDS)
def test_hot_mix_small_batches_equal_one_batch(seed):
    """RawData.iter_windows with the map in the config: windows, record bytes and truth rows do not depend on max_batch_quanta (as
    test_random_mix_small_batches_equal_one_batch compares them); every window that was held back at a cut is a window of the uncut run"""
    (w1, t1, held1), *cut = _cut_runs(seed)
    assert held1 == [] and len(w1) > 0
    for w2, t2, held in cut:
        assert w1 == w2
        assert len(t1) == len(t2)
        for f in ('n_photon', 'n_pe', 't_first_photon', 't_last_photon', 'n_electron', 'amp', 'time', 'event_number'):
            assert np.array_equal(t1[f], t2[f], equal_nan=True), f
        assert np.allclose(t1['raw_area'], t2['raw_area'], rtol=1e-12)        # float sum over the photons of a tile: order dependent
        assert set(held) <= {w[0] for w in w1}
    print(f'seed {seed}: windows with a bright S2 held back at a cut and simulated again: {[h for _, _, h in cut]}')


def test_a_bright_s2_is_carried_across_a_cut():
    """in at least two of the cases above a bright S2 lies in a window that is carried across a cut (hot_patterns.CARRY_SEEDS: one
    case as drawn, two with the designed instructions of hot_patterns.batch_case)"""
    carried = [seed for seed in H.CARRY_SEEDS if any(held for _, _, held in _cut_runs(seed)[1:])]
    assert len(carried) >= 2, carried


# ------------------------------------------------------------------------------------------------------- 4: shards
@pytest.mark.parametrize('seed,world', list(zip(H.SHARD_SEEDS, [2, 3, 8, 3])))
def test_hot_mix_sharded_equals_single(seed, world, monkeypatch):
    """what every rank of a multi-GPU run would compute, one after the other on this GPU (test_random_mix_sharded_equals_single)"""
    import wfsim_amd
    from wfsim_amd.distributed import shard_clusters, safe_cut_gap
    cfg, ins, ap, noise, knobs = H.hot_case(seed)
    _set_knobs(monkeypatch, knobs)
    single = b''.join(w['records'].tobytes() for w in wfsim_amd.RawData(cfg).iter_windows(ins))
    order, key, cluster = schedule(ins, cfg)
    s_ins = ins[order]
    b = shard_clusters(cluster, np.maximum(s_ins['amp'], 1), world, key=key, min_gap=safe_cut_gap(cfg))
    parts = []
    for r in range(world):
        mine = s_ins[b[r]:b[r + 1]]
        if len(mine) == 0:
            continue
        rd = wfsim_amd.RawData(cfg)
        rd.global_ids = order[b[r]:b[r + 1]]
        parts.append(b''.join(w['records'].tobytes() for w in rd.iter_windows(mine)))
    assert len(parts) > 1 and b''.join(parts) == single and len(single) > 0


# ------------------------------------------------------------------------------------------------------- 5: electron afterpulses
@pytest.mark.parametrize('seed', H.EAP_SEEDS)
def test_hot_mix_with_electron_afterpulses(seed, monkeypatch):
    """RawData end to end under the map against the oracle's simulate_scheduled (test_random_mix_with_electron_afterpulses): the
    secondaries have an emitter base, so they take the block generator under a peaked row, next to the tile-generated primaries.  The
    oracle gets the device's rows of primaries and secondaries."""
    import wfsim_amd
    from tests.helpers import make_oracle
    from wfsim_amd.scheduler import feedback_schedule
    case, ins, _, _, knobs = H.hot_case(seed)
    _set_knobs(monkeypatch, knobs)
    rng = np.random.default_rng(5000 + seed)
    edges = np.linspace(0, float(rng.choice([150e3, 700e3])), 141)
    hist = np.exp(-np.arange(140) / 30.0); hist *= float(rng.choice([5e-4, 3e-3])) / hist.sum()
    cfg = dict(case, enable_electron_afterpulses=True, uniform_to_ele_ap=(hist, edges), enable_pmt_afterpulses=False, enable_noise=False,
               emit_sum_signal=False, high_energy_deamplification_factor=H.BASE['high_energy_deamplification_factor'])
    if rng.random() < 0.5:
        cfg.update(enable_gate_afterpulses=True, photoelectric_p=float(rng.choice([1e-4, 2e-3])))
    n = len(ins)
    rd = wfsim_amd.RawData(cfg)
    rd.max_batch_quanta = int(rng.choice([30_000, 2_000_000_000]))
    windows = list(rd.iter_windows(ins))
    rec = np.concatenate([w['records'] for w in windows]) if windows else np.zeros(0)
    sec, sec_gid, sec_base, sec_parent = rd.electron_afterpulse_instructions(ins, np.arange(n), with_parent=True)
    assert len(sec) > 0
    allins = np.concatenate([ins, sec]); gids = np.concatenate([np.arange(n), sec_gid])
    base = np.concatenate([np.zeros(n, np.uint32), sec_base]); parent = np.concatenate([np.full(n, -1), sec_parent])
    order, key, cluster, rs = feedback_schedule(allins, parent, cfg)
    s_ins, gid = allins[order], gids[order].astype(np.uint32)
    res = Resource(cfg)
    eng = rd.engine                                    # the rows of every instruction as the device evaluates them (no run)
    ip = instruction_params(s_ins, cfg, res, device_maps=eng.device_maps)
    eng.load_instructions(s_ins, gid, cluster, key, ip)
    row, table = eng.cdf_rows()
    orc = make_oracle(cfg)
    orc.simulate_scheduled(s_ins, gid, dict(ip, cdf_row=row, cdf_table=table), base[order], cluster, key, rs)
    o = orc.results()
    assert len(windows) == len(o['dg_left']) and np.array_equal([w['left'] for w in windows], o['dg_left'])
    assert (rec.tobytes() if len(rec) else b'') == orc.pack_records().tobytes()


# ------------------------------------------------------------------------------------------------------- 6: one engine, changing batches
def test_one_engine_hot_and_plain_batches(monkeypatch):
    """One engine over batches with bright tiles, without, with the huge order class next to them, nearly empty, without a photon, and
    with bright tiles again: every batch gives the record bytes, counts, truth and tile_kernels() of a fresh engine on the same batch
    (n_bright_tiles, max_bright_bins, n_order_huge and tile_kind go from non-zero to zero and back)."""
    cfg, ap, knobs, batches = H.one_engine_sequence()
    _set_knobs(monkeypatch, knobs)
    eng = None
    seen = []
    for name, ins in batches:
        eng, counts, s, res = _run_device(cfg, ins, profiling=True, eng=eng)
        got = dict(counts=dict(counts), records=eng.records().tobytes(), kind=eng.tile_kernels(), acc=eng.truth()[0], kt=eng.kernel_times())
        new, ncounts, _, _ = _run_device(cfg, ins, profiling=True)
        assert got['counts'] == dict(ncounts), name
        assert got['records'] == new.records().tobytes(), name
        assert np.array_equal(got['kind'], new.tile_kernels()), name
        assert np.array_equal(got['acc'][:, INT_TRUTH], new.truth()[0][:, INT_TRUTH]), name
        seen.append((name, got))
    by = dict(seen)
    assert (by['bright']['kind'] >= 2).any() and (by['bright_again']['kind'] == 2).any() and (by['bright_and_huge']['kind'] == 3).any()      # (deep tiles do not fit 1400 start bins, shallow ones do)
    assert not (by['none']['kind'] >= 2).any()
    assert 'k_tile_order_huge' in by['bright_and_huge']['kt'] and 'k_tile_order_huge' not in by['none']['kt'], sorted(by['bright_and_huge']['kt'])
    assert 'k_s2_bright' in by['bright_and_huge']['kt'] and 'k_s2_bright' not in by['none']['kt'] and 'k_s2_bright' not in by['tiny']['kt']
    assert by['tiny']['counts']['n_photons'] > 0 and by['empty']['counts']['n_photons'] == 0 and by['empty']['counts']['n_records'] == 0
    assert not by['empty']['kind'].any()


# ------------------------------------------------------------------------------------------------------- 7: the bench workload in miniature
@pytest.mark.parametrize('pmt_afterpulses', [False, True])
def test_bench_pattern_workload_in_miniature(pmt_afterpulses):
    """bench.py --workload s2map at three instructions: workloads.s2map_config + s2_batch(spread_xy=True), the bench's own config and
    generator.  Photons and records equal the oracle on the device's rows; bright tiles take k_s2_bright; more than 0.4 of the first
    instruction's photons sit in tiles above 2048 photons (the oracle on host rows: 0.496).  The dense pulse kernel has work only where a
    bright tile went through the photon array -- or, with PMT afterpulses, for the afterpulse tiles, which are pulsed by the tile classes."""
    cfg = W.s2map_config(seed=3, pmt_afterpulses=pmt_afterpulses)
    ins = W.s2_batch(3, spread_xy=True)
    ap = cfg['uniform_to_pmt_ap'] if pmt_afterpulses else None
    eng, counts, s, res = _run_device(cfg, ins, profiling=True)
    assert eng.device_maps == {'s2'}
    orc, o, s = _oracle_on_device_rows(cfg, ap, eng, s, res)
    sets, of_call, n_prim = _compare(cfg, None, orc, o, eng, counts, s)
    kind, n, bright = _check_tile_kernels(cfg, {}, eng, o, s, of_call, n_prim)
    assert (kind == 3).any()
    share = n[0][n[0] > H.BRIGHT].sum() / n[0].sum()
    print(f'photons {counts["n_photons"]}; share of the first instruction in tiles above 2048 photons: {share:.3f} ({int((n[0] > H.BRIGHT).sum())} tiles)')
    assert share > 0.4
    kt = eng.kernel_times()
    assert kt['k_s2_bright'][1] >= 1 and 'k_s2_tile' in kt, sorted(kt)
    if not pmt_afterpulses:
        assert ('k_pulse_dense' in kt) <= bool((kind == 2).any()), sorted(kt)
