"""Noise-hit seeds of the lone-hit rows on the device (config 'noise_lone_hits', wfs_set_lone_noise_hits; MI355X only).

The rule is restated in numpy in tests/lone_noise.py (tests/test_lone_noise_cpu.py pins the restatement on the unchanged oracle).  The
device is held to it -- rows, both per-row counts, ix_rand, records -- on eight channels and stretches of 2^15 - 2^16 samples under a
model with almost all mass on 0 and 2^-9 on a value that crosses the threshold: designed seams found by a CPU scan of the restatement
(the finders of tests/lone_noise.py) and, against the rows of a run, supplied photons placed around isolated noise hits.  Every test
asserts with the restatement alone that it holds the seeds it is about: none can pass empty.
"""
import numpy as np
import pytest

import wfsim_amd
from tests import dark_counts as DK
from tests import lone_hits as LH
from tests import lone_noise as LN
from tests.helpers import make_engine, make_oracle
from tests.test_gpu_lone_hits import _assert_chunks, _ins, _run_rawdata, _run_rows
from tests.test_gpu_noise_model import _photon_sets
from tests.test_lone_noise_cpu import N_MODEL, REACH, SEED, SMALL, SPIKE, model_config, rates
from wfsim_amd.engine import WfsError

pytestmark = pytest.mark.gpu
CH = 5
SCAN = 1 << 16


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _ln_of(eng, cfg):
    model, seed = LN.model_of(cfg)
    p = eng.params
    lone = LH.Lone(DK.Dark.of_engine(eng), p['trigger_window'])
    return LN.LoneNoise(lone, model, seed, eng.tables['thr_zle'], p['baseline'], p['n_tpc'], photons=eng.dark_count_rate is not None)


def _rows_key(rows):
    return [(int(r['channel']), int(r['left']), int(r['right']), int(r['ix_rand']), int(r['n_photons'])) for r in rows]


def _assert_pass(eng, ln, s0, s1, s_limit, rows_of=None, channels=range(N_MODEL)):
    """one pass on the device against the restatement: the row listing with both counts, then the records byte for byte"""
    for ch in channels:
        ln.prime(ch, s0 - ln.G - ln.tlen - 8, s_limit + ln.tlen + 8)
    rec = eng.lone_hits(s0, s1, s_limit)
    got, got_nn = eng.lone_hit_rows(), eng.lone_hit_noise_seeds()
    exp = ln.pass_rows(channels, s0, s1, s_limit, rows_of)
    assert _rows_key(got) == _rows_key(exp), (s0, s1, s_limit)
    assert got_nn.tolist() == [r['n_noise'] for r in exp]
    want = ln.records(exp, eng.params['dt'])
    assert len(rec) == len(want) and rec.tobytes() == want.tobytes(), (s0, s1, s_limit, len(rec), len(want))
    return exp, rec


def _noise(exp, ch=None):
    return [r for r in exp if r['n_noise'] > 0 and (ch is None or r['channel'] == ch)]


@pytest.fixture(scope='module')
def both():
    """dark-count rates and the model, nothing run: every dark photon is lone, every crossing a seed"""
    cfg = model_config(dark_count_rate=rates())
    eng = make_engine(cfg)
    assert eng.noise_lone_hits is True and eng.lone_hits_on is True
    ln = _ln_of(eng, cfg)
    return eng, ln, LN.seed_table(ln, range(N_MODEL), 0, SCAN)


@pytest.fixture(scope='module')
def only():
    """the model without rates: a noise-only pass"""
    cfg = model_config()
    eng = make_engine(cfg)
    assert eng.noise_lone_hits is True and eng.dark_count_rate is None
    ln = _ln_of(eng, cfg)
    return eng, ln, LN.seed_table(ln, range(N_MODEL), 0, 8 * SCAN)


# ---------------------------------------------------------------------------------------------------- 1: passes against no rows
def test_a_stretch_of_every_kind_of_chain(both):
    """2^15 samples on eight channels: some hundred noise hits a channel (the crossing samples of the dark pulses among them), chains of
    noise hits alone, chains that mix photons and noise hits, a hit inside a lone photon's pulse, a hit only D and noise together make"""
    eng, ln, tab = both
    c_in, at_in = LN.find_inside_pulse(ln, tab)
    c_b, at_b = LN.find_needs_both(ln, tab)
    assert at_in < SCAN // 2 and at_b < SCAN // 2
    exp, rec = _assert_pass(eng, ln, 0, SCAN // 2, SCAN // 2 + REACH)
    for ch in range(N_MODEL):
        assert 60 <= sum(r['n_noise'] for r in exp if r['channel'] == ch) or ch == 6
    assert 40 <= sum(r['n_noise'] for r in exp if r['channel'] == 6) <= 130 and not any(r['n_photons'] for r in exp if r['channel'] == 6)
    assert sum(r['n_noise'] > 0 and r['n_photons'] > 0 for r in exp) > 50 and sum(r['n_photons'] == 0 for r in exp) > 100
    assert any(r['channel'] == c_in and at_in in r['starts'].tolist() and r['n_photons'] for r in exp)
    row = [r for r in exp if r['channel'] == c_b and at_b in r['starts'].tolist()][0]
    D, nz = int(ln.dark(c_b, at_b, 1)[0]), int(ln.noise(c_b, at_b, 1)[0])
    assert nz == -SMALL and -SMALL < D < 0 and row['n_noise'] >= 1
    assert len(rec) > 500


def test_hits_G_and_G_plus_1_apart_without_rates(only):
    """a noise-only pass (no dark-count rates: the photon scan is skipped, the rows are finished without D): two hits G apart are one
    row, G + 1 apart two"""
    eng, ln, tab = only
    G = ln.G
    ch, at = LN.find_pair(tab, G, 150)
    exp, _ = _assert_pass(eng, ln, at - 1000, at + 2000, at + 2000 + REACH)
    assert any(r['channel'] == ch and r['starts'].tolist() == [at, at + G] for r in exp) and not any(r['n_photons'] for r in exp)
    ch, at = LN.find_pair(tab, G + 1, 150)
    exp, _ = _assert_pass(eng, ln, at - 1000, at + 2000, at + 2000 + REACH)
    assert any(r['channel'] == ch and r['starts'].tolist() == [at] for r in exp) and any(r['channel'] == ch and r['starts'].tolist() == [at + G + 1] for r in exp)
    with pytest.raises(WfsError, match='no dark-count rates are set'):
        eng.dark_count_samples(0, 0, 10)


def test_ownership_at_the_ends_of_a_pass(both):
    """a hit at s0 - 1, s0, s1 - 1, s1; a chain that begins in front of s0 (not owned), one followed beyond s1, one cut by s_limit"""
    eng, ln, tab = both
    ch, S = LN.find_isolated(tab, 400)
    for s0, s1, owned in ((S + 1, S + 900, False), (S, S + 900, True), (S - 900, S, False), (S - 900, S + 1, True)):
        exp, _ = _assert_pass(eng, ln, s0, s1, s1 + 500)
        assert any(r['channel'] == ch and r['starts'][0] == S for r in exp) == owned, (s0, s1)
    ln.prime(ch, -1000, SCAN + REACH)
    chain = [r for r in ln.rows(ch, 0, SCAN, SCAN + REACH) if r['n_noise'] >= 1 and r['starts'][-1] - r['starts'][0] > 30 and r['starts'][0] > 2000][0]
    st = chain['starts']
    f, last = int(st[0]), int(st[-1])
    second = int(st[st > f][0])
    exp, _ = _assert_pass(eng, ln, second, second + 900, second + 1400)                     # begins in front of s0: not this pass's
    assert not any(r['channel'] == ch and r['left'] <= last <= r['right'] for r in exp)
    exp, _ = _assert_pass(eng, ln, f - 700, f + 1, last + 700)                              # runs beyond s1: owned and followed to its end
    assert any(r['channel'] == ch and r['starts'].tolist() == st.tolist() for r in exp)
    exp, _ = _assert_pass(eng, ln, f - 700, f + 1, second)                                  # cut by s_limit
    cut = [r for r in exp if r['channel'] == ch and r['starts'][0] == f][0]
    assert cut['starts'].max() < second and cut['right'] == min(second - 1, int(cut['starts'].max()) + ln.tlen - 1 + ln.tw) < chain['right']


def test_one_pass_is_three_passes(both):
    """cut inside a chain and one sample behind a chain's first seed: the same records"""
    eng, ln, tab = both
    a, n = 3000, 6000
    ln.prime(CH, a - 1000, a + n + REACH + 100)
    chains = [r for r in ln.rows(CH, a + 100, a + n - 100, a + n + REACH) if r['n_noise'] >= 1 and r['starts'][-1] - r['starts'][0] >= 2]
    assert len(chains) >= 2
    c1, c2 = int(chains[0]['starts'][0]) + 1, int(chains[-1]['starts'][-1])
    assert a < c1 < c2 < a + n
    whole = eng.lone_hits(a, a + n, a + n + REACH)
    parts = np.concatenate([eng.lone_hits(x, y, a + n + REACH) for x, y in ((a, c1), (c1, c2), (c2, a + n))])
    assert len(whole) > 100 and LH.sort_records(parts).tobytes() == LH.sort_records(whole).tobytes()


@pytest.mark.parametrize('s0', [-4321, -5, 2 ** 40 + 77, -2 ** 40 - 13])
def test_negative_and_large_samples(both, s0):
    eng, ln, tab = both
    exp, rec = _assert_pass(eng, ln, s0, s0 + 4000, s0 + 4500)
    assert len(_noise(exp)) >= 20 and len({r['left'] % 4 for r in exp}) == 4 and len(rec) >= 20


@pytest.mark.parametrize('pos', [0, 1, 254, 255])
def test_hits_at_the_edges_of_the_scan_blocks(both, only, pos):
    """the scan takes the samples from a0 = s0 - G on in blocks of 256: an isolated hit in the first and in the last sample of a block,
    as the last sample of the pass (taken) and as the first behind it (not taken), in a full and in a partial last block; and a hit in
    the first sample of the first block, which keeps the hit G behind it from beginning a row"""
    eng, ln, tab = both
    ch, S = LN.find_isolated(tab, 400, skip=1)
    a0 = S - 512 - pos
    assert (S - a0) % 256 == pos
    s0 = a0 + ln.G
    exp, _ = _assert_pass(eng, ln, s0, S + 1, S + 1)                    # the last sample of the last block's used part
    mine = [r for r in exp if r['channel'] == ch and r['starts'][0] == S]
    assert len(mine) == 1 and mine[0]['right'] == S
    exp, _ = _assert_pass(eng, ln, s0, S, S)                            # ... one behind it
    assert not any(r['channel'] == ch and S in r['starts'].tolist() for r in exp)
    exp, _ = _assert_pass(eng, ln, s0, S + 1, a0 + 1024)                # whole blocks
    assert any(r['channel'] == ch and r['starts'][0] == S for r in exp)
    if pos in (0, 255):
        eng2, ln2, tab2 = only
        G = ln.G
        c2, P = LN.find_pair(tab2, G, 150)
        if pos == 0:        # a0 = P: the pair's first hit is the first sample of the first block, and the second, at s0, begins no row
            exp, _ = _assert_pass(eng2, ln2, P + G, P + G + 300, P + G + 800)
            assert not any(r['channel'] == c2 and P + G in r['starts'].tolist() for r in exp)
        else:               # the first hit in the last sample of the first block: owned, one row with the second
            exp, _ = _assert_pass(eng2, ln2, P - 255 + G, P + G + 300, P + G + 800)
            assert any(r['channel'] == c2 and r['starts'].tolist() == [P, P + G] for r in exp)


# ---------------------------------------------------------------------------------------------------- 2: records against the oracle
def test_records_are_the_oracles(both):
    """the device's own rows, photons, D and noise (Engine.lone_hit_rows, dark_count_photons, dark_count_samples, noise_samples) on the
    unchanged oracle: the records of a channel byte for byte"""
    eng, ln, tab = both
    p = eng.params
    a, n = 5000, 5000
    rec = eng.lone_hits(a, a + n, a + n + REACH)
    rows, nn = eng.lone_hit_rows(), eng.lone_hit_noise_seeds()
    sel = rows['channel'] == CH
    assert sel.sum() >= 8 and nn[sel].sum() >= 8 and rows['n_photons'][sel].sum() >= 3
    fed = []
    for r in rows[sel]:
        first, last = int(r['left']) + p['trigger_window'], int(r['right']) - p['trigger_window'] - p['tlen'] + 1       # (no row in the way: not clipped)
        t, g = eng.dark_count_photons(CH, first + p['samples_before'], last - first + 1)
        st = t // p['dt'] - p['samples_before']
        starts = np.concatenate([st, [first, last]]).astype(np.int64)
        kinds = np.concatenate([np.full(len(st), LN.PHOTON), [LN.NOISE, LN.NOISE]]).astype(np.int64)
        o = np.lexsort((kinds, starts))
        # (a gain-0 call at either end spans the row where no photon does; photons sort in front of them at one start)
        fed.append(dict(channel=CH, left=int(r['left']), right=int(r['right']), starts=starts[o], kinds=kinds[o], t_ns=t, gain=g))
    cfg = model_config(dark_count_rate=rates())
    off = {k: v for k, v in cfg.items() if k not in ('noise_model', 'noise_lone_hits', 'dark_count_rate')}
    orc_of = lambda table: make_oracle(dict(off, enable_noise=False) if table is None else dict(off, enable_noise=True, noise_data=table))
    theirs = LN.oracle_records(orc_of, fed, ln, p, noise_of=lambda ch, t0, k: eng.noise_samples(ch, t0, k).astype(np.int64),
                               dark_of=lambda ch, t0, k: eng.dark_count_samples(ch, t0, k).astype(np.int64))
    mine = rec[rec['channel'] == CH]
    assert len(mine) >= 8 and mine.tobytes() == theirs.tobytes()


# ---------------------------------------------------------------------------------------------------- 3: passes against the rows of a run
def _seam_case(full):
    """five windows of supplied photons, 12000 samples apart, the first four placed around a noise hit of channel 5 at S with no other seed within G of it: the
    row of channel 5 begins at S + 1 (the hit at row_lo - 1: a seed, its row clipped), at S (row_lo: no seed), ends at S (row_hi: no
    seed), at S - 1 (row_hi + 1: a seed, clipped on the left); the fifth is 1700 samples long on channel 3 alone, so that the other
    channels' hits inside it are seeds, and none is under full readout"""
    cfg = model_config(dark_count_rate=rates(), full_readout=full)
    probe = make_engine(cfg)
    ln = _ln_of(probe, cfg)
    p = probe.params
    dt, tw = p['dt'], p['trigger_window']
    lead, tail = p['store_before'] + p['samples_before'] + tw, p['store_after'] + p['samples_after'] + tw
    tab = LN.seed_table(ln, [CH], 10000, 62000)
    st, kd = tab[CH]
    S = []
    for k in range(1, 5):
        lo, hi = 12000 * k + 1500, 12000 * k + 9000
        iso = [int(s) for j, s in enumerate(st.tolist()) if lo <= s < hi and kd[j] == LN.NOISE and 0 < j < len(st) - 1 and s - st[j - 1] > ln.G + 8 and st[j + 1] - s > ln.G + 8]
        S.append(iso[0])
    idx = [S[0] + 1 + lead, S[1] + lead, S[2] - tail, S[3] - 1 - tail]
    windows = [(dt * i, [(CH, [0], 1.0), (3, [5 * dt], 1.0)]) for i in idx]
    windows.append((dt * 64000, [(3, [0, 800 * dt, 1500 * dt], 1.0)]))
    sets, _ = _photon_sets(windows, np.asarray(cfg['gains'], dtype=np.float64))
    probe.set_debug(True)
    probe.load_photons(*sets)
    probe.run()
    rows_of, ranges = _run_rows(probe, full)
    return probe, ln, S, rows_of, ranges


def test_seams_against_the_rows_of_a_run():
    eng, ln, S, rows_of, ranges = _seam_case(False)
    mine = sorted(rows_of[CH])
    assert len(mine) == 4 and len(ranges) == 5
    assert mine[0][0] == S[0] + 1 and mine[1][0] == S[1] and mine[2][1] == S[2] and mine[3][1] == S[3] - 1
    exp, rec = _assert_pass(eng, ln, 11000, 68000, 69000, rows_of)
    five = {int(r['starts'][0]): r for r in exp if r['channel'] == CH}
    assert five[S[0]]['right'] == S[0] == mine[0][0] - 1 and five[S[0]]['n_noise'] >= 1         # clipped in front of the row
    assert five[S[3]]['left'] == S[3] == mine[3][1] + 1                                         # clipped behind the row: the seed starts at its sample
    assert not any(S[1] in r['starts'].tolist() or S[2] in r['starts'].tolist() for r in exp if r['channel'] == CH)
    # a channel of a window without a row of its own: its hits inside the window are seeds
    inside = [r for r in _noise(exp) if r['channel'] != 3 and any(a <= s <= b for a, b in ranges for s in r['starts'][r['kinds'] == LN.NOISE].tolist())]
    assert len(inside) >= 3 and len({r['channel'] for r in inside}) >= 2
    assert len(rec) > 300


def test_full_readout_leaves_no_seed_inside_a_window():
    eng, ln, S, rows_of, ranges = _seam_case(True)
    assert len(ranges) == 5 and all(rows_of[ch] == ranges for ch in range(N_MODEL))
    exp, rec = _assert_pass(eng, ln, 11000, 68000, 69000, rows_of)
    assert len(_noise(exp)) > 100 and not any(a <= s <= b for r in exp for s in r['starts'].tolist() for a, b in ranges)
    assert sum(len(ln.crossings(ch, ranges[-1][0], ranges[-1][1] + 1)) for ch in range(N_MODEL) if ch != 3) >= 3     # hits the plain run read out as seeds


def test_every_crossing_is_read_out():
    """completeness on the mixed case with a run in the middle: every sample of a model channel in the scanned stretch whose value --
    Engine.noise_samples, Engine.dark_count_samples, baseline, clamp, on the host -- lies below the channel's threshold is inside a
    record of that channel, a window record or a lone record; s_limit = s1 cuts nothing that is asked for (samples behind it are not).
    The pass begins 2000 samples in front of the stretch that is checked, and every channel is quiet for more than G samples somewhere
    in between (asserted): no chain that reaches the stretch began in front of the pass"""
    eng, ln, S, rows_of, ranges = _seam_case(False)
    p = eng.params
    s0, s1, ahead = 11000, 68000, 2000
    win = eng.records()
    lone = eng.lone_hits(s0 - ahead, s1, s1)
    rec = np.concatenate([win, lone])
    n_cross = 0
    for ch in range(N_MODEL):
        v = np.maximum(eng.noise_samples(ch, s0 - ahead, s1 - s0 + ahead).astype(np.int64) + eng.dark_count_samples(ch, s0 - ahead, s1 - s0 + ahead) + p['baseline'], 0)
        cross = s0 - ahead + np.flatnonzero(v < int(eng.tables['thr_zle'][ch]))
        early = np.concatenate([[s0 - ahead - 1], cross[cross < s0], [s0]])
        assert np.diff(early).max() > ln.G + 1, 'a chain may run from in front of the pass into the stretch'
        cross = cross[cross >= s0]
        covered = np.zeros(s1 - s0, dtype=bool)
        r = rec[rec['channel'] == ch]
        for t, n in zip((r['time'] // p['dt']).tolist(), r['length'].tolist()):
            covered[max(t - s0, 0):max(t - s0 + n, 0)] = True
        missed = [int(t) for t in cross if not covered[t - s0]]
        assert not missed, (ch, missed[:10])
        n_cross += len(cross)
    assert n_cross > 2000 and len(win) > 0 and len(lone) > 300


def test_a_pass_leaves_the_batch_alone():
    eng, ln, S, rows_of, ranges = _seam_case(False)
    before, counts = eng.records().tobytes(), dict(eng.counts)
    eng.lone_hits(11000, 68000, 69000)
    assert eng.records().tobytes() == before and len(before) > 0
    eng.run()
    assert eng.records().tobytes() == before and eng.counts == counts


# ---------------------------------------------------------------------------------------------------- 4: coloured and slow models
def test_common_stream_hits_every_channel_of_its_group():
    """kind 4: the channels' own distributions are all 0; a common stream with the spike reaches channels 0 - 3 with gain 1: one draw
    puts a hit on every channel of the group at the same sample and on no channel outside it"""
    pmf, vmin = LN.spike_pmf(N_MODEL, SPIKE, p_spike=0.0)
    cpmf, _ = LN.spike_pmf(1, SPIKE)
    group = np.array([0, 0, 0, 0, -1, -1, -1, -1])
    cfg = model_config()
    cfg['noise_model'] = dict(pmf=pmf, vmin=vmin, common=dict(groups=group, gain=1.0, pmf=cpmf))
    eng = make_engine(cfg)
    assert 'k_lone_noise_scan' not in eng.kernel_times()
    ln = _ln_of(eng, cfg)
    eng.set_profiling(True)
    exp, rec = _assert_pass(eng, ln, 0, SCAN // 2, SCAN // 2 + REACH)
    assert 'k_lone_noise_scan' in eng.kernel_times() and 'k_lone_scan' not in eng.kernel_times()
    eng.set_profiling(False)
    seeds = {ch: sorted(int(s) for r in exp if r['channel'] == ch for s in r['starts']) for ch in range(N_MODEL)}
    assert 40 <= len(seeds[0]) <= 130 and seeds[0] == seeds[1] == seeds[2] == seeds[3] and not any(seeds[ch] for ch in range(4, N_MODEL))
    assert set(rec['channel'].tolist()) == {0, 1, 2, 3}


def test_slow_level_makes_long_chains():
    """kind 5: a knot of the spike value pulls the baseline across the threshold for a stretch of the level's period: one long chain"""
    from tests.test_gpu_noise_slow import _slow
    cfg = model_config(dark_count_rate=rates())
    cfg['noise_model'] = dict(cfg['noise_model'], slow=_slow(N_MODEL, (4, 6)))
    eng = make_engine(cfg)
    ln = _ln_of(eng, cfg)
    exp, rec = _assert_pass(eng, ln, -2000, SCAN // 2, SCAN // 2 + REACH)

    def longest_run(r):         # consecutive samples that cross: a dark pulse makes a handful, a spike of the pmf one
        t = np.unique(r['starts'][r['kinds'] == LN.NOISE])
        return int(np.diff(np.concatenate([[-1], np.flatnonzero(np.diff(t) > 1), [len(t) - 1]])).max()) if len(t) else 0
    runs = [r for r in exp if longest_run(r) >= 12]
    assert len(runs) >= 3 and len({r['channel'] for r in runs}) >= 2 and max(longest_run(r) for r in runs) >= 40


# ---------------------------------------------------------------------------------------------------- 5: the setter
def test_errors_and_the_switch():
    from wfsim_amd.config import xenonnt_test_config
    from tests.helpers import with_fma
    eng = make_engine(with_fma(xenonnt_test_config(seed=3), False))                 # the recorded noise table
    assert eng.noise_lone_hits is False and eng.lone_hits_on is False
    with pytest.raises(WfsError, match='libwfsim_amd error -4: wfs_set_lone_noise_hits: no drawn noise model is set'):
        eng.set_lone_noise_hits(True)
    eng.set_lone_noise_hits(False)
    eng = make_engine(with_fma(xenonnt_test_config(seed=3, enable_noise=False), False))
    pmf, vmin = LN.spike_pmf(N_MODEL, SPIKE)
    eng.set_noise_model(pmf, vmin)
    with pytest.raises(WfsError, match='wfs_set_lone_noise_hits: enable_noise is off'):
        eng.set_lone_noise_hits(True)
    cfg = model_config()
    del cfg['noise_lone_hits']
    eng = make_engine(cfg)
    assert eng.noise_lone_hits is False and eng.lone_hits_on is False
    with pytest.raises(WfsError, match='wfs_lone_hits: no dark-count rates are set'):
        eng.lone_hits(0, 100)
    eng.set_lone_noise_hits(True)
    assert len(eng.lone_hits(0, 8000)) > 5 and eng.lone_hit_noise_seeds().sum() > 5 and len(eng.lone_hit_noise_seeds()) == len(eng.lone_hit_rows())
    with pytest.raises(WfsError, match='wfs_lone_hits: s1 < s0'):
        eng.lone_hits(10, 9)
    assert len(eng.lone_hits(7, 7)) == 0 and len(eng.lone_hit_noise_seeds()) == 0
    eng.set_noise_model(None)                                                       # clearing the model switches the seeds off
    assert eng.noise_lone_hits is False
    with pytest.raises(WfsError, match='wfs_lone_hits: no dark-count rates are set'):
        eng.lone_hits(0, 100)
    with pytest.raises(ValueError, match="noise_lone_hits: needs config\\['noise_model'\\]"):
        make_engine(with_fma(xenonnt_test_config(seed=3, noise_lone_hits=True), False))
    with pytest.raises(ValueError, match='noise_lone_hits: right_raw_extension 3000 ns below'):
        make_engine(dict(model_config(), right_raw_extension=3000))


def test_dark_lone_hits_alone_are_what_they_were(both):
    """the switch off on an engine with rates and a model: the rows of DESIGN 3f, no noise-hit seed, a noise count of 0 in every row"""
    eng, ln, tab = both
    eng.set_lone_noise_hits(False)
    try:
        rec = eng.lone_hits(0, 8000, 8000 + REACH)
        rows = eng.lone_hit_rows()
        exp = ln.lone.pass_rows(range(N_MODEL), 0, 8000, 8000 + REACH)
        assert _rows_key(rows) == _rows_key(exp) and len(exp) > 50 and not eng.lone_hit_noise_seeds().any() and len(rec) > 50
    finally:
        eng.set_lone_noise_hits(True)


# ---------------------------------------------------------------------------------------------------- 6: above the engine
MS = 1_000_000
TIMES = [MS + 130_000 * k for k in range(9)]


def _rawdata_cfg(**kw):
    from wfsim_amd.config import xenonnt_test_config
    pmf, vmin = LN.spike_pmf(N_MODEL, SPIKE)
    return xenonnt_test_config(seed=SEED + 2, enable_noise=True, noise_model=dict(pmf=pmf, vmin=vmin), **kw)


def test_rawdata_batches_and_the_key():
    """key absent == key False: no entry, the same bytes; one batch == small batches; the window records do not depend on the key;
    iter_windows yields the lone entries between the windows"""
    mixed = _ins(TIMES[:5], s2=True)
    off_rd, off_b, off_win, off_lone = _run_rawdata(_rawdata_cfg(), mixed)
    no_rd, no_b, no_win, no_lone = _run_rawdata(_rawdata_cfg(noise_lone_hits=False), mixed)
    assert off_lone is None and no_lone is None and no_win.tobytes() == off_win.tobytes() and len(off_win) > 100
    assert all(set(a) == set(b) and 'lone_records' not in a for a, b in zip(off_b, no_b))
    assert off_rd.engine.lone_hits_on is False and no_rd.engine.noise_lone_hits is False
    ins = _ins(TIMES)
    _, _, off_win, _ = _run_rawdata(_rawdata_cfg(), ins)
    one_rd, one_b, one_win, one_lone = _run_rawdata(_rawdata_cfg(noise_lone_hits=True), ins)
    few_rd, few_b, few_win, few_lone = _run_rawdata(_rawdata_cfg(noise_lone_hits=True), ins, quanta=100)
    assert len(one_b) == 1 and len(one_b[0]['left']) == len(TIMES) and len(few_b) >= 3
    assert one_win.tobytes() == off_win.tobytes() and few_win.tobytes() == off_win.tobytes()
    assert len(one_lone) > 100 and LH.sort_records(few_lone).tobytes() == LH.sort_records(one_lone).tobytes()
    assert set(one_lone['channel'].tolist()) == set(range(N_MODEL))
    left, right = int(one_b[0]['left'][0]), int(one_b[0]['right'][-1])
    rext, dt = 100000, 10
    direct = one_rd.engine.lone_hits(left - rext // dt, right + 1 + rext // dt)
    assert LH.sort_records(direct).tobytes() == LH.sort_records(one_lone).tobytes()
    both_rd, _, both_win, both_lone = _run_rawdata(_rawdata_cfg(noise_lone_hits=True, dark_count_lone_hits=True, dark_count_rate=np.full(N_MODEL, 4e4)), ins)
    dark_rd, _, dark_win, dark_lone = _run_rawdata(_rawdata_cfg(dark_count_lone_hits=True, dark_count_rate=np.full(N_MODEL, 4e4)), ins)
    assert both_win.tobytes() == dark_win.tobytes() and len(both_lone) > len(dark_lone) > 100 and dark_rd.engine.noise_lone_hits is False
    rd = wfsim_amd.RawData(_rawdata_cfg(noise_lone_hits=True))
    entries = list(rd.iter_windows(ins))
    lone_e = [e for e in entries if e.get('lone')]
    assert rd.source_finished and len(lone_e) > 50 and len(entries) - len(lone_e) == len(TIMES)
    assert all(a['left'] <= b['left'] for a, b in zip(entries[:-1], entries[1:]))
    assert LH.sort_records(np.concatenate([e['records'] for e in lone_e])).tobytes() == LH.sort_records(one_lone).tobytes()


def test_chunker_merges_lone_records():
    """every record inside its chunk, records time sorted, no overlap within a channel, the chunks hold the window records and every
    lone record exactly once"""
    cfg = _rawdata_cfg(noise_lone_hits=True, chunk_size=0.0004)
    ins = _ins(TIMES)
    sim = wfsim_amd.ChunkRawRecords(cfg)
    chunks, bounds = [], []
    for c in sim(ins):
        chunks.append(c)
        bounds.append((sim.chunk_time_pre, sim.chunk_time))
    assert len(chunks) >= 3
    _, _, win, lone = _run_rawdata(dict(cfg, lone_hits_begin=bounds[0][0] + 50 * 10), ins)
    _assert_chunks(chunks, bounds, win, lone)
    assert len(lone) > 100 and sum(len(c['raw_records']) > 0 for c in chunks) >= 3
    off = np.concatenate([c['raw_records'] for c in wfsim_amd.ChunkRawRecords(_rawdata_cfg(chunk_size=0.0004))(ins)])
    assert LH.sort_records(off).tobytes() == LH.sort_records(win).tobytes()
