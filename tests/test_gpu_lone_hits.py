"""Lone-hit rows on the device (config 'dark_count_lone_hits', wfs_lone_hits; MI355X only).

The rule is restated in numpy in tests/lone_hits.py (tests/test_lone_hits_cpu.py pins the restatement on the unchanged oracle).  The
device is held to it on designed seams: rows, photon counts, ix_rand and records of a pass against the rows of a run whose supplied
photons were placed around known dark photons, ownership at the ends of a pass, chains across them, negative and large cells,
per-channel SPE rows, every noise kind; to the oracle directly with the device's own photons; and above the engine through RawData,
RawDataOptical and ChunkRawRecords.  Every test asserts with the restatement alone that the seam it is about occurs.
"""
import numpy as np
import pytest

import wfsim_amd
from tests import dark_counts as DK
from tests import lone_hits as LH
from tests import spe_channels as SC
from tests.helpers import make_engine, make_oracle, with_fma
from tests.test_gpu_noise_model import _engine_photons, _instructions, _photon_sets
from tests.test_lone_hits_cpu import AT, NEAR_LIMIT, REACH, SEED, STRETCHES
from wfsim_amd import dark_counts as DC
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype
from wfsim_amd.engine import WfsError

pytestmark = pytest.mark.gpu
MS = 1_000_000
CH = 5                          # the channel of the designed photons
N_RATES = 8                     # channels 0 .. 7 have a rate; 6 has rate 0 and 7 (SC.DEAD_CH) gain 0: lone rows on six channels


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _rates(n=N_RATES, dt=10):
    r = np.full(n, NEAR_LIMIT * DC.max_rate(dt))
    r[6] = 0.0
    return r


def _base(**kw):
    """per-channel SPE rows (the 'shaped' family of spe_channels.npz), non-uniform gains"""
    return dict(with_fma(SC.config('shaped', seed=SEED), False), dark_count_rate=_rates(), **kw)


def _lone_of(eng, noise_len=0):
    return LH.Lone(DK.Dark.of_engine(eng), eng.params['trigger_window'], noise_len)


def _rows_key(rows):
    return [(int(r['channel']), int(r['left']), int(r['right']), int(r['ix_rand']), int(r['n_photons'])) for r in rows]


def _expected_records(eng, lone, exp, noise_of=None, float_noise=False):
    p = eng.params
    data = [LH.finish(lone.term(r), p['baseline'], None if noise_of is None else noise_of(r), float_noise) for r in exp]
    return LH.records_of_rows(exp, data, lambda ch: int(eng.tables['thr_zle'][ch]), p['trigger_window'], p['dt'])


def _assert_pass(eng, lone, s0, s1, s_limit, rows_of=None, noise_of=None, float_noise=False):
    """one pass on the device against the restatement: the row listing, then the records byte for byte; returns the restated rows"""
    rec = eng.lone_hits(s0, s1, s_limit)
    got = eng.lone_hit_rows()
    exp = lone.pass_rows(range(N_RATES), s0, s1, s_limit, rows_of)
    assert _rows_key(got) == _rows_key(exp), (s0, s1, s_limit)
    want = _expected_records(eng, lone, exp, noise_of, float_noise)
    assert len(rec) == len(want) and rec.tobytes() == want.tobytes(), (s0, s1, s_limit, len(rec), len(want))
    return exp, rec


@pytest.fixture(scope='module')
def bare():
    """an engine that has run nothing: every dark photon is lone"""
    eng = make_engine(_base(enable_noise=False))
    assert eng.tables['spe'].shape[0] == 494 and eng.lone_hits_on is False
    return eng, _lone_of(eng)


# ---------------------------------------------------------------------------------------------------- 1: passes against no rows
def test_designed_stretches(bare):
    """the stretches of the CPU pin on channel 5: a cell of four photons, chains of two and three, a pair G apart (one row) and
    G + 1 apart (two rows)"""
    eng, lone = bare
    seen = set()
    for name in ('four', 'gap_G_5', 'gap_G1_5'):
        ch, a, n = STRETCHES[name]
        exp, rec = _assert_pass(eng, lone, a, a + n, a + n + REACH)
        mine = [r for r in exp if r['channel'] == CH]
        seen |= {r['n_photons'] for r in mine}
        if name == 'four':
            assert any(np.sum((r['starts'] + lone.before) >> 6 == 1354) == 4 for r in mine)
        elif name == 'gap_G_5':
            assert any(AT[name] in r['starts'].tolist() and AT[name] + lone.G in r['starts'].tolist() for r in mine)
        else:
            assert any(r['starts'][-1] == AT[name] for r in mine) and any(r['starts'][0] == AT[name] + lone.G + 1 for r in mine)
        assert len(rec) >= 10 and not np.any(rec['channel'] == 6) and len(set(rec['channel'].tolist())) >= 5
    assert {1, 2, 3} <= seen


def test_ownership_at_the_ends_of_a_pass(bare):
    """start at s0 - 1, s0, s1 - 1, s1; a chain that begins in front of s0 (not owned), one that runs beyond s1 (owned, followed), one
    that s_limit cuts"""
    eng, lone = bare
    a = STRETCHES['gap_G_5'][1]
    rows = lone.rows(CH, a, a + 3000, a + 3000 + REACH)
    single = [r for r in rows if r['n_photons'] == 1][0]
    S = int(single['starts'][0])
    for s0, s1, owned in ((S + 1, S + 900, False), (S, S + 900, True), (S - 900, S, False), (S - 900, S + 1, True)):
        exp, _ = _assert_pass(eng, lone, s0, s1, s1 + 500)
        assert any(r['channel'] == CH and r['starts'][0] == S for r in exp) == owned, (s0, s1)
    chain = [r for r in rows if r['n_photons'] >= 2][0]
    f, second, last = int(chain['starts'][0]), int(chain['starts'][1]), int(chain['starts'][-1])
    exp, _ = _assert_pass(eng, lone, second, second + 900, second + 1400)                   # begins in front of s0: no pass of this kind owns it
    assert not any(r['channel'] == CH and r['left'] <= last <= r['right'] for r in exp)
    exp, _ = _assert_pass(eng, lone, f - 700, f + 1, last + 700)                            # runs beyond s1: owned and followed to its end
    assert any(r['channel'] == CH and r['starts'].tolist() == chain['starts'].tolist() for r in exp)
    exp, _ = _assert_pass(eng, lone, f - 700, f + 1, second)                                # cut by s_limit
    cut = [r for r in exp if r['channel'] == CH and r['starts'][0] == f][0]
    assert cut['n_photons'] == 1 and cut['right'] == min(second - 1, f + lone.tlen - 1 + lone.tw) < chain['right']


def test_one_pass_is_three_passes(bare):
    """cut inside a chain and one sample behind a chain's first photon: the same records"""
    eng, lone = bare
    a, n = STRETCHES['gap_G_5'][1], 3000
    chains = [r for r in lone.rows(CH, a, a + n, a + n + REACH) if r['n_photons'] >= 2]
    assert len(chains) >= 2
    c1, c2 = int(chains[0]['starts'][0]) + 1, int((chains[-1]['starts'][0] + chains[-1]['starts'][1]) // 2)
    assert a < c1 < c2 < a + n and chains[-1]['starts'][0] < c2 <= chains[-1]['starts'][1]
    whole = eng.lone_hits(a, a + n, a + n + REACH)
    parts = np.concatenate([eng.lone_hits(x, y, a + n + REACH) for x, y in ((a, c1), (c1, c2), (c2, a + n))])
    assert len(whole) > 20 and LH.sort_records(parts).tobytes() == LH.sort_records(whole).tobytes()


@pytest.mark.parametrize('s0', [-64 * 3000 - 1, -5, 2 ** 40 + 77, -2 ** 40 - 13])
def test_negative_and_large_cells(bare, s0):
    eng, lone = bare
    exp, rec = _assert_pass(eng, lone, s0, s0 + 4000, s0 + 4500)
    assert len(exp) >= 10 and len(rec) >= 5


@pytest.mark.parametrize('cells', [255, 256, 257, 512])
def test_scan_ranges_around_the_block_size(bare, cells):
    """the scan takes 256 cells of a channel per workgroup: ranges of one cell less, exactly that, one more, two blocks"""
    eng, lone = bare
    p = eng.params
    a0 = 64 * 7000 - p['samples_before']                    # the first scanned start opens a cell
    s0, s_limit = a0 + lone.G, a0 + 64 * cells
    assert ((s_limit - 1 + p['samples_before']) >> 6) - ((a0 + p['samples_before']) >> 6) + 1 == cells
    s1 = max(s0, s_limit - 10)
    exp, _ = _assert_pass(eng, lone, s0, s1, s_limit)
    assert cells < 255 or len(exp) >= 20


def test_no_rows_where_no_photon_is_due():
    """rate 0 between two channels with a rate, gain 0, an SPE row of zeros (photons of gain 0: rows, flat ones), channels beyond the rates"""
    cfg = dict(with_fma(SC.config('shaped', seed=SEED), False), enable_noise=False)
    rates = np.zeros(max(SC.DEAD_CH, SC.ZERO_CH) + 1)
    rates[[5, SC.DEAD_CH, SC.ZERO_CH]] = NEAR_LIMIT * DC.max_rate(10)
    eng = make_engine(dict(cfg, dark_count_rate=rates))
    lone = _lone_of(eng)
    rec = eng.lone_hits(0, 20000, 20000)
    rows = eng.lone_hit_rows()
    exp = [r for ch in (5, SC.DEAD_CH, SC.ZERO_CH) for r in lone.rows(ch, 0, 20000, 20000)]
    assert _rows_key(rows) == _rows_key(sorted(exp, key=lambda r: (r['channel'], r['left'])))
    assert set(rows['channel'].tolist()) == {5, SC.ZERO_CH} and set(rec['channel'].tolist()) == {5}


def test_errors_and_off():
    eng = make_engine(with_fma(xenonnt_test_config(seed=3), False))
    assert eng.lone_hits_on is False
    with pytest.raises(WfsError, match='libwfsim_amd error -4: wfs_lone_hits: no dark-count rates are set'):         # WFS_E_STATE
        eng.lone_hits(0, 100)
    eng.set_dark_counts(100.0)
    with pytest.raises(WfsError, match='wfs_lone_hits: s1 < s0'):
        eng.lone_hits(10, 9)
    with pytest.raises(WfsError, match='wfs_lone_hits: s_limit < s1'):
        eng.lone_hits(0, 10, 9)
    with pytest.raises(WfsError, match='lone hits: a pass of more than 2\\^34 cells'):
        eng.lone_hits(0, 2 ** 32)
    assert len(eng.lone_hits(7, 7)) == 0 and len(eng.lone_hit_rows()) == 0
    with pytest.raises(ValueError, match='dark_count_lone_hits: needs'):
        make_engine(with_fma(xenonnt_test_config(seed=3, dark_count_lone_hits=True), False))
    with pytest.raises(ValueError, match='right_raw_extension 3000 ns below'):
        make_engine(with_fma(xenonnt_test_config(seed=3, dark_count_lone_hits=True, dark_count_rate=40.0, right_raw_extension=3000), False))


# ---------------------------------------------------------------------------------------------------- 2: records against the oracle
@pytest.mark.parametrize('name', sorted(STRETCHES))
def test_records_are_the_oracles(name):
    """the stretches and Pulse calls of the CPU pin with the device's own photons (Engine.dark_count_photons), noise off"""
    cfg = with_fma(xenonnt_test_config(seed=SEED, enable_noise=False), False)
    rates = np.full(300, NEAR_LIMIT * DC.max_rate(10))
    rates[6] = 0.0
    eng = make_engine(dict(cfg, dark_count_rate=rates))
    p = eng.params
    ch, a, n = STRETCHES[name]
    rec = eng.lone_hits(a, a + n, a + n + REACH)
    rows = eng.lone_hit_rows()
    rows = rows[rows['channel'] == ch]
    assert len(rows) >= 3 and len(set(eng.lone_hit_rows()['channel'].tolist())) > 200
    fed = []
    for r in rows:
        first, last = int(r['left']) + p['trigger_window'], int(r['right']) - p['trigger_window'] - p['tlen'] + 1       # (no row in the way: not clipped)
        t, g = eng.dark_count_photons(ch, first + p['samples_before'], last - first + 1)
        assert len(t) == r['n_photons'] and t[0] // p['dt'] - p['samples_before'] == first and t[-1] // p['dt'] - p['samples_before'] == last
        fed.append(dict(channel=ch, left=int(r['left']), t_ns=t, gain=g))
    theirs = LH.oracle_records(make_oracle(cfg), fed, p['n_tpc'], p['samples_before'], p['dt'])
    mine = rec[rec['channel'] == ch]
    assert len(mine) >= 3 and mine.tobytes() == theirs.tobytes()


# ---------------------------------------------------------------------------------------------------- 3: passes against the rows of a run
def _isolated(lone, ch, lo, hi, clear=400):
    """the first photon of ch that starts in [lo, hi) with no other photon of ch within `clear` samples"""
    st, _, _ = lone.photons(ch, lo - clear, hi + clear)
    for k, s in enumerate(st.tolist()):
        if lo <= s < hi and all(abs(s - o) > clear for j, o in enumerate(st.tolist()) if j != k):
            return s
    raise AssertionError('no isolated photon')


def _seam_windows(lone, p):
    """five windows of supplied photons, 20000 samples apart, each placed around an isolated dark photon of channel 5 that starts at S:
    the row of channel 5 begins at S + tlen (the pulse ends one sample in front of it: lone, clipped), at S + tlen - 1 (not lone), ends
    at S (not lone), at S - 1 (lone, clipped on the left); the fifth is 1700 samples long on channel 3 alone, so that the other
    channels' photons inside it are lone.  Returns (windows for _photon_sets, the four S)."""
    dt, tw, tlen = p['dt'], p['trigger_window'], p['tlen']
    lead = p['store_before'] + p['samples_before'] + tw                    # a row begins this far in front of its first photon's sample
    tail = p['store_after'] + p['samples_after'] + tw                      # ... and ends this far behind its last photon's
    S = [_isolated(lone, CH, 20000 * k + 2000, 20000 * k + 12000) for k in range(1, 5)]
    idx = [S[0] + tlen + lead, S[1] + tlen - 1 + lead, S[2] - tail, S[3] - 1 - tail]
    windows = [(dt * i, [(CH, [0], 1.0), (3, [5 * dt], 1.0)]) for i in idx]
    windows.append((dt * 110000, [(3, [0, 800 * dt, 1500 * dt], 1.0)]))
    return windows, S


def _run_rows(eng, full):
    """{channel: [(l, r)]} of the final rows of the engine's last run (debug copy of the rows with pulses; under full readout every
    channel of a window has the range the listed rows have), and the windows' ranges"""
    g, r = eng.groups(), eng.rows()
    out, ranges = {}, {}
    for k in range(len(r['channel'])):
        grp = int(r['group'][k])
        l, rr = int(g['left'][grp]) + int(r['left'][k]), int(g['left'][grp]) + int(r['right'][k])
        ranges.setdefault(grp, (l, rr))
        if full:
            assert ranges[grp] == (l, rr)
        elif int(r['channel'][k]) < N_RATES:
            out.setdefault(int(r['channel'][k]), []).append((l, rr))
    if full:
        out = {ch: sorted(ranges.values()) for ch in range(N_RATES)}
    return out, sorted(ranges.values())


def _seam_case(full, **noise):
    cfg = _base(full_readout=full, **(noise or dict(enable_noise=False)))
    probe = make_engine(cfg)
    lone = _lone_of(probe, len(cfg['noise_data']) if 'noise_data' in cfg else 0)
    windows, S = _seam_windows(lone, probe.params)
    sets, _ = _photon_sets(windows, np.asarray(cfg['gains'], dtype=np.float64))
    eng = make_engine(cfg)
    eng.set_debug(True)
    eng.load_photons(*sets)
    eng.run()
    rows_of, ranges = _run_rows(eng, full)
    return eng, lone, S, rows_of, ranges


def test_seams_against_the_rows_of_a_run():
    eng, lone, S, rows_of, ranges = _seam_case(False)
    tlen, tw = lone.tlen, lone.tw
    mine = sorted(rows_of[CH])
    assert len(mine) == 4 and len(ranges) == 5
    assert mine[0][0] == S[0] + tlen and mine[1][0] == S[1] + tlen - 1 and mine[2][1] == S[2] and mine[3][1] == S[3] - 1
    assert lone.is_lone(S[0], mine) and not lone.is_lone(S[1], mine) and not lone.is_lone(S[2], mine) and lone.is_lone(S[3], mine)
    exp, rec = _assert_pass(eng, lone, 15000, 115000, 116000, rows_of)
    five = {int(r['starts'][0]): r for r in exp if r['channel'] == CH}
    assert five[S[0]]['right'] == mine[0][0] - 1 < S[0] + tlen - 1 + tw             # clipped in front of the row
    assert five[S[3]]['left'] == mine[3][1] + 1 > S[3] - tw                         # clipped behind the row
    assert S[1] not in five and S[2] not in five
    # a channel of a window without a row of its own: lone inside the window
    inside = [r for r in exp if r['channel'] != 3 and any(a <= r['starts'][0] and r['starts'][-1] + tlen - 1 <= b for a, b in ranges)]
    assert len(inside) >= 3 and len({r['channel'] for r in inside}) >= 2
    # ... and the tail of a photon that is not lone shows in a lone row it reaches (every dark photon counts)
    assert len(rec) > 100


def test_full_readout_leaves_no_lone_photon_inside_a_window():
    eng, lone, S, rows_of, ranges = _seam_case(True)
    assert len(ranges) == 5 and all(rows_of[ch] == ranges for ch in range(N_RATES))
    exp, rec = _assert_pass(eng, lone, 15000, 115000, 116000, rows_of)
    assert len(exp) > 100 and not any(a <= s + lone.tlen - 1 and s <= b for r in exp for s in r['starts'].tolist() for a, b in ranges)
    st, _, _ = lone.photons(0, ranges[-1][0], ranges[-1][1])
    assert len(st) >= 1                                                             # photons the plain run read out as lone


def test_a_pass_leaves_the_batch_alone():
    """the records and counts of the run a pass follows are what they were"""
    eng, lone, S, rows_of, ranges = _seam_case(False)
    before, counts = eng.records().tobytes(), dict(eng.counts)
    eng.lone_hits(15000, 115000, 116000)
    assert eng.records().tobytes() == before and len(before) > 0
    eng.run()
    assert eng.records().tobytes() == before and eng.counts == counts


# ---------------------------------------------------------------------------------------------------- 4: noise
TABLE_LEN = 3000


def _whole_rows(rec, exp):
    """a store-everything threshold: every row is one interval from its first sample to its last even one"""
    assert len(exp) >= 20 and int(rec['length'].sum()) == sum((r['right'] - r['left']) // 2 * 2 + 1 for r in exp)


@pytest.mark.parametrize('kind', [3, 5])
def test_drawn_noise_at_the_absolute_sample(kind):
    from tests.test_gpu_noise_slow import _slow
    m = {'sigma': np.random.default_rng(3).uniform(0.0, 4.0, 494)}
    if kind == 5:
        m['slow'] = _slow(494, (5, 9))
    eng = make_engine(_base(enable_noise=True, noise_model=m, zle_threshold=-40000))
    lone = _lone_of(eng)
    noise_of = lambda r: eng.noise_samples(r['channel'], r['left'], r['right'] - r['left'] + 1)
    for s0 in (64 * 1354 - 1000, -2 ** 36 - 7):
        exp, rec = _assert_pass(eng, lone, s0, s0 + 3000, s0 + 3500, noise_of=noise_of)
        _whole_rows(rec, exp)
        assert len({r['left'] % 4 for r in exp}) == 4                   # the rows' first samples take every residue of the drawn quads
    r = exp[0]
    assert np.array_equal(eng.dark_count_samples(r['channel'], r['left'], r['right'] - r['left'] + 1), lone.term(r)) and noise_of(r).any()


@pytest.mark.parametrize('kind', [1, 2])
def test_table_noise_from_the_rows_own_offset(kind):
    noise = np.random.default_rng(5).integers(-9, 10, size=(TABLE_LEN, 494)).astype(np.float64 if kind == 2 else np.int16)
    if kind == 2:           # multiples of 1/8: table + D is exact in float64, the truncated sum is the device's
        noise = noise + np.random.default_rng(6).integers(-3, 4, size=noise.shape) / 8.0
    eng = make_engine(_base(enable_noise=True, noise_data=noise, zle_threshold=-40000))
    lone = _lone_of(eng, TABLE_LEN)
    noise_of = lambda r: noise[(r['ix_rand'] + np.arange(r['right'] - r['left'] + 1)) % TABLE_LEN, r['channel']]
    s0 = 64 * 1354 - 1000
    exp, rec = _assert_pass(eng, lone, s0, s0 + 12000, s0 + 12500, noise_of=noise_of, float_noise=kind == 2)
    _whole_rows(rec, exp)
    ix = [r['ix_rand'] for r in exp]
    assert len(set(ix)) > len(ix) // 2 and any(i + r['right'] - r['left'] + 1 > TABLE_LEN for i, r in zip(ix, exp))       # a row that wraps


# ---------------------------------------------------------------------------------------------------- 5: above the engine
def _ins(times, amp=300, s2=False):
    rows = []
    for k, t in enumerate(times):
        rows.append(dict(type=1, time=t, x=0, y=0, z=-10 - k, amp=amp))
        if s2:
            rows.append(dict(type=2, time=t, x=1, y=-2, z=-10 - k, amp=20))
    return _instructions(rows)


LONE_RATES = np.concatenate([np.full(5, 4e4), [0.0], np.full(2, 4e4)])          # 40 kHz on seven tubes: some 0.3 lone rows per us
TIMES = [MS + 130_000 * k for k in range(9)]


def _rawdata_cfg(**kw):
    return xenonnt_test_config(seed=SEED + 2, dark_count_rate=LONE_RATES, **kw)


def _run_rawdata(cfg, ins, quanta=None):
    rd = wfsim_amd.RawData(cfg)
    if quanta:
        rd.max_batch_quanta = quanta
    rd.engine.set_record_order(True)
    batches = list(rd.iter_batches(ins))
    win = np.concatenate([np.asarray(b['records'][:b['first'][-1]]) for b in batches])
    lone = [b['lone_records'] for b in batches if 'lone_records' in b]
    return rd, batches, win, (np.concatenate(lone) if lone else None)


def test_rawdata_batches_and_the_key():
    """key absent == key False, on a mixed case: no entry, the same bytes; one batch == small batches; the window records do not
    depend on the key"""
    mixed = _ins(TIMES[:5], s2=True)
    off_rd, off_b, off_win, off_lone = _run_rawdata(_rawdata_cfg(), mixed)
    no_rd, no_b, no_win, no_lone = _run_rawdata(_rawdata_cfg(dark_count_lone_hits=False), mixed)
    assert off_lone is None and no_lone is None and no_win.tobytes() == off_win.tobytes() and len(off_win) > 100
    assert all(set(a) == set(b) and 'lone_records' not in a for a, b in zip(off_b, no_b))
    assert off_rd.engine.lone_hits_on is False and no_rd.engine.lone_hits_on is False
    ins = _ins(TIMES)                                       # S1s 130 us apart: a window each
    _, _, off_win, _ = _run_rawdata(_rawdata_cfg(), ins)
    one_rd, one_b, one_win, one_lone = _run_rawdata(_rawdata_cfg(dark_count_lone_hits=True), ins)
    few_rd, few_b, few_win, few_lone = _run_rawdata(_rawdata_cfg(dark_count_lone_hits=True), ins, quanta=100)
    assert len(one_b) == 1 and len(one_b[0]['left']) == len(TIMES) and len(few_b) >= 3
    assert one_win.tobytes() == off_win.tobytes() and few_win.tobytes() == off_win.tobytes()
    assert len(one_lone) > 100 and LH.sort_records(few_lone).tobytes() == LH.sort_records(one_lone).tobytes()
    # the span: from right_raw_extension in front of the first window to right_raw_extension behind the last
    left, right = int(one_b[0]['left'][0]), int(one_b[0]['right'][-1])
    rext, dt = 100000, 10
    assert one_lone['time'].min() >= (left - rext // dt - 50) * dt and one_lone['time'].max() < (right + 1 + rext // dt) * dt
    assert one_lone['time'].min() < left * dt - rext // 2 and one_lone['time'].max() > right * dt + rext // 2
    # ... and what the one pass of the single batch reads out is what the engine reads out over that span against the same rows
    direct = one_rd.engine.lone_hits(left - rext // dt, right + 1 + rext // dt)
    assert LH.sort_records(direct).tobytes() == LH.sort_records(one_lone).tobytes()
    # iter_windows: the same records, lone entries between the windows in time order
    rd = wfsim_amd.RawData(_rawdata_cfg(dark_count_lone_hits=True))
    entries = list(rd.iter_windows(ins))
    assert rd.source_finished
    lone_e = [e for e in entries if e.get('lone')]
    assert len(lone_e) > 50 and len(entries) - len(lone_e) == len(one_b[0]['left'])
    assert all(a['left'] <= b['left'] for a, b in zip(entries[:-1], entries[1:]))
    assert LH.sort_records(np.concatenate([e['records'] for e in lone_e])).tobytes() == LH.sort_records(one_lone).tobytes()
    assert all(e['left'] * dt == e['records']['time'].min() and e['right'] * dt >= e['records']['time'].max() for e in lone_e)


def _assert_chunks(chunks, bounds, win, lone):
    """every record inside its chunk; records time sorted; the chunks hold the window records and every lone record exactly once;
    no two records of a channel overlap"""
    rr = np.concatenate([c['raw_records'] for c in chunks])
    for c, (pre, end) in zip(chunks, bounds):
        if len(c['raw_records']):
            assert c['raw_records']['time'].min() >= pre and c['raw_records']['time'].max() <= end
    assert np.all(np.diff(rr['time']) >= 0)
    both = np.concatenate([win, lone])
    assert len(rr) == len(both) and LH.sort_records(rr).tobytes() == LH.sort_records(both).tobytes()
    for ch in np.unique(rr['channel']):
        r = rr[rr['channel'] == ch]
        assert np.all(r['time'][1:] >= r['time'][:-1] + r['length'][:-1].astype(np.int64) * r['dt'][:-1]), ch
    return rr


def test_chunker_merges_lone_records():
    """a few instructions over three short chunks; a chunk boundary cuts no lone row (a row's records share a chunk)"""
    cfg = _rawdata_cfg(dark_count_lone_hits=True, chunk_size=0.0004)
    ins = _ins(TIMES)
    sim = wfsim_amd.ChunkRawRecords(cfg)
    chunks, bounds = [], []
    for c in sim(ins):
        chunks.append(c)
        bounds.append((sim.chunk_time_pre, sim.chunk_time))
    assert len(chunks) >= 3
    # the same span through RawData alone (the chunker begins trigger_window samples behind the first chunk's start)
    _, _, win, lone = _run_rawdata(dict(cfg, lone_hits_begin=bounds[0][0] + 50 * 10), ins)
    rr = _assert_chunks(chunks, bounds, win, lone)
    assert len(lone) > 100 and sum(len(c['raw_records']) > 0 for c in chunks) >= 3
    for c in chunks:                                        # the fragments of an interval are in one chunk
        r = c['raw_records']
        last = r[r['record_i'] > 0]
        assert len(r) == 0 or np.all(np.isin(last['time'] - 110 * 10 * last['record_i'].astype(np.int64), r['time'][r['record_i'] == 0]))
    off = np.concatenate([c['raw_records'] for c in wfsim_amd.ChunkRawRecords(_rawdata_cfg(chunk_size=0.0004))(ins)])
    assert LH.sort_records(off).tobytes() == LH.sort_records(win).tobytes()


def test_optical_input_with_veto_rates():
    from wfsim_amd.workloads import nveto_config, optical_instructions
    ins, channels, timings = optical_instructions(60, 20000.0, 3)
    channels = channels % 8                                 # eight veto-shaped channels carry the photons and the rates
    cfg = nveto_config(seed=SEED + 3, right_raw_extension=5000, chunk_size=0.0004, dark_count_rate=np.full(8, 4e4), dark_count_lone_hits=True)
    sim = wfsim_amd.ChunkRawRecords(cfg, rawdata_generator=wfsim_amd.RawDataOptical, channels=channels, timings=timings)
    sim.truth_buffer = np.zeros(1000, dtype=instruction_dtype + optical_extra_dtype + sim.truth_dtype + [('fill', bool)])
    chunks, bounds = [], []
    for c in sim(ins):
        chunks.append(c)
        bounds.append((sim.chunk_time_pre, sim.chunk_time))
    assert len(chunks) >= 3
    rd = wfsim_amd.RawDataOptical(dict(cfg, lone_hits_begin=bounds[0][0] + 50 * 10), channels=channels, timings=timings)
    rd.engine.set_record_order(True)
    batches = list(rd.iter_batches(ins))
    lone = np.concatenate([b['lone_records'] for b in batches])
    win = np.concatenate([np.asarray(b['records'][:b['first'][-1]]) for b in batches])
    rr = _assert_chunks(chunks, bounds, win, lone)
    assert len(lone) > 50 and len(win) > 50 and rr['channel'].max() < 8 and 7 not in rr['channel']
