"""The overlay pass on the device (config 'overlay_records', wfs_overlay_records; MI355X only).

The rule is restated twice in numpy in tests/overlay.py (tests/test_overlay_cpu.py holds the two against each other).  The device is
held to the restatement byte for byte: on the designed cases with both streams supplied from the host, on random mixes, on invalid
streams, and with the records of a run where the device holds them, through RawData and ChunkRawRecords.  No test compares the device
with itself.
"""
import numpy as np
import pytest

import wfsim_amd
from tests import overlay as OV
from tests.helpers import make_engine, with_fma
from tests.test_gpu_noise_model import _instructions
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.engine import WfsError, device_allocations
from wfsim_amd.overlay import OverlaySource

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


@pytest.fixture(scope='module')
def eng():
    return make_engine(with_fma(xenonnt_test_config(), False))


def _chs(p):
    return dict(first=0, last_tpc=p['n_tpc'] - 1, he=p['he_first'] + 3, sum=p['sum_channel'])


def _cases(p):
    return OV.designed_cases(_chs(p), p['baseline'])


def _expect(p, A, B, overrides=None):
    base = OV.base_array(p['n_rows'], p['baseline'], overrides or {})
    return OV.merge_intervals(A, B, p['baseline'], base, p['dt']), base


def _assert_case(eng, A, B, overrides, what):
    p = eng.params
    want, base = _expect(p, A, B, overrides)
    got = eng.overlay_records(OV.fragments(B, p['dt']), sim=OV.fragments(A, p['dt']), baseline=base if overrides else None)
    assert len(got) == len(want), (what, len(got), len(want))
    assert got.tobytes() == want.tobytes(), (what, np.flatnonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)])[:5])
    return got


CASE_NAMES = ['front_one_sample', 'back_one_sample', 'touching', 'b_inside_a', 'a_inside_b', 'chain_abab', 'merged_109', 'merged_110',
              'merged_111', 'merged_220', 'merged_221', 'offset_1', 'offset_109', 'five_against_one', 'channels', 'equal_times', 'epoch',
              'clamp', 'base', 'lone_pulses']


def test_the_case_list_is_whole(eng):
    p = eng.params
    assert sorted(_cases(p)) == sorted(CASE_NAMES)
    assert p['he_first'] + 3 < p['sum_channel'] < p['n_rows'] and p['n_tpc'] <= p['he_first']


@pytest.mark.parametrize('name', CASE_NAMES)
def test_designed_case(eng, name):
    A, B, overrides = _cases(eng.params)[name]
    got = _assert_case(eng, A, B, overrides, name)
    pulses = OV.pulses_of(got, eng.params['dt'])
    if name in ('front_one_sample', 'back_one_sample', 'b_inside_a', 'a_inside_b', 'chain_abab', 'offset_1', 'offset_109', 'five_against_one'):
        assert len(pulses) == 1
    if name == 'touching':
        assert len(pulses) == 3
    if name.startswith('merged_'):
        assert len(pulses) == 1 and len(pulses[0][2]) == int(name[7:])
    if name == 'epoch':
        assert got['time'].min() > 1.69e18
    if name == 'clamp':
        assert (got['data'] == 0).any() and (got['data'] == 32767).any()
    if name == 'channels':
        assert sorted(set(got['channel'].tolist())) == sorted(_chs(eng.params).values())


@pytest.mark.parametrize('name', ['chain_abab', 'channels', 'epoch'])
def test_identities(eng, name):
    """B empty with the default base gives A sorted by (time, channel); A empty gives B sorted"""
    p = eng.params
    A, B, _ = _cases(p)[name]
    a, b = OV.fragments(A, p['dt']), OV.fragments(B, p['dt'])
    rng = np.random.default_rng(5)
    none = np.zeros(0, dtype=OV.DTYPE)
    assert eng.overlay_records(none, sim=a[rng.permutation(len(a))]).tobytes() == a.tobytes()
    assert eng.overlay_records(b[rng.permutation(len(b))], sim=none).tobytes() == b.tobytes()
    assert len(eng.overlay_records(none, sim=none)) == 0


@pytest.mark.parametrize('seed', [11, 12, 13])
def test_random_mixes(eng, seed):
    """200 pulses per stream on 8 channels, a recorded baseline of its own on every channel"""
    p = eng.params
    level = {ch: p['baseline'] - 400 + 100 * ch for ch in range(8)}
    A, B = OV.random_streams(seed, baseline=p['baseline'], base_level=level)
    got = _assert_case(eng, A, B, level, seed)
    assert len(OV.pulses_of(got, p['dt'])) < 400 and OV.no_shared_samples(got, p['dt'])
    assert got.tobytes() == OV.merge_dense(A, B, p['baseline'], OV.base_array(p['n_rows'], p['baseline'], level), p['dt']).tobytes()


def _invalid_streams(p):
    dt = p['dt']
    good = OV.fragments([(3, 1000, np.full(250, 15000, dtype=np.int16)), (3, 2000, np.full(30, 15000, dtype=np.int16))], dt)
    out = {}
    r = good.copy(); r['dt'][1] = dt + 1; out['dt'] = r
    r = good.copy(); r['time'][2] += 1; out['time'] = r
    r = good.copy(); r['length'][3] = 0; out['length_0'] = r
    r = good.copy(); r['length'][0] = 111; out['length_111'] = r
    r = good.copy(); r['channel'][3] = p['n_rows']; out['channel'] = r
    r = good.copy(); r['channel'][3] = -1; out['channel_negative'] = r
    out['missing_middle'] = good[[0, 2, 3]]
    out['missing_last'] = good[[0, 1, 3]]
    out['missing_first'] = good[[1, 2, 3]]
    r = good.copy(); r['time'][1] += dt; out['spacing'] = r
    r = good.copy(); r['length'][2] = 31; out['fragment_length'] = r
    r = good.copy(); r['record_i'][3] = 1; out['record_i'] = r
    r = good.copy(); r['pulse_length'][1] = 251; out['pulse_length'] = r
    out['overlap'] = OV.sort_records(np.concatenate([good, OV.fragments([(3, 1249, np.full(5, 15000, dtype=np.int16))], dt)]))
    out['inside'] = OV.sort_records(np.concatenate([good, OV.fragments([(3, 1050, np.full(5, 15000, dtype=np.int16))], dt)]))
    out['twice'] = OV.sort_records(np.concatenate([good, good[3:]]))
    return good, out


def test_invalid_streams(eng):
    """each kind of invalid stream, as A and as B: WFS_E_INVALID with the stream named, and the handle stays usable"""
    p = eng.params
    good, bad = _invalid_streams(p)
    other = OV.fragments([(3, 1100, np.full(40, 15000, dtype=np.int16))], p['dt'])
    for name, r in bad.items():
        with pytest.raises(WfsError, match=r'background record \d+') as e:
            eng.overlay_records(r, sim=other)
        assert 'error -1:' in str(e.value), name                     # WFS_E_INVALID
        with pytest.raises(WfsError, match=r'simulated record \d+'):
            eng.overlay_records(other, sim=r)
    A, B = OV.pulses_of(other, p['dt']), OV.pulses_of(good, p['dt'])
    _assert_case(eng, A, B, {}, 'after the invalid streams')
    # a pulse of B on the samples of one of A is no fault of either stream
    assert len(eng.overlay_records(good, sim=good)) == len(good)


def test_state_before_a_run():
    """A = the records of the last run: WFS_E_STATE before one"""
    e = make_engine(with_fma(xenonnt_test_config(), False))
    bg = OV.fragments([(3, 1000, np.full(250, 15000, dtype=np.int16))], e.params['dt'])
    with pytest.raises(WfsError) as err:
        e.overlay_records(bg)
    assert 'error -4:' in str(err.value) and 'wfs_run has not completed' in str(err.value)          # WFS_E_STATE
    assert e.overlay_records(bg, sim=np.zeros(0, dtype=OV.DTYPE)).tobytes() == bg.tobytes()
    e.close()


# ---------------------------------------------------------------------------------------------------- above the engine
MS = 1_000_000
TIMES = [MS + 130_000 * k for k in range(3)]


def _ins():
    return _instructions([dict(type=2, time=t, x=1, y=-2, z=-10 - k, amp=20) for k, t in enumerate(TIMES)])


def _cfg(**kw):
    return with_fma(xenonnt_test_config(seed=77, **kw), False)


def _run(cfg, quanta=None):
    rd = wfsim_amd.RawData(cfg)
    if quanta:
        rd.max_batch_quanta = quanta
    rd.engine.set_record_order(True)
    batches = []
    for b in rd.iter_batches(_ins()):
        batches.append(dict(b, records=np.array(b['records'][:b['first'][-1]])))
    return rd, batches


@pytest.fixture(scope='module')
def plain():
    """the run without the key: its windows, its records, the device memory it holds"""
    rd, batches = _run(_cfg())
    assert len(batches) == 1 and len(batches[0]['left']) == 3 and 'overlay_records' not in batches[0]
    alloc = device_allocations()
    b = batches[0]
    out = dict(left=b['left'].copy(), right=b['right'].copy(), records=b['records'].copy(), alloc=alloc, params=dict(rd.engine.params))
    rd.engine.close()
    return out


def _background(plain):
    """designed pulses: across the first window's left, across the last window's right, inside a simulated pulse, on the sum channel
    (which the run does not emit) and far from every window"""
    p, rec = plain['params'], plain['records']
    rng = np.random.default_rng(9)
    mk = lambda ch, s, n: (int(ch), int(s), (p['baseline'] - 700 + rng.integers(-20, 21, size=n)).astype(np.int16))      # noqa: E731
    first = rec[np.argmin(rec['time'])]
    last = rec[np.argmax(rec['time'] + rec['length'].astype(np.int64) * p['dt'])]
    mid = rec[(rec['record_i'] == 0) & (rec['length'] > 40)][7]
    B = [mk(first['channel'], first['time'] // p['dt'] - 100, 130),                                # ends 30 samples inside the first pulse
         mk(last['channel'], last['time'] // p['dt'] + last['length'] - 10, 300),                  # begins 10 samples in front of the last end
         mk(mid['channel'], mid['time'] // p['dt'] + 5, 20),                                       # inside a simulated pulse
         mk(p['sum_channel'], plain['left'][0] - 50, 400), mk(3, plain['right'][0] + 3000, 250), mk(3, plain['left'][0] - 9000, 5)]
    assert plain['left'][0] - 100 < first['time'] // p['dt'] and last['time'] // p['dt'] + last['length'] + 300 > plain['right'][-1]
    return B


def _want(plain, own, B, level):
    p = plain['params']
    base = OV.base_array(p['n_rows'], p['baseline'], {} if level is None else {ch: level for ch in range(p['n_rows'])})
    return OV.merge_intervals(OV.pulses_of(own, p['dt']), B, p['baseline'], base, p['dt'])


def test_rawdata_overlays_the_records_of_a_run(plain):
    """A = the records of the run where the device holds them; the batch's own records keep every byte"""
    p = plain['params']
    B = _background(plain)
    bg = OV.fragments(B, p['dt'])
    rd, batches = _run(_cfg(overlay_records=bg, overlay_baseline=p['baseline'] - 700))
    assert len(batches) == 1
    own, got = batches[0]['records'], batches[0]['overlay_records']
    assert own.tobytes() == plain['records'].tobytes() and len(own) > 50
    want = _want(plain, own, B, p['baseline'] - 700)
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    assert len(OV.pulses_of(got, p['dt'])) == len(OV.pulses_of(own, p['dt'])) + 3          # three of the six merged into simulated pulses
    # the callable form, and iter_windows: window entries without records, the stretches between them in time order
    src = OverlaySource(bg)
    rd2 = wfsim_amd.RawData(_cfg(overlay_records=lambda a, b: src.take(a, b), overlay_baseline=p['baseline'] - 700))
    entries = list(rd2.iter_windows(_ins()))
    wins, stretches = [e for e in entries if not e.get('overlay')], [e for e in entries if e.get('overlay')]
    assert len(wins) == 3 and all(len(e['records']) == 0 for e in wins) and len(stretches) >= 4
    assert all(a['left'] <= b['left'] for a, b in zip(entries[:-1], entries[1:]))
    assert OV.sort_records(np.concatenate([e['records'] for e in stretches])).tobytes() == want.tobytes()
    rd.engine.close(), rd2.engine.close()


def test_small_batches_cut_a_long_background_pulse(plain):
    """a window per batch: the same records where no background pulse runs past a pass, and a pulse of 12000 samples from inside the
    first window on the sum channel cut where the next batch's window can first begin -- every sample of it delivered once"""
    p = plain['params']
    B = _background(plain)
    bg = OV.fragments(B, p['dt'])
    rd, batches = _run(_cfg(overlay_records=bg), quanta=100)
    assert len(batches) == 3
    got = OV.sort_records(np.concatenate([b['overlay_records'] for b in batches]))
    own = np.concatenate([b['records'] for b in batches])
    assert got.tobytes() == _want(plain, own, B, None).tobytes()
    long = (p['sum_channel'], int(plain['right'][0]) - 20, np.arange(12000, dtype=np.int16))
    B2 = [q for q in B if q[0] != p['sum_channel']] + [long]
    rd2, batches2 = _run(_cfg(overlay_records=OV.fragments(B2, p['dt'])), quanta=100)
    got2 = OV.sort_records(np.concatenate([b['overlay_records'] for b in batches2]))
    assert OV.no_shared_samples(got2, p['dt'])
    parts = [q for q in OV.pulses_of(got2, p['dt']) if q[0] == p['sum_channel']]
    assert len(parts) == 2 and parts[0][1] == long[1] and parts[1][1] == parts[0][1] + len(parts[0][2])
    assert np.concatenate([parts[0][2], parts[1][2]]).tobytes() == long[2].tobytes()
    assert plain['right'][0] < parts[1][1] <= plain['left'][1]
    rest = got2[got2['channel'] != p['sum_channel']]
    assert rest.tobytes() == _want(plain, own, [q for q in B2 if q[0] != p['sum_channel']], None).tobytes()
    rd.engine.close(), rd2.engine.close()


def test_chunker_takes_the_overlay(plain):
    """through ChunkRawRecords: time sorted, no two pulses share a sample on a channel, every record inside its chunk, no pulse cut"""
    p = plain['params']
    B = _background(plain)
    cfg = _cfg(overlay_records=OV.fragments(B, p['dt']), chunk_size=0.0001)
    sim = wfsim_amd.ChunkRawRecords(cfg)
    chunks, bounds = [], []
    for c in sim(_ins()):
        chunks.append(c['raw_records'].copy())
        bounds.append((sim.chunk_time_pre, sim.chunk_time))
    assert sum(len(c) > 0 for c in chunks) >= 3
    for c, (pre, end) in zip(chunks, bounds):
        if len(c):
            assert c['time'].min() >= pre and (c['time'] + c['length'].astype(np.int64) * c['dt']).max() <= end
            assert OV.no_shared_samples(c, p['dt'])              # (complete pulses: no pulse is cut at a chunk end)
    rr = np.concatenate(chunks)
    assert np.all(np.diff(rr['time']) >= 0) and OV.no_shared_samples(rr, p['dt'])
    # what the chunks hold is the restatement over the same span: the chunker lets no recorded pulse begin in front of the first chunk
    own = plain['records']
    Bin = [q for q in B if q[1] * p['dt'] >= bounds[0][0]]
    assert OV.sort_records(rr).tobytes() == _want(plain, own, Bin, None).tobytes()
    sim.rawdata.engine.close()


def test_key_absent_changes_nothing(plain):
    """no buffer is allocated and no byte differs without the key; a pass allocates its own and leaves the run's records alone"""
    rd, batches = _run(_cfg())
    assert batches[0]['records'].tobytes() == plain['records'].tobytes() and 'overlay_records' not in batches[0]
    assert rd.overlay is None and device_allocations() == plain['alloc']
    bg = OV.fragments(_background(plain), plain['params']['dt'])
    got = rd.engine.overlay_records(bg)
    assert len(got) > len(bg) and device_allocations()[0] > plain['alloc'][0]
    assert rd.engine.records().tobytes() == plain['records'].tobytes()
    rd.engine.close()
