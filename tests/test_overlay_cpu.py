"""The overlay rule on the CPU (config 'overlay_records'): the two numpy restatements of tests/overlay.py against each
other, the identities, the config checks, the cut of a background pulse at a pass boundary on a hand-made schedule, and
wfsim_amd/csrc/wfs_overlay.h in a program of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import overlay as OV
from wfsim_amd import overlay as WO
from wfsim_amd.config import kernel_params, xenonnt_test_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = kernel_params(xenonnt_test_config())
DT, BASELINE, N_ROWS = int(P['dt']), int(P['baseline']), int(P['n_rows'])
CHS = dict(first=0, last_tpc=P['n_tpc'] - 1, he=P['he_first'] + 3, sum=P['sum_channel'])
CASES = OV.designed_cases(CHS, BASELINE)


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatements_agree_on_designed_cases(name):
    A, B, overrides = CASES[name]
    base = OV.base_array(N_ROWS, BASELINE, overrides)
    x, y = OV.merge_intervals(A, B, BASELINE, base, DT), OV.merge_dense(A, B, BASELINE, base, DT)
    assert len(x) and x.tobytes() == y.tobytes()
    assert OV.no_shared_samples(x, DT)
    assert not np.any(x['baseline']) and np.all(x['dt'] == DT)
    for r in x:
        assert not np.any(r['data'][r['length']:])


@pytest.mark.parametrize('seed', [11, 12, 13, 14])
def test_restatements_agree_on_random_mixes(seed):
    level = {ch: BASELINE - 400 + 100 * ch for ch in range(8)}
    A, B = OV.random_streams(seed, baseline=BASELINE, base_level=level)
    base = OV.base_array(N_ROWS, BASELINE, level)
    x, y = OV.merge_intervals(A, B, BASELINE, base, DT), OV.merge_dense(A, B, BASELINE, base, DT)
    assert x.tobytes() == y.tobytes() and OV.no_shared_samples(x, DT)
    n_in = len(A) + len(B)
    assert len(OV.pulses_of(x, DT)) < n_in              # some pulses merged


@pytest.mark.parametrize('merge', [OV.merge_intervals, OV.merge_dense])
def test_identities(merge):
    """B empty with the default base gives A sorted by (time, channel); A empty gives B sorted, whatever the base"""
    base = OV.base_array(N_ROWS, BASELINE, {})
    A, B = OV.random_streams(21, baseline=BASELINE)
    a, b = OV.fragments(A, DT), OV.fragments(B, DT)
    assert merge(A, [], BASELINE, base, DT).tobytes() == a.tobytes()
    assert merge([], B, BASELINE, OV.base_array(N_ROWS, BASELINE, {0: 1, 3: 20000}), DT).tobytes() == b.tobytes()
    assert np.all(np.diff(a['time']) >= 0) and OV.pulses_of(a, DT)[0][2].tobytes() == sorted(A, key=lambda p: (p[0], p[1]))[0][2].tobytes()


def test_config_errors():
    cfg = xenonnt_test_config()
    bg = OV.fragments(OV.random_streams(3, n_pulses=5)[1], DT)
    assert WO.overlay_from(cfg, P) == (None, None)
    src, base = WO.overlay_from(dict(cfg, overlay_records=bg), P)
    assert base is None and len(src.take(0, 2 ** 62)) == len(bg)
    for key in ('dark_count_lone_hits', 'noise_lone_hits'):
        with pytest.raises(ValueError, match=key):
            WO.overlay_from(dict(cfg, overlay_records=bg, **{key: True}), P)
    with pytest.raises(ValueError, match='shard'):
        WO.overlay_from(dict(cfg, overlay_records=bg), P, sharded=True)
    with pytest.raises(ValueError, match='sorted'):
        WO.overlay_from(dict(cfg, overlay_records=bg[::-1]), P)
    with pytest.raises(ValueError, match='raw_records'):
        WO.overlay_from(dict(cfg, overlay_records=np.zeros(3)), P)
    _, base = WO.overlay_from(dict(cfg, overlay_records=bg, overlay_baseline=15000), P)
    assert base.dtype == np.int32 and base.tolist() == [15000] * N_ROWS
    _, base = WO.overlay_from(dict(cfg, overlay_records=bg, overlay_baseline=[15000, 15001]), P)
    assert base.tolist() == [15000, 15001] + [BASELINE] * (N_ROWS - 2)
    from wfsim_amd.strax_interface import RawRecordsFromFaxNT
    plug = RawRecordsFromFaxNT.__new__(RawRecordsFromFaxNT)
    plug.config = dict(cfg, overlay_records=bg, shard=(0, 2))
    with pytest.raises(ValueError, match='shard'):
        plug._shard()
    from wfsim_amd import distributed
    with pytest.raises(ValueError, match='shard'):
        distributed.simulate_sharded(dict(cfg, overlay_records=bg), np.zeros(0))


def test_source_takes_pulses_by_their_start():
    """a pulse belongs to the range its FIRST fragment starts in, with all its fragments; array and callable agree"""
    t0 = OV.EPOCH // 10
    B = [(1, t0, np.arange(300, dtype=np.int16)), (2, t0 + 100, np.arange(5, dtype=np.int16)), (1, t0 + 400, np.arange(120, dtype=np.int16))]
    rec = OV.fragments(B, DT)
    src = WO.OverlaySource(rec)
    got = src.take(t0 * DT, (t0 + 100) * DT)
    assert [(c, s, len(d)) for c, s, d in OV.pulses_of(got, DT)] == [(1, t0, 300)]
    got = src.take((t0 + 100) * DT, (t0 + 401) * DT)
    assert [(c, s, len(d)) for c, s, d in OV.pulses_of(got, DT)] == [(1, t0 + 400, 120), (2, t0 + 100, 5)]
    assert len(src.take((t0 + 401) * DT, 2 ** 62)) == 0
    fn = WO.OverlaySource(lambda a, b: src.take(a, b)[::-1])
    assert fn.take(t0 * DT, (t0 + 401) * DT).tobytes() == rec.tobytes()


def test_pass_boundary_cut_on_a_hand_made_schedule():
    """three passes (T, cut) over a stream whose pulses straddle T, the cut, both, and two cuts in a row: the fronts go to the pass, the
    rests are pulses of the next; no output pulse shares a sample with another on its channel and every background sample is delivered
    exactly once"""
    t0 = OV.EPOCH // 10
    rng = np.random.default_rng(7)
    mk = lambda ch, s, n: (ch, t0 + s, rng.integers(0, 16000, size=n).astype(np.int16))          # noqa: E731
    B = [mk(0, 10, 50), mk(0, 950, 100),      # across T = 1000, ends in front of the cut at 1200: whole in pass 0
         mk(1, 990, 400),                      # across T and the cut: front 210 samples, rest a pulse of pass 1
         mk(2, 1100, 50),                      # starts behind T: pass 1
         mk(3, 900, 2000),                     # across the cuts of pass 0 (1200) and pass 1 (2500): cut twice
         mk(4, 1199, 1), mk(4, 1200, 1),       # the last sample in front of the cut, the first behind it (starts behind T: pass 1)
         mk(0, 2300, 220), mk(5, 2600, 30), mk(5, 5000, 10)]
    src = WO.OverlaySource(OV.fragments(B, DT))
    schedule = [(1000, 1200), (2400, 2500), (6000, None)]         # (T, cut) in samples relative to t0
    carry, begin, outs = np.zeros(0, dtype=OV.DTYPE), t0 * DT, []
    base = OV.base_array(N_ROWS, BASELINE, {})
    for T, cut in schedule:
        bg, carry = WO.pass_pulses(src, carry, begin, (t0 + T) * DT, None if cut is None else t0 + cut, DT)
        begin = (t0 + T) * DT
        if cut is not None:
            assert all(s + len(d) <= t0 + cut for _, s, d in OV.pulses_of(bg, DT))
            assert all(s >= t0 + cut for _, s, d in OV.pulses_of(carry, DT))
        out = OV.merge_intervals([], OV.pulses_of(bg, DT), BASELINE, base, DT)
        assert out.tobytes() == bg.tobytes()           # (the records a pass is given are a valid stream in time order)
        outs.append(out)
    assert len(carry) == 0
    assert [len(OV.pulses_of(o, DT)) for o in outs] == [4, 6, 4]           # (counted by hand from the list above)
    allrec = OV.sort_records(np.concatenate(outs))
    assert OV.no_shared_samples(allrec, DT)
    dense = {}
    for ch, s, d in OV.pulses_of(allrec, DT):
        for k, v in enumerate(d.tolist()):
            assert (ch, s + k) not in dense
            dense[(ch, s + k)] = v
    want = {(ch, s + k): v for ch, s, d in B for k, v in enumerate(d.tolist())}
    assert dense == want
    cut3 = [(s - t0, len(d)) for ch, s, d in OV.pulses_of(allrec, DT) if ch == 3]
    assert cut3 == [(900, 300), (1200, 1300), (2500, 400)]


# ---------------------------------------------------------------------------------------------------- wfs_overlay.h on the host
HOST_CASES = ['header', 'record', 'pairs', 'keys', 'merge', 'sample']


def test_host_rules_under_sanitizers(tmp_path_factory):
    """tests/host/overlay_rules_main.cpp: a program of its own, built with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes, run on the CPU"""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('overlay_rules') / 'overlay_rules_main')
    cmd = [cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-g', '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'), '-o', exe,
           os.path.join(ROOT, 'tests', 'host', 'overlay_rules_main.cpp')]
    if subprocess.run(cmd + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    q = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert q.returncode == 0, (q.returncode, q.stdout, q.stderr)
    lines = [ln.split() for ln in q.stdout.splitlines()]
    assert [ln[0] for ln in lines] == HOST_CASES and all(ln[1:] == ['ok'] for ln in lines), lines
