"""Lone-hit rows (config 'dark_count_lone_hits') without a GPU: properties of the restatement (tests/lone_hits.py), the
restatement pinned on the UNCHANGED oracle, the config checks, and the host-only pieces of wfs_lone.h in a program of their own.

The designed stretches were found by a CPU scan of the restatement at 0.96 of the largest rate under SEED: on channel 5 the cell 1354
holds four photons, two consecutive photons start exactly G = 122 samples apart at sample 1059965 (one row) and G + 1 apart at 272538
(two rows); on channel 260 the same gaps are at 456649 and 11403.  Every test asserts what it relies on before it compares anything.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dark_counts as DK
from tests import lone_hits as LH
from tests.helpers import host_tables, make_oracle, with_fma
from wfsim_amd import dark_counts as DC
from wfsim_amd.config import kernel_params, xenonnt_test_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
NEAR_LIMIT = 0.96
# (channel, first sample, samples) of the designed stretches, and what each holds
STRETCHES = {'four': (5, 64 * 1354 - 1000, 3000), 'gap_G_5': (5, 1059965 - 1000, 3000), 'gap_G1_5': (5, 272538 - 1000, 3000),
             'gap_G_260': (260, 456649 - 1000, 3000), 'gap_G1_260': (260, 11403 - 1000, 3000)}
AT = {'gap_G_5': 1059965, 'gap_G1_5': 272538, 'gap_G_260': 456649, 'gap_G1_260': 11403}
REACH = 5000            # s_limit - s1 of the stretches: no chain of theirs is that long (asserted)


def _config(**kw):
    return with_fma(xenonnt_test_config(seed=SEED, enable_noise=False, **kw), False)


@pytest.fixture(scope='module')
def world():
    cfg = _config()
    p = kernel_params(cfg)
    rates = np.full(300, DC.max_rate(p['dt']) * NEAR_LIMIT)
    rates[6] = 0.0                                          # rate 0 between two channels with a rate
    dark = DK.Dark.of_config(cfg, DC.thresholds(rates, 494, p['dt']))
    return cfg, p, dark, LH.Lone(dark, p['trigger_window'])


def _key(rows):
    return [(r['channel'], r['left'], r['right'], r['n_photons'], tuple(r['starts'].tolist())) for r in rows]


# ---------------------------------------------------------------------------------------------------- the restatement
def test_chains_never_straddle_a_row(world):
    """rows of the shortest length a row with a pulse can have, dropped every 700 samples: photons on the two sides of one are never one
    chain (Lone.rows asserts it for every chain it forms), every lone photon is in exactly one row, clipped rows touch no row"""
    cfg, p, dark, lone = world
    G = lone.G
    rows = [(a, a + G - 1) for a in range(1000, 60000, 700)]
    got = lone.rows(5, 0, 60000, 60000 + REACH, rows)
    assert len(got) > 50
    starts, _, _ = lone.photons(5, 0, 60000)
    lone_starts = [int(s) for s in starts if lone.is_lone(int(s), rows)]
    in_rows = sorted(int(s) for r in got for s in r['starts'] if s < 60000)
    assert in_rows == lone_starts and len(lone_starts) < len(starts)
    clipped = 0
    for r in got:
        assert r['left'] <= r['starts'][0] and r['right'] >= r['starts'][-1] + lone.tlen - 1
        assert not any(r['left'] <= b and r['right'] >= a for a, b in rows)
        assert all(np.diff(r['starts']) <= G)
        clipped += int(r['left'] > r['starts'][0] - lone.tw or r['right'] < r['starts'][-1] + lone.tlen - 1 + lone.tw)
    assert clipped >= 10
    firsts = [r['starts'][0] for r in got]
    lasts = [r['starts'][-1] for r in got]
    assert all(f - l > G for f, l in zip(firsts[1:], lasts[:-1]))


def test_a_pass_split_anywhere_gives_the_rows_of_one_pass(world):
    cfg, p, dark, lone = world
    a, n = 272538 - 1000, 2000
    rows = [(a + 600, a + 600 + lone.G + 30)]
    for ch in (5, 260):             # (0.12 photons per cell: some four photons in 2000 samples)
        whole = _key(lone.rows(ch, a, a + n, a + n + 300, rows))
        assert len(whole) >= 2
        for cut in range(a, a + n + 1):
            parts = _key(lone.rows(ch, a, cut, a + n + 300, rows)) + _key(lone.rows(ch, cut, a + n, a + n + 300, rows))
            assert parts == whole, (ch, cut)
    # the awkward cuts are among them: inside a chain, and one sample behind a chain's first photon
    multi = [r for r in lone.rows(5, a, a + n, a + n + 300, rows) if r['n_photons'] >= 2]
    assert multi and all(a < r['starts'][0] + 1 <= a + n and a < r['starts'][1] <= a + n for r in multi)


def test_s_limit_cuts_a_chain(world):
    cfg, p, dark, lone = world
    a = 1059965 - 1000
    whole = [r for r in lone.rows(5, a, a + 3000, a + 3000 + REACH) if r['n_photons'] >= 2][0]
    cut_at = int(whole['starts'][1])                      # the second photon starts at s_limit: not taken
    s1 = int(whole['starts'][0]) + 1
    cut = [r for r in lone.rows(5, a, s1, cut_at) if r['starts'][0] == whole['starts'][0]][0]
    assert cut['n_photons'] == 1 and cut['right'] == min(cut_at - 1, whole['starts'][0] + lone.tlen - 1 + lone.tw) and cut['left'] == whole['left']


def test_no_rows_where_no_photon_is_due(world):
    cfg, p, dark, lone = world
    gains = np.asarray(cfg['gains'])
    dead = int(np.flatnonzero(gains[:300] == 0)[0]) if np.any(gains[:300] == 0) else None
    assert lone.rows(6, 0, 50000, 50000) == [] and lone.rows(300, 0, 50000, 50000) == [] and lone.rows(493, 0, 50000, 50000) == []
    if dead is not None:
        assert lone.rows(dead, 0, 50000, 50000) == []
    d0 = DK.Dark(dark.seed, dark.dt, dark.before, dark.tlen, dark.c2a, dark.templates, dark.spe, np.zeros_like(dark.gains), dark.thr)
    assert LH.Lone(d0, lone.tw).rows(5, 0, 50000, 50000) == [] and len(lone.rows(5, 0, 50000, 50000)) > 40      # (781 cells x 0.12: some 94 photons)


def test_ix_rand(world):
    cfg, p, dark, lone = world
    tab = LH.Lone(dark, lone.tw, noise_len=3000)
    ix = [tab.ix_rand(5, left) for left in range(-40, 40)] + [tab.ix_rand(5, 2 ** 40 + 3), tab.ix_rand(5, -2 ** 40 - 3)]
    assert all(0 <= i < 3000 for i in ix) and len(set(ix)) > 70 and lone.ix_rand(5, 17) == 0
    assert tab.ix_rand(5, 17) != tab.ix_rand(8, 17)


# ---------------------------------------------------------------------------------------------------- the oracle pin
def _stretch_rows(lone, name):
    ch, a, n = STRETCHES[name]
    rows = lone.rows(ch, a, a + n, a + n + REACH)
    assert rows and all(r['right'] < a + n + REACH - 1 for r in rows)           # no chain reaches s_limit
    return rows


def test_designed_stretches_hold_their_seams(world):
    cfg, p, dark, lone = world
    G = lone.G
    rows = _stretch_rows(lone, 'four')
    m = 1354
    assert dark.counts(5, [m])[0] == 4
    four = [r for r in rows if np.sum((r['starts'] + lone.before) >> 6 == m) == 4]
    assert len(four) == 1
    assert any(r['n_photons'] == 2 for r in rows) and any(r['n_photons'] >= 3 for r in rows)
    for name in ('gap_G_5', 'gap_G_260'):
        rows = _stretch_rows(lone, name)
        assert any(AT[name] in r['starts'].tolist() and AT[name] + G in r['starts'].tolist() for r in rows), name          # one row
    for name in ('gap_G1_5', 'gap_G1_260'):
        rows = _stretch_rows(lone, name)
        ends = [r for r in rows if r['starts'][-1] == AT[name]]
        begins = [r for r in rows if r['starts'][0] == AT[name] + G + 1]
        assert len(ends) == 1 and len(begins) == 1 and begins[0]['left'] == ends[0]['right'] + 2, name      # two rows, one sample between them


@pytest.mark.parametrize('name', sorted(STRETCHES))
def test_records_are_the_oracles(world, name):
    """noise off, the thresholds of the bundled configuration: range, per-photon rounding, ZLE and fragments against the reference's
    rules, byte for byte"""
    cfg, p, dark, lone = world
    assert (p['store_before'] + p['samples_before']) % 2 == 0           # (the oracle's wider pulse keeps the parity of a lone row's first sample)
    rows = _stretch_rows(lone, name)
    thr = host_tables(cfg)['thr_zle']
    data = [LH.finish(lone.term(r), p['baseline']) for r in rows]
    mine = LH.records_of_rows(rows, data, lambda ch: int(thr[ch]), p['trigger_window'], p['dt'])
    assert len(mine) >= 3 and mine['pulse_length'].max() > 2 * lone.tw          # dark pulses cross the threshold (a photon of a small gain does not)
    theirs = LH.oracle_records(make_oracle(cfg), rows, p['n_tpc'], p['samples_before'], p['dt'])
    assert len(theirs) == len(mine) and theirs.tobytes() == mine.tobytes()


# ---------------------------------------------------------------------------------------------------- config
def test_config_key():
    assert DC.lone_hits_from(_config()) is False
    assert DC.lone_hits_from(_config(dark_count_rate=40.0)) is False
    assert DC.lone_hits_from(_config(dark_count_rate=40.0, dark_count_lone_hits=True)) is True
    with pytest.raises(ValueError, match='dark_count_lone_hits: needs'):
        DC.lone_hits_from(_config(dark_count_lone_hits=True))
    with pytest.raises(ValueError, match='dark_count_lone_hits: needs'):
        DC.lone_hits_from(_config(dark_count_lone_hits=True, dark_count_rate=np.zeros(494)))
    p = kernel_params(_config())
    need = DC.lone_min_rext(p)
    assert need == (2 * (p['tlen'] + 2 * p['trigger_window']) + 64) * p['dt'] == 3080
    with pytest.raises(ValueError, match='right_raw_extension 3079 ns below'):
        DC.lone_hits_from(_config(dark_count_lone_hits=True, dark_count_rate=40.0, right_raw_extension=need - 1))
    assert DC.lone_hits_from(_config(dark_count_lone_hits=True, dark_count_rate=40.0, right_raw_extension=need)) is True


def test_stretches_of_lone_records():
    from wfsim_amd.dtypes import raw_record_dtype
    from wfsim_amd.rawdata import lone_stretches
    r = np.zeros(6, dtype=raw_record_dtype())
    r['dt'], r['length'] = 10, [110, 40, 30, 20, 110, 10]
    r['time'] = np.array([100, 210, 215, 300, 400, 510]) * 10          # 100 .. 249 (two fragments), 215 .. 244 inside, 300 .. 319, 400 .. 519
    left, right, first = lone_stretches(r)
    assert left.tolist() == [100, 300, 400] and right.tolist() == [249, 319, 519] and first.tolist() == [0, 3, 4, 6]
    left, right, first = lone_stretches(r[:0])
    assert len(left) == 0 and first.tolist() == [0]


# ---------------------------------------------------------------------------------------------------- the host pieces of wfs_lone.h
HOST_CASES = ['gap', 'cells', 'pulse_meets', 'range', 'straddle', 'ix_rand', 'check', 'rext']


def test_host_rules_under_sanitizers(tmp_path_factory):
    """tests/host/lone_rules_main.cpp: a program of its own, built with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes, run on the CPU"""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('lone_rules') / 'lone_rules_main')
    cmd = [cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-g', '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'), '-o', exe,
           os.path.join(ROOT, 'tests', 'host', 'lone_rules_main.cpp')]
    if subprocess.run(cmd + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    q = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert q.returncode == 0, (q.returncode, q.stdout, q.stderr)
    lines = [ln.split() for ln in q.stdout.splitlines()]
    assert [ln[0] for ln in lines] == HOST_CASES and all(ln[1:] == ['ok'] for ln in lines), lines
