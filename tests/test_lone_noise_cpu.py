"""Noise-hit seeds of the lone-hit rows (config 'noise_lone_hits') without a GPU: properties of the restatement
(tests/lone_noise.py), the restatement pinned on the UNCHANGED oracle, the config checks, the C header, and the host-only pieces added
to wfs_lone.h in a program of their own.

The model: almost all mass on 0, 2^-9 on -40 ADC counts (the ZLE threshold lies 16 below the baseline: a crossing on its own) and 1/16
on -13 (a crossing only on top of at least -4 of a dark pulse).  The designed positions are found by a scan of the restatement under
SEED (tests/lone_noise.py, the finders); every test asserts what it relies on before it compares anything.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import dark_counts as DK
from tests import lone_hits as LH
from tests import lone_noise as LN
from tests.helpers import host_tables, make_oracle, with_fma
from wfsim_amd import dark_counts as DC
from wfsim_amd.config import kernel_params, xenonnt_test_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261021
NEAR_LIMIT = 0.96
N_MODEL = 8                     # channels 0 .. 7 are inside the model and have a rate; 6 has rate 0: noise hits alone
SPIKE, SMALL = 40, 13
SCAN = 1 << 17
REACH = 5000


def model_config(**kw):
    pmf, vmin = LN.spike_pmf(N_MODEL, SPIKE, small=SMALL, p_small=1.0 / 16)
    return with_fma(xenonnt_test_config(seed=SEED, enable_noise=True, noise_model=dict(pmf=pmf, vmin=vmin), noise_lone_hits=True, **kw), False)


def rates(dt=10):
    r = np.full(N_MODEL, DC.max_rate(dt) * NEAR_LIMIT)
    r[6] = 0.0
    return r


@pytest.fixture(scope='module')
def world():
    cfg = model_config()
    assert DC.noise_lone_hits_from(cfg) is True         # (the configuration the restatement stands for)
    p, t = kernel_params(cfg), host_tables(cfg)
    model, seed = LN.model_of(cfg)
    lone = LH.Lone(DK.Dark.of_config(cfg, DC.thresholds(rates(p['dt']), 494, p['dt'])), p['trigger_window'])
    both = LN.LoneNoise(lone, model, seed, t['thr_zle'], p['baseline'], p['n_tpc'])
    only = LN.LoneNoise(lone, model, seed, t['thr_zle'], p['baseline'], p['n_tpc'], photons=False)
    assert p['baseline'] - SPIKE < t['thr_zle'][0] <= p['baseline'] - SMALL
    return cfg, p, both, only


def _key(rows):
    return [(r['channel'], r['left'], r['right'], r['n_photons'], r['n_noise'], tuple(r['starts'].tolist()), tuple(r['kinds'].tolist())) for r in rows]


# ---------------------------------------------------------------------------------------------------- the restatement
def test_chains_never_straddle_a_row(world):
    """rows of the shortest length a row with a pulse can have, dropped every 700 samples: seeds at row_lo - 1 and row_hi + 1 are never
    one chain (LoneNoise.rows asserts it for every chain), every crossing outside the rows is a seed of exactly one lone row, every
    seed a hit of its row (asserted there too), clipped rows touch no row"""
    cfg, p, ln, _ = world
    G = ln.G
    rows = [(a, a + G - 1) for a in range(1000, 60000, 700)]
    ln.prime(5, -G, 60000 + REACH + ln.tlen)
    got = ln.rows(5, 0, 60000, 60000 + REACH, rows)
    assert len(got) > 80
    cross = ln.crossings(5, 0, 60000)
    outside = [int(t) for t in cross if not any(l <= t <= r for l, r in rows)]
    in_rows = sorted(int(s) for r in got for s, k in zip(r['starts'], r['kinds']) if k == LN.NOISE and s < 60000)
    assert in_rows == outside and 20 < len(outside) < len(cross)
    # seeds on the two sides of one row, directly at it: two chains
    at_lo = {l - 1 for l, r in rows} & set(outside)
    at_hi = {r + 1 for l, r in rows} & set(outside)
    assert at_lo or at_hi
    clipped = 0
    for r in got:
        assert r['left'] <= r['starts'][0] and r['right'] >= r['starts'][-1]
        assert not any(r['left'] <= b and r['right'] >= a for a, b in rows)
        assert all(np.diff(r['starts']) <= G)
        clipped += int(r['left'] > r['starts'][0] - ln.tw or r['right'] < r['starts'][-1] + ln.tlen - 1 + ln.tw)
    assert clipped >= 10
    firsts, lasts = [r['starts'][0] for r in got], [r['starts'][-1] for r in got]
    assert all(f - l > G for f, l in zip(firsts[1:], lasts[:-1]))


def test_a_dark_pulse_that_crosses_seeds_its_own_samples(world):
    """the crossing samples of a lone photon's pulse never start before the photon, so the first start of its chain does not move; they
    can start later, so a row may be up to tlen - 1 samples longer than the same row of tests/lone_hits.py"""
    cfg, p, ln, _ = world
    ln.prime(5, -ln.G, 30000 + REACH + ln.tlen)
    mine = ln.rows(5, 0, 30000, 30000 + REACH)
    theirs = {int(r['starts'][0]): r for r in ln.lone.rows(5, 0, 30000, 30000 + REACH)}
    longer = 0
    for r in mine:
        ph = r['starts'][r['kinds'] == LN.PHOTON]
        if len(ph) and r['starts'][0] == ph[0] and int(ph[0]) in theirs and r['n_photons'] == theirs[int(ph[0])]['n_photons']:
            nz = r['starts'][r['kinds'] == LN.NOISE]
            if len(nz) and nz.max() < ph.max() + ln.tlen:
                assert r['left'] == theirs[int(ph[0])]['left'] and 0 <= r['right'] - theirs[int(ph[0])]['right'] <= ln.tlen - 1
                longer += int(r['right'] > theirs[int(ph[0])]['right'])
    assert longer >= 5


def test_a_pass_split_anywhere_gives_the_rows_of_one_pass(world):
    cfg, p, ln, only = world
    a, n = 90540 - 1000, 2000
    rows = [(a + 600, a + 600 + ln.G + 30)]
    for w, ch in ((ln, 5), (only, 6)):
        w.prime(ch, a - ln.G - ln.tlen, a + n + 300 + ln.tlen)
        whole = _key(w.rows(ch, a, a + n, a + n + 300, rows))
        assert len(whole) >= 1 and sum(k[4] for k in whole) >= 2 and (w is only or len(whole) >= 3)
        for cut in range(a, a + n + 1):
            parts = _key(w.rows(ch, a, cut, a + n + 300, rows)) + _key(w.rows(ch, cut, a + n, a + n + 300, rows))
            assert parts == whole, (ch, cut)
    multi = [r for r in ln.rows(5, a, a + n, a + n + 300, rows) if len(r['starts']) >= 2 and r['starts'][1] > r['starts'][0]]
    assert multi           # the awkward cuts are among them: inside a chain, one sample behind a chain's first seed


def test_no_seeds_where_none_are_due(world):
    cfg, p, ln, only = world
    assert ln.channels == N_MODEL
    assert only.rows(N_MODEL, 0, 50000, 50000) == [] and only.rows(300, 0, 50000, 50000) == []      # beyond the model's channels
    assert len(only.rows(6, 0, 50000, 50000)) > 50
    deep = LN.LoneNoise(ln.lone, ln.model, ln.seed, np.full(494, p['baseline'] - SPIKE), p['baseline'], p['n_tpc'], photons=False)
    assert deep.rows(6, 0, 50000, 50000) == [] and len(deep.crossings(6, 0, 50000)) == 0            # no value of the pmf is below that threshold
    assert int(only.noise(6, 0, 50000).min()) == -SPIKE


# ---------------------------------------------------------------------------------------------------- the oracle pin
@pytest.fixture(scope='module')
def designed(world):
    cfg, p, ln, only = world
    tab = LN.seed_table(ln, range(N_MODEL), 0, SCAN)
    tab_only = LN.seed_table(only, range(N_MODEL), 0, 4 * SCAN)
    G = ln.G
    return {'isolated': (ln, LN.find_isolated(tab, 400)), 'gap_G': (only, LN.find_pair(tab_only, G, 150)), 'gap_G1': (only, LN.find_pair(tab_only, G + 1, 150)),
            'inside_pulse': (ln, LN.find_inside_pulse(ln, tab)), 'needs_both': (ln, LN.find_needs_both(ln, tab))}


def _stretch_rows(w, ch, at):
    a, n = at - 1000, 3000
    w.prime(ch, a - w.G - w.tlen, a + n + REACH + w.tlen)
    rows = w.rows(ch, a, a + n, a + n + REACH)
    assert rows and all(r['right'] < a + n + REACH - 1 for r in rows)
    return rows


def test_designed_stretches_hold_their_seams(world, designed):
    cfg, p, ln, only = world
    G = ln.G
    w, (ch, at) = designed['isolated']
    row = [r for r in _stretch_rows(w, ch, at) if at in r['starts'].tolist()][0]
    assert row['n_noise'] == 1 and row['n_photons'] == 0 and (row['left'], row['right']) == (at - ln.tw, at + ln.tlen - 1 + ln.tw)
    w, (ch, at) = designed['gap_G']
    row = [r for r in _stretch_rows(w, ch, at) if at in r['starts'].tolist()][0]
    assert row['starts'].tolist() == [at, at + G] and row['n_noise'] == 2                                # one row
    w, (ch, at) = designed['gap_G1']
    rows = _stretch_rows(w, ch, at)
    ends, begins = [r for r in rows if r['starts'][-1] == at], [r for r in rows if r['starts'][0] == at + G + 1]
    assert len(ends) == 1 and len(begins) == 1 and begins[0]['left'] == ends[0]['right'] + 2      # two rows, one sample between them
    w, (ch, at) = designed['inside_pulse']
    row = [r for r in _stretch_rows(w, ch, at) if at in r['starts'].tolist()][0]
    assert row['n_photons'] >= 1 and row['n_noise'] >= 1
    w, (ch, at) = designed['needs_both']
    row = [r for r in _stretch_rows(w, ch, at) if at in r['starts'].tolist()][0]
    D, nz = int(w.dark(ch, at, 1)[0]), int(w.noise(ch, at, 1)[0])
    assert nz == -SMALL and -SMALL < D < 0 and p['baseline'] + D + nz < w.thr[ch]


@pytest.mark.parametrize('name', ['isolated', 'gap_G', 'gap_G1', 'inside_pulse', 'needs_both'])
def test_records_are_the_oracles(world, designed, name):
    """the restated rows of a stretch on the unchanged oracle, the model's samples as a noise table with a forced ix_rand: range,
    per-photon rounding, noise, ZLE and fragments byte for byte"""
    cfg, p, ln, only = world
    assert (p['store_before'] + p['samples_before']) % 2 == 0
    w, (ch, at) = designed[name]
    rows = _stretch_rows(w, ch, at)
    mine = w.records(rows, p['dt'])
    assert len(mine) >= 3 and any(at in r['starts'].tolist() for r in rows)
    off = {k: v for k, v in cfg.items() if k not in ('noise_model', 'noise_lone_hits')}
    orc_of = lambda table: make_oracle(dict(off, enable_noise=False) if table is None else dict(off, enable_noise=True, noise_data=table))
    theirs = LN.oracle_records(orc_of, rows, w, p)
    assert len(theirs) == len(mine) and theirs.tobytes() == mine.tobytes()


# ---------------------------------------------------------------------------------------------------- config, header
def test_config_key():
    cfg = model_config()
    del cfg['noise_lone_hits']
    plain = {k: v for k, v in cfg.items() if k != 'noise_model'}
    assert DC.noise_lone_hits_from(cfg) is False and DC.noise_lone_hits_from(dict(cfg, noise_lone_hits=False)) is False
    assert DC.noise_lone_hits_from(dict(cfg, noise_lone_hits=True)) is True
    assert DC.lone_hits_from(dict(cfg, noise_lone_hits=True)) is False                  # independent of 'dark_count_lone_hits'
    with pytest.raises(ValueError, match="noise_lone_hits: needs config\\['noise_model'\\]"):
        DC.noise_lone_hits_from(dict(plain, noise_lone_hits=True))
    with pytest.raises(ValueError, match='noise_lone_hits: enable_noise is off'):
        DC.noise_lone_hits_from(dict(cfg, noise_lone_hits=True, enable_noise=False))
    need = DC.lone_min_rext(kernel_params(cfg))
    assert need == 3080
    with pytest.raises(ValueError, match='noise_lone_hits: right_raw_extension 3079 ns below'):
        DC.noise_lone_hits_from(dict(cfg, noise_lone_hits=True, right_raw_extension=need - 1))
    assert DC.noise_lone_hits_from(dict(cfg, noise_lone_hits=True, right_raw_extension=need)) is True
    with pytest.raises(ValueError, match='dark_count_lone_hits: right_raw_extension 3079 ns below'):    # (the message still names its own key)
        DC.lone_hits_from(dict(cfg, dark_count_lone_hits=True, dark_count_rate=40.0, right_raw_extension=need - 1))


def test_header_declares_and_engine_lists_the_entry_points():
    from wfsim_amd import engine
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wfsim_amd.h')).read(), flags=re.S)
    for name in ('wfs_set_lone_noise_hits', 'wfs_copy_lone_row_noise_hits'):
        assert re.search(r'\bint\s+' + name + r'\s*\(\s*wfs_handle\s*\*', txt), name
        assert name in engine.EXPORTS
    assert hasattr(engine.Engine, 'set_lone_noise_hits') and hasattr(engine.Engine, 'lone_hit_noise_seeds')


# ---------------------------------------------------------------------------------------------------- the host pieces of wfs_lone.h
HOST_CASES = ['key', 'seed_clear', 'seed_range', 'straddle', 'blocks', 'check']


def test_host_rules_under_sanitizers(tmp_path_factory):
    """tests/host/lone_noise_rules_main.cpp: a program of its own, built with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes, run on the CPU"""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('lone_noise_rules') / 'lone_noise_rules_main')
    cmd = [cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-g', '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'), '-o', exe,
           os.path.join(ROOT, 'tests', 'host', 'lone_noise_rules_main.cpp')]
    if subprocess.run(cmd + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    q = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert q.returncode == 0, (q.returncode, q.stdout, q.stderr)
    lines = [ln.split() for ln in q.stdout.splitlines()]
    assert [ln[0] for ln in lines] == HOST_CASES and all(ln[1:] == ['ok'] for ln in lines), lines
