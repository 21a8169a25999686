"""The designed cases of tests/tile_rows.py on the oracle alone (CPU): rows that the device reads in place from the tile buffers of
k_s2_tile and k_s2_bright.  tests/test_zle_edges_reference.py pins the oracle on the reference at these very seams; here every case must
reach its seam ACCORDING TO THE ORACLE'S OUTPUT on a row whose samples the tile generator made, so that device bytes equal to oracle
bytes (tests/test_gpu_tile_rows.py) are a pin with the seam reached by construction.

  * the threshold condition: the table without spikes gives no interval on any case row, and the hit level lies more than 3 counts
    below the deepest pulse sample of any row
  * every case of every (source, family) reaches its seam; a case no row qualifies for fails (nothing is dropped silently)
  * the stand-alone interval finder agrees with the oracle on every case row
  * the row-end and clip-edge cases carry spikes in the cells just BEHIND the row, for every (L % 4, acc_off % 4): cells the oracle never
    reads and that would be hits if the device looked at them (the tail test of k_zle's nibble)
  * COVERAGE, frozen: per source the rows that reach each seam and each (L % 4, acc_off % 4) class over the six trigger-window families
  * the noise-free case (special_thresholds per channel): the table of what it reaches, frozen
"""
import numpy as np
import pytest

from tests import tile_rows as TR
from tests import zle_edges as ZE
from tests.helpers import make_oracle
from wfsim_amd.config import kernel_params

PAIRS = [(s, f) for s in TR.SOURCES for f in TR.FAMILIES]
TW_FAMILIES = [f for f in TR.FAMILIES if f.startswith('tw')]

# Per source, over the six trigger-window families: the longest row (tw = 50), cases whose hit pair straddles each seam (first hit below
# the seam, second at or beyond it), and the (L % 4, acc_off % 4) classes with hits on sample 0 and L - 1.  Mandatory on k_s2_tile rows
# (tile_shallow + tile_deep) and on k_s2_bright rows (bright + bright_deep): the 16 classes and the seams 64 .. 768.  Seam 1024 is
# reached on k_s2_tile rows only, 2048 on none.  bright_fits admits about 1596 start bins (128 KB of H table); at that limit a bright row
# would be about 1030 samples.  bright_deep keeps a margin (BRIGHT_MAX_BINS) so that it fits whatever LDS the device grants, and a pair
# is placed at a seam only where ten rows hold seam + gap + 1 samples: 1024 is out of reach by that margin and that rule.
COVERAGE = {
    'tile_shallow': {'longest': 567, 'seams': {64: 38, 256: 46}, 'classes': 16},
    'tile_deep': {'longest': 1228, 'seams': {64: 38, 256: 46, 512: 46, 768: 46, 1024: 46}, 'classes': 16},
    'bright': {'longest': 662, 'seams': {64: 38, 256: 46, 512: 46}, 'classes': 16},
    'bright_deep': {'longest': 885, 'seams': {64: 38, 256: 46, 512: 46, 768: 46}, 'classes': 16},
    'mixed_window': {'longest': 567, 'seams': {64: 38, 256: 46}, 'classes': 16},
    'three_windows': {'longest': 642, 'seams': {64: 38, 256: 46, 512: 46}, 'classes': 16},
}
# Cases per (source, family), frozen: a case group is left out where the tenth-longest row of a source is too short for it (pairs at a
# seam, three hits at 1024, fragment lengths, interval counts), so a change of source that loses some changes these numbers.
CASES = {
    'tile_shallow': {'tw0': 80, 'tw1': 89, 'tw10': 87, 'tw31': 83, 'tw32': 80, 'tw50': 79, 'n700': 79, 'n513': 79, 'n100': 87, 'nfloat': 79, 'he801': 84, 'sum801': 79},
    'tile_deep': {'tw0': 102, 'tw1': 121, 'tw10': 115, 'tw31': 112, 'tw32': 108, 'tw50': 107, 'n700': 107, 'n513': 107, 'n100': 115, 'nfloat': 107, 'he801': 112, 'sum801': 107},
    'bright': {'tw0': 87, 'tw1': 99, 'tw10': 96, 'tw31': 93, 'tw32': 89, 'tw50': 88, 'n700': 88, 'n513': 88, 'n100': 96, 'nfloat': 88, 'he801': 93, 'sum801': 88},
    'bright_deep': {'tw0': 93, 'tw1': 110, 'tw10': 104, 'tw31': 101, 'tw32': 97, 'tw50': 96, 'n700': 96, 'n513': 96, 'n100': 104, 'nfloat': 96, 'he801': 101, 'sum801': 96},
    'mixed_window': {'tw0': 109, 'tw1': 124, 'tw10': 121, 'tw31': 115, 'tw32': 107, 'tw50': 105, 'n700': 105, 'n513': 105, 'n100': 121, 'nfloat': 105, 'he801': 110, 'sum801': 105},
    'three_windows': {'tw0': 87, 'tw1': 99, 'tw10': 96, 'tw31': 93, 'tw32': 89, 'tw50': 88, 'n700': 88, 'n513': 88, 'n100': 96, 'nfloat': 88, 'he801': 93, 'sum801': 88},
}
MANDATORY = {'k_s2_tile': (('tile_shallow', 'tile_deep'), (64, 256, 512, 768, 1024)), 'k_s2_bright': (('bright', 'bright_deep'), (64, 256, 512, 768))}


def _coverage(source):
    seams, classes, longest = {}, set(), 0
    for family in TW_FAMILIES:
        fam, cfg, orc, o = TR.oracle_run(source, family)
        rows = TR.finished_rows(o)
        for case, r in fam.case_rows():
            if case['pool'] != 'direct':
                continue
            row_abs, data, itv = rows[(case['window'], case['channel'])]
            m = TR.measure(fam, case, data, itv)
            longest = max(longest, m['length'])
            if case['expect'].get('seam') and m.get('seam') == case['expect']['seam']:
                seams[m['seam']] = seams.get(m['seam'], 0) + 1
            if case['name'].startswith('ends_') and m['hits'] == (0, m['length'] - 1):
                classes.add((m['len_mod4'], m['acc_mod4']))
    return dict(longest=longest, seams=dict(sorted(seams.items())), classes=len(classes))


def test_the_restatement_of_the_buffer_layout():
    """what buffer_caps and the expected tile kinds take from the device code, checked against the oracle's own tables and counts"""
    for source in TR.SOURCES:
        g = TR.geometry(source, 'tw50')
        assert np.array_equal(g['fused'], g['sched']['s_ins']['type'] == 2) and np.array_equal(g['cap'] > 0, g['fused']), source
        e = g['o']['e_t']
        if source in TR.KERNEL:
            n = g['sizes'][g['sizes'] > 0]
            bright = TR.KERNEL[source] == 'k_s2_bright'
            assert (n.min() > TR.TILE_MAX_PHOTONS) if bright else (n.max() <= TR.TILE_MAX_PHOTONS), (source, n.min(), n.max())
            if bright:
                assert (int(e.max()) - int(e.min()) + TR.TABLE_SPAN) // 10 + 2 <= TR.BRIGHT_MAX_BINS, source
    orc = make_oracle(TR.family_config('tile_shallow', 'tw50'))
    assert len(orc.alias_pmf(8)[0]) == TR.TABLE_SPAN
    assert {c % 4 for c in TR.geometry('three_windows', 'tw50')['cap']} >= {1, 0} and all(TR.geometry(s, 'tw50')['cap'][0] % 2 for s in TR.KERNEL)


@pytest.mark.parametrize('source,family', PAIRS)
def test_background_alone_makes_no_interval(source, family):
    fam, cfg, orc, o = TR.oracle_run(source, family, spikes=False)
    assert fam.g['deepest'] - 3 >= fam.thr and fam.base - fam.g['deepest'] + 3 <= TR.ZLE, (fam.g['deepest'], fam.thr)
    rows = TR.finished_rows(o)
    assert len({(c['window'], c['channel']) for c in fam.cases}) == len(fam.cases) > 40
    case_rows = {(c['window'], c['channel']) for c in fam.cases if c['pool'] != 'he'}          # (an HE row is its top row times 20: the pulse makes hits there)
    bad = [k for k in case_rows if rows[k][2] or np.any(rows[k][1] < fam.thr)]
    assert not bad, (source, family, bad[:5])
    quiet = fam.table(spikes=False)
    assert np.abs(quiet).max() < 3 and np.any(quiet != 0)


@pytest.mark.parametrize('source,family', PAIRS)
def test_every_case_reaches_its_seam(source, family):
    fam, cfg, orc, o = TR.oracle_run(source, family)
    assert not fam.missing, (source, family, 'no row qualifies for', fam.missing)
    assert len(fam.cases) == CASES[source][family], (source, family, len(fam.cases))
    # the cells behind a row-end or clip-edge row (samples L .. ceil4(L) - 1) would be hits if anything read them; the oracle does not
    table, behind = cfg['noise_data'], [c for c in fam.cases if 'behind' in c]
    assert len(behind) >= 32 + (8 if fam.tw > 0 else 0) and {(c['length'] % 4, c['acc_mod4']) for c in behind if c['pool'] == 'direct'} == {(m, a) for m in range(4) for a in range(4)}
    for c in behind:
        assert len(c['behind']) == 4 - c['length'] % 4 and all(int(fam.base + table[j, c['channel']]) < fam.thr for j in c['behind']), (source, family, c['name'])
    assert o['dg_ix_rand'].tolist() == fam.ix.tolist()
    rows = TR.finished_rows(o)
    missed, n_itv, pools = {}, 0, {}
    for case, r in fam.case_rows():
        row_abs, data, itv = rows[(case['window'], case['channel'])]
        assert row_abs == r['abs'] and len(data) == r['L']
        bad = TR.check_case(fam, case, row_abs, data, itv)
        if fam.wraps and not TR.measure(fam, case, data, itv)['wraps']:
            bad.append(('the row does not wrap',))
        if TR.standalone_intervals(fam, data) != itv:
            bad.append(('stand-alone finder', TR.standalone_intervals(fam, data)[:3], itv[:3]))
        if bad:
            missed[case['name']] = bad
        n_itv += len(itv)
        pools[case['pool']] = pools.get(case['pool'], 0) + 1
    assert not missed, (source, family, missed)
    if source == 'mixed_window':
        assert pools.get('shared', 0) >= 20 and pools['direct'] >= 40, pools
    if family == 'he801':
        assert pools.get('he', 0) == 5, pools
    if family == 'sum801':
        assert all(c['channel'] >= fam.n_top for c in fam.cases if c['pool'] == 'direct')          # (the oracle makes no sum row: tests/sum_signal.py restates it)
        sums = TR.expected_sum_rows(o, kernel_params(cfg), orc.tables['thr_zle'], noise=cfg['noise_data'], ix_rand=fam.ix)
        assert len(sums) == len(fam.ix) and all(len(e['intervals']) >= 1 for e in sums) and fam.sum_spikes()
        assert {c['acc_mod4'] for c in fam.cases if c['pool'] == 'direct'} == {0, 1, 2, 3}
    if source == 'three_windows':
        last = max(k for k, r in fam.g['rows'].items() if r['ch'] < fam.n_tpc and r['window'] == 2)
        assert any((c['window'], c['channel']) == last for c in fam.cases)
    print(f'\n{source} / {family}: {len(fam.cases)} cases {pools}, {n_itv} intervals on them; {len(o["zl_ch"])} intervals in all')


@pytest.mark.parametrize('source', list(TR.SOURCES))
def test_coverage_is_the_frozen_table(source):
    got = _coverage(source)
    print(f'\n    {source!r}: {got},')
    assert got == COVERAGE[source], (source, got)
    for s in ZE.SEAMS:
        if s not in got['seams']:
            print(f'{source}: no row reaches seam {s} (longest row {got["longest"]})')


def test_mandatory_coverage():
    for kernel, (sources, seams) in MANDATORY.items():
        for s in seams:
            assert sum(COVERAGE[src]['seams'].get(s, 0) for src in sources) >= 8, (kernel, s)
        assert all(COVERAGE[src]['classes'] == 16 for src in sources), kernel
    assert all(2048 not in COVERAGE[src]['seams'] and COVERAGE[src]['longest'] < 2048 for src in COVERAGE)          # stated in DESIGN.md 5
    assert COVERAGE['mixed_window']['classes'] == 16 and COVERAGE['three_windows']['classes'] == 16


# What the noise-free case reaches (source -> rows with 1 / 2 / 3+ hits, distinct hit positions mod 64 and mod 256, landing parities
# (row start, raw left, raw right) met, (L % 4, acc_off % 4) classes).  Pair gaps are reported by the test, not required.
NOISELESS = {
    'tile_shallow': {'rows': {1: 162, 2: 157, 3: 175}, 'mod64': 64, 'mod256': 172, 'parities': 8, 'classes': 16},
    'bright': {'rows': {1: 165, 2: 162, 3: 167}, 'mod64': 64, 'mod256': 92, 'parities': 8, 'classes': 16},
}


@pytest.mark.parametrize('source', TR.NOISELESS)
def test_noiseless_thresholds(source):
    cfg, hits = TR.noiseless_config(source)
    g = TR.geometry(source, 'tw50')
    s = g['sched']
    orc = make_oracle(cfg)
    orc.simulate(s['s_ins'], s['gid'], s['ip'])
    o = orc.results()
    rows = TR.finished_rows(o)
    tw = 50
    n_hits, mod64, mod256, parities, classes, gaps = {}, set(), set(), set(), set(), set()
    for ch, h in hits.items():
        row_abs, data, itv = rows[(0, ch)]
        r = g['rows'][(0, ch)]
        assert np.array_equal(data, r['data']) and len(h) >= 1 and len(itv) >= 1, ch
        assert len(itv) == 1 or h[-1] - h[0] > 2 * tw + 1, ch
        n_hits[min(len(h), 3)] = n_hits.get(min(len(h), 3), 0) + 1
        mod64 |= {i % 64 for i in h}
        mod256 |= {i % 256 for i in h}
        parities.add((row_abs % 2, (h[0] - tw) % 2, (h[-1] + tw) % 2))
        classes.add((r['L'] % 4, r['acc_mod4']))
        gaps |= set(np.diff(h).tolist())
    other = [k for k in rows if k[1] not in hits and rows[k][2]]
    assert not other, other[:5]
    got = dict(rows=dict(sorted(n_hits.items())), mod64=len(mod64), mod256=len(mod256), parities=len(parities), classes=len(classes))
    print(f'\n    {source!r}: {got},\n{source}: gaps between the hits of a row: {sorted(gaps)[:12]}')
    assert got == NOISELESS[source], (source, got)
