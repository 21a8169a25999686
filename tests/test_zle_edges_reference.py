"""The CPU oracle on reference runs of rows DESIGNED sample by sample (tests/golden/zle_edges.npz; case table, noise-table builder and
coverage function in tests/zle_edges.py; made by tests/golden/make_golden.py zle_edges).  CPU only.

Per family (a trigger window / threshold / HE configuration with its own noise table): the oracle replays the reference's photons with
the designed noise start indices and must give the reference's finished rows, ZLE tuples and -- through a numpy restatement of
strax_interface.py:425-435 on the reference's tuples -- the bytes of pack_records(); every case must reach the seam it was designed
for ACCORDING TO THE REFERENCE'S OUTPUT, so a case that drifted off its seam fails instead of passing vacuously; and the stand-alone
find_intervals_below_threshold answers to the reference's tuples on every designed row.

The sample above 32767: the reference's ZLE tuple keeps 32768 (int64 samples); the record field is int16 and numpy's assignment keeps
the low 16 bits (-32768) -- restated in zle_edges.expected_records.  The chunker fixtures (tests/test_chunker_reference.py) pin that the
oracle's pack_records() is the reference's record layout on physics-shaped rows; no sample of theirs is that wide.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle, noise_high
from tests import zle_edges as ZE
from tests.helpers import golden, make_oracle, replay_chain_on_oracle, with_fma, zle_edges_config

_cache = {}


def fixture(name):
    """(the family's arrays, its config with the designed table as noise_data, the Family, the reference's rows, their index)"""
    if name not in _cache:
        a = ZE.family_arrays(golden('zle_edges.npz'), name)
        tab = golden('tables.npz')
        cfg0 = zle_edges_config(name)
        fam = ZE.family(name, cfg0, tab['templates'], float(tab['current_2_adc']))
        rows, index = ZE.rows_of(a)
        _cache[name] = (a, dict(cfg0, noise_data=fam.table()), fam, rows, index)
    return _cache[name]


def case_rows(name):
    """per case: (case, its row in the reference's output, its HE row or None, the window's ix_rand)"""
    a, cfg, fam, rows, index = fixture(name)
    out = []
    for case in fam.cases:
        he = index.get((case['window'], fam.he_first + case['channel']))
        out.append((case, rows[index[(case['window'], case['channel'])]], None if he is None else rows[he], int(a['dg_ix_rand'][case['window']])))
    return out


def test_the_fixture_holds_every_family():
    d = golden('zle_edges.npz')
    assert [str(x) for x in d['families']] == ZE.FAMILIES
    assert {f'tw{tw}' for tw in (0, 1, 10, 31, 32, 50)} <= set(ZE.FAMILIES)
    holds = sorted(fixture(n)[2].hold for n in ZE.TW_FAMILIES)
    assert holds == [1, 3, 21, 63, 65, 101]


@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_tables_and_start_indices_are_ones_the_reference_takes(name):
    """the table the builder makes is the one the fixture was made with (shape; the generator asserted the reference loaded it), the
    designed ix_rand of every window is what the reference recorded and lies below the `high` of rawdata.py:407-417 computed from the
    reference's rows; a row wraps only where the window is longer than the table"""
    a, cfg, fam, rows, index = fixture(name)
    t = cfg['noise_data']
    assert t.shape == tuple(a['noise_shape']) == (fam.N, fam.columns) and t.dtype == (np.float64 if fam.float_table else np.int16)
    assert np.array_equal(a['dg_ix_rand'], fam.ix_rands()) and [str(x) for x in a['case_names']] == [c['name'] for c in fam.cases]
    assert len(set(c['name'] for c in fam.cases)) == len(fam.cases)
    assert np.all(np.abs(t[t != np.trunc(t)] - np.trunc(t[t != np.trunc(t)])) < 0.9)
    for g in range(len(a['dg_left'])):
        r0, r1 = int(a['dg_row_off'][g]), int(a['dg_row_off'][g + 1])
        n = r1 - r0
        high = noise_high(np.ones(n, np.uint8), a['row_left'][r0:r1], a['row_right'][r0:r1], fam.N)
        ix = int(a['dg_ix_rand'][g])
        assert 0 <= ix < high, (name, g, ix, high)
        span = int(a['row_right'][r0:r1].max() - a['row_left'][r0:r1].min())
        longest = int((a['row_right'][r0:r1] - a['row_left'][r0:r1]).max()) + 1
        if ix + longest > fam.N:
            assert span >= fam.N, (name, g)
    assert len(a['row_data']) and int((a['row_right'] - a['row_left']).max()) + 1 < 15000


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_oracle_replays_the_reference(name, fma):
    """finished rows, ZLE tuples and record bytes"""
    a, cfg, fam, rows, index = fixture(name)
    orc = make_oracle(with_fma(cfg, fma))
    orc.set_noise_override(a['dg_ix_rand'])
    r = replay_chain_on_oracle(orc, a)
    for x, y in [('pl_ch', 'pl_ch'), ('pl_left', 'pl_left'), ('pl_right', 'pl_right'), ('dg_left', 'dg_left'), ('dg_right', 'dg_right'), ('dg_ix_rand', 'dg_ix_rand'),
                 ('row_ch', 'row_ch'), ('row_left', 'row_left'), ('row_right', 'row_right'), ('row_data_off', 'row_data_off')]:
        assert np.array_equal(r[x], a[y]), (name, x)
    if not np.array_equal(r['row_data'], a['row_data']):
        bad = np.flatnonzero(r['row_data'] != a['row_data'])
        row = int(np.searchsorted(a['row_data_off'], bad[0], side='right') - 1)
        g = int(np.searchsorted(a['dg_row_off'], row, side='right') - 1)
        who = [c['name'] for c in fam.cases if c['window'] == g and c['channel'] in (int(a['row_ch'][row]), int(a['row_ch'][row]) - fam.he_first)]
        raise AssertionError(f'{name}: {len(bad)} row samples differ, first in window {g} channel {a["row_ch"][row]} sample {bad[0] - a["row_data_off"][row]} ({who})')
    for k in ['digit', 'ch', 'left', 'right', 'data_off', 'data']:
        if not np.array_equal(r['zl_' + k], a['zle_' + k]):
            n = min(len(r['zl_' + k]), len(a['zle_' + k]))
            j = int(np.flatnonzero(np.asarray(r['zl_' + k][:n]) != np.asarray(a['zle_' + k][:n]))[0]) if n and np.any(np.asarray(r['zl_' + k][:n]) != np.asarray(a['zle_' + k][:n])) else n
            j = min(j, len(a['zle_ch']) - 1) if k != 'data' else 0
            who = [c['name'] for c in fam.cases if k != 'data' and c['window'] == int(a['zle_digit'][j]) and c['channel'] == int(a['zle_ch'][j])]
            raise AssertionError(f'{name}: ZLE {k} differs ({len(r["zl_" + k])} against {len(a["zle_" + k])}), first at tuple {j} {who}')
    exp = ZE.expected_records(a, int(cfg.get('sample_duration', 10)))
    got = orc.pack_records()
    assert len(got) == exp.nbytes, (name, len(got) // 244, len(exp))
    if got.tobytes() != exp.tobytes():
        rec = np.frombuffer(got.tobytes(), dtype=exp.dtype)
        j = int(np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(rec, exp)])[0])
        who = [c['name'] for c in fam.cases if c['channel'] in (int(exp['channel'][j]), int(exp['channel'][j]) - fam.he_first)]
        raise AssertionError(f'{name}: record {j} differs (channel {exp["channel"][j]}, fragment {exp["record_i"][j]} of a pulse of {exp["pulse_length"][j]}) {who}')


@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_every_case_reaches_its_seam(name):
    """the coverage table, case by case, from the reference's own rows and tuples"""
    a, cfg, fam, rows, index = fixture(name)
    assert len(a['row_ch']) == len(fam.cases) * (2 if name.startswith('he') else 1)
    missed = {}
    for case, row, he_row, ix in case_rows(name):
        bad = ZE.check_case(fam, case, row, he_row, ix)
        if bad:
            missed[case['name']] = bad
    assert not missed, missed


def _measured(name):
    a, cfg, fam, rows, index = fixture(name)
    return fam, [(case, ZE.measure(fam, case, row, he_row, ix)) for case, row, he_row, ix in case_rows(name)]


@pytest.mark.parametrize('name', list(ZE.TW_FAMILIES))
def test_hold_off_families_cover_the_list(name):
    """what the issue lists for a trigger-window family is there, measured on the reference's output"""
    fam, ms = _measured(name)
    hold, tw = fam.hold, fam.tw
    gaps = [g for g in (hold - 1, hold, hold + 1, hold + 2) if g >= 1]
    assert gaps == ([1, 2, 3] if tw == 0 else [hold - 1, hold, hold + 1, hold + 2])
    pairs = {}
    for case, m in ms:
        h = m['hits']
        if case['name'].startswith('pairs_'):
            assert len(h) % 2 == 0 and not any(m['joined'][1::2])           # the pairs of a row stay apart
            for q in range(len(h) // 2):
                a, b = h[2 * q], h[2 * q + 1]
                for seam in ZE.SEAMS:
                    if a < seam <= b:
                        pairs.setdefault((b - a, seam), set()).add((m['joined'][2 * q], a == seam - 1, b == seam))
        if case['name'].startswith('pair_') and len(h) == 2 and m['same_chunk']:
            pairs.setdefault((h[1] - h[0], 'chunk'), set()).add((m['merged'], False, False))
    for gap in gaps:
        for seam in ZE.SEAMS:
            got = pairs.get((gap, seam), set())
            assert got and all(x[0] == (gap <= hold) for x in got), (name, gap, seam, got)
            assert any(x[1] for x in got), (name, gap, seam, 'a pair whose first hit is the last sample before the seam')
            if seam - gap >= 0:
                assert any(x[2] for x in got), (name, gap, seam, 'a pair whose second hit is the first sample behind the seam')
        if gap < ZE.CHUNK:
            assert (gap, 'chunk') in pairs, (name, gap)
    by = {case['name']: m for case, m in ms}
    for seam in (64, 1024):
        m = by[f'three_hits_seam{seam}']
        h = m['hits']
        assert len(h) == 3 and h[1] - h[0] == hold and h[2] - h[0] == 2 * hold and m['n_intervals'] == 1 and h[0] < seam <= h[2]
    # row ends
    assert {m['len_mod4'] for n, m in by.items() if n.startswith('ends_len_mod4_') and m['hits'][0] == 0 and m['hits'][-1] == m['length'] - 1} == {0, 1, 2, 3}
    assert by['no_hit']['n_intervals'] == 0 and by['no_hit']['hits'] == ()
    assert all(by[f'one_interval_end_to_end_{k}']['spans_row'] for k in (0, 1)) and {by[f'one_interval_end_to_end_{k}']['length'] % 2 for k in (0, 1)} == {0, 1}
    # even landing: all eight combinations, each one interval
    combos = {(m['start_parity'], m['raw_left_parity'], m['raw_right_parity']) for n, m in by.items() if n.startswith('landing_') and m['n_intervals'] == 1}
    assert len(combos) == 8
    if tw == 0:
        m = by['single_hit_odd_sample']
        assert m['hits'][0] % 2 == 1 and m['plens'] == (-1,) and m['n_records'] == 0          # left lands above right: an empty slice
    # record fragments: every length, and one at the very end of a row of each len % 4
    assert {m['plens'][0] for n, m in by.items() if n.startswith('fragments_') and m['n_intervals'] == 1} >= set(ZE.FRAGMENT_PLENS)
    assert {m['n_records'] for n, m in by.items() if n.startswith('fragments_')} >= {1, 2, 3, ZE.PACK_U, ZE.PACK_U + 1, 8, 9}
    assert {m['len_mod4'] for n, m in by.items() if n.startswith('fragments_') and m.get('ends_at_row_end')} == {0, 1, 2, 3}
    if tw == 31:
        assert [by[f'intervals_{n}']['n_intervals'] for n in ZE.INTERVAL_COUNTS] == list(ZE.INTERVAL_COUNTS)
        assert all(by[f'intervals_{n}']['length'] < 9000 for n in ZE.INTERVAL_COUNTS)
    if tw in (0, 31):
        m, nb = by['tightest_row'], by['tightest_row_neighbour']
        assert m['n_intervals'] == m['reserved'] == (m['length'] + hold) // (hold + 1) and m['hits'][0] == 0 and m['hits'][-1] == m['length'] - 1
        assert set(np.diff(m['hits']).tolist()) == {hold + 1}
        cases = {c['name']: c for c in fam.cases}
        assert cases['tightest_row_neighbour']['channel'] == cases['tightest_row']['channel'] + 1 and cases['tightest_row_neighbour']['window'] == cases['tightest_row']['window']
        assert nb['first_interval_at_row_start']
    # thresholds and the clamp
    assert by['pulse_peak_no_hit']['hits'] == () and len(by['pulse_peak_hit']['hits']) == 1
    if fam.special:
        assert by['noise_at_threshold_special']['n_intervals'] == 1 and fam.threshold(ZE.SPECIAL_CHANNEL) == fam.base - ZE.SPECIAL_THRESHOLD - 1 != fam.threshold(0)
        assert by['pulse_peak_no_hit_special']['hits'] == () and len(by['pulse_peak_hit_special']['hits']) == 1
        cases = {c['name']: c for c in fam.cases}
        assert {cases[n]['channel'] for n in ('noise_at_threshold_special', 'pulse_peak_no_hit_special', 'pulse_peak_hit_special')} == set(ZE.SPECIAL_CHANNELS)


@pytest.mark.parametrize('name', ['n512', 'n513', 'n700', 'n100', 'n511'])
def test_noise_index_families_cover_the_list(name):
    fam, ms = _measured(name)
    fast = name in ('n512', 'n513', 'n700')
    assert (fam.N >= ZE.NOISE_MIN_FAST) == fast
    assert {m['wraps'] for _, m in ms} >= {1, 2, 3}
    firsts = {m['first_wrap'] for _, m in ms}
    assert {w % 4 for w in firsts} == ({0, 1, 2, 3} if fast else {w % 4 for w in firsts}) and (not fast or any(w % ZE.BLOCK == 0 for w in firsts))
    if fast:
        pos = set().union(*[set(m['wrap_record_pos']) for _, m in ms])
        assert 0 in pos and ZE.WFS_SPR - 1 in pos, pos          # a wrap on the first and on the last sample of a record
    # the spike pattern is not periodic inside the table: no shift of a column reproduces it
    t = fixture(name)[1]['noise_data']
    for case, _ in ms:
        col = t[:, case['channel']].astype(np.int64)
        assert all(not np.array_equal(np.roll(col, s), col) for s in range(1, fam.N))
    # every row of these families does wrap, in a window longer than the table
    assert all(m['wraps'] >= 1 for _, m in ms)


def test_float_table_truncates_toward_zero_at_the_threshold():
    a, cfg, fam, rows, index = fixture('nfloat')
    t = cfg['noise_data']
    assert t.dtype == np.float64 and np.any(t != np.trunc(t))
    thr = fam.threshold(0)
    decided = 0
    for case, row, he_row, ix in case_rows('nfloat'):
        nz = t[(ix + np.arange(len(row['data']))) % fam.N, case['channel']]
        assert np.array_equal(row['data'], np.trunc(nz).astype(np.int64) + fam.base)            # (adc 0 everywhere: the weak pair)
        hit = row['data'] < thr
        decided += int(np.sum(hit != (np.floor(nz) + fam.base < thr))) + int(np.sum(hit != (np.around(nz) + fam.base < thr)))
        assert np.any(row['data'] == thr) and np.any(row['data'] == thr - 1)
    assert decided >= 10            # samples where floor or round-to-nearest would have decided otherwise


@pytest.mark.parametrize('name', ZE.FAMILIES)
def test_standalone_interval_finder_on_the_designed_rows(name):
    """Oracle.find_intervals_below_threshold on every finished row of the reference, then the window, the clip and the even landing of
    rawdata.py:302-308 in numpy: the reference's tuples"""
    a, cfg, fam, rows, index = fixture(name)
    n = 0
    for row in rows:
        raw = Oracle.find_intervals_below_threshold(row['data'], fam.threshold(row['channel']), 2 * fam.tw + 1)
        itv = raw.copy()
        itv[:, 0] -= fam.tw
        itv[:, 1] += fam.tw
        itv = np.clip(itv, 0, len(row['data']) - 1)
        itv[:, 0] = np.ceil(itv[:, 0] / 2.0) * 2
        itv[:, 1] = np.floor(itv[:, 1] / 2.0) * 2
        assert [tuple(x) for x in itv.tolist()] == row['intervals'], (name, row['window'], row['channel'])
        for (l, r), z in zip(row['intervals'], row['zle']):
            assert np.array_equal(z, row['data'][l:r + 1])
        n += len(itv)
    assert n == len(a['zle_ch'])
