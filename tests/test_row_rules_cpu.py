"""The rules of the back end of a row (wfsim_amd/csrc/wfs_rows.h) on the host alone, against the reference's own output:
tests/host/rows_main.cpp is compiled against the header with the host compiler (with the address and undefined-behaviour sanitizers
where the compiler has their runtimes: the program stands alone) and run.

For every family of tests/golden/zle_edges.npz the test writes one line per finished row of the reference -- length, trigger window,
absolute first sample, channel, dt, the positions of the hits (data < Family.threshold(channel)) -- and the program groups the hits
with zle_holdoff, closes every interval with zle_window, counts the slots with zle_slots and makes the header of every record with
rec_header.  What it prints is compared HERE with the reference's ZLE tuples (all 499 rows of all 14 families, none left out) and with
the records zle_edges.expected_records makes of them, field by field.  The rules that need no rows -- the record geometry, the noise
index walked as the kernels walk it, the finished sample and the resident rule on its domain, the 32-bit threshold, the padded length
of a finished row -- are checked by the program itself on values worked out by hand from rawdata.py:398-458 and strax_interface.py:
391-436; so are the bits of the sort keys (bits_below; the end bits of the record sort and the lone seed sort and the key fields of the
overlay against the loops they replaced, which the program writes out).  The last test holds that the kernels and the engine no longer write any of these rules out."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import zle_edges as ZE
from tests.test_zle_edges_reference import case_rows, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'wfsim_amd', 'csrc')
SELF_CASES = ['geometry', 'noise_index', 'finish', 'padded_len', 'key_bits']
N_ROWS, N_RECORDS = 499, 2499


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = str(tmp_path_factory.mktemp('rows') / 'rows_main')
    cmd = [cxx, '-std=c++17', '-Wall', '-Werror', '-O2', '-I', CSRC, '-o', out, os.path.join(ROOT, 'tests', 'host', 'rows_main.cpp')]
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:      # (no sanitizer runtimes: the plain build must succeed)
        subprocess.check_call(cmd)
    return out


def _run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return [ln.split() for ln in p.stdout.splitlines()]


@pytest.fixture(scope='module')
def self_checks(exe):
    lines = _run(exe)
    assert [ln[0] for ln in lines] == SELF_CASES
    return {ln[0]: ln[1:] for ln in lines}


@pytest.mark.parametrize('case', SELF_CASES)
def test_case(self_checks, case):
    assert self_checks[case] == ['ok'], self_checks[case]


@pytest.fixture(scope='module')
def families(exe, tmp_path_factory):
    """per family: the reference's rows, and per row what the program made of its hits: slots, [(left, right, records)], {interval: [header dwords]}"""
    tmp = tmp_path_factory.mktemp('row_cases')
    out = {}
    for name in ZE.FAMILIES:
        a, cfg, fam, rows, index = fixture(name)
        path = str(tmp / (name + '.txt'))
        with open(path, 'w') as f:
            for row in rows:
                hits = np.flatnonzero(row['data'] < fam.threshold(row['channel']))
                f.write(' '.join(str(int(x)) for x in [len(row['data']), fam.tw, row['abs'], row['channel'], fam.dt, *hits]) + '\n')
        got = [dict(slots=None, itv=[], rec={}) for _ in rows]
        verdict = {}
        for ln in _run(exe, 'rows', path):
            if ln[0] == 'row':
                got[int(ln[1])]['slots'], got[int(ln[1])]['count'] = int(ln[2]), int(ln[3])
            elif ln[0] == 'itv':
                assert int(ln[2]) == len(got[int(ln[1])]['itv'])
                got[int(ln[1])]['itv'].append(tuple(int(x) for x in ln[3:6]))
            elif ln[0] == 'rec':
                recs = got[int(ln[1])]['rec'].setdefault(int(ln[2]), [])
                assert int(ln[3]) == len(recs)
                recs.append([int(x) for x in ln[4:10]])
            else:
                verdict[ln[0]] = ln[1:]
        assert verdict == {'intervals': ['ok'], 'records': ['ok']}, (name, verdict)
        out[name] = (a, fam, rows, index, got)
    return out


def test_intervals(families):
    """left, right and records of every interval of every row: the reference's tuples; no row needs more than its reserved slots and the
    rows the fixture designed to fill them do"""
    n_rows = n_rec = n_tight = 0
    for name, (a, fam, rows, index, got) in families.items():
        assert fam.hold == max(2 * fam.tw + 1, 1)
        for r, (row, g) in enumerate(zip(rows, got)):
            assert [(l, rr) for l, rr, _ in g['itv']] == row['intervals'], (name, r, row['window'], row['channel'])
            assert [n for _, _, n in g['itv']] == [max(0, -(-(rr - l + 1) // ZE.WFS_SPR)) for l, rr in row['intervals']], (name, r)
            assert g['count'] == len(row['intervals']) <= g['slots'] == (len(row['data']) + fam.hold) // (fam.hold + 1), (name, r)
            n_rows += 1
            n_rec += sum(n for _, _, n in g['itv'])
        for case, row, he_row, ix in case_rows(name):
            g = got[index[(case['window'], case['channel'])]]
            fills = ZE.measure(fam, case, row, he_row, ix)['fills_reserved_slots']
            assert fills == (g['count'] == g['slots']), (name, case['name'])
            if case['name'] == 'tightest_row':
                assert fills, name
                n_tight += 1
        assert sum(len(g['itv']) for g in got) == len(a['zle_ch']), name
    assert n_rows == N_ROWS and n_rec == N_RECORDS and n_tight >= 1
    assert n_rec == sum(len(ZE.expected_records(a)) for a, *_ in families.values())


def test_records(families):
    """the header of every record of every interval, through the shared definition, read back with the record dtype: time, length, dt,
    channel, pulse_length, record_i (and baseline 0) of zle_edges.expected_records; an empty interval (family tw0) makes none"""
    from wfsim_amd.dtypes import raw_record_dtype
    header = np.dtype(raw_record_dtype()[:-1])
    assert header.itemsize == 24 and np.dtype(raw_record_dtype()).itemsize == 244
    n = empty = 0
    for name, (a, fam, rows, index, got) in families.items():
        exp = ZE.expected_records(a, fam.dt)
        seen = {}
        words = []
        for k in range(len(a['zle_ch'])):               # the tuples in the order the reference yielded them: the k-th of its row
            r = index[(int(a['zle_digit'][k]), int(a['zle_ch'][k]))]
            j = seen.get(r, 0)
            seen[r] = j + 1
            l, rr, nrec = got[r]['itv'][j]
            assert len(got[r]['rec'].get(j, [])) == nrec
            empty += rr - l + 1 <= 0
            assert nrec > 0 or rr - l + 1 <= 0
            words += got[r]['rec'].get(j, [])
        mine = np.frombuffer(np.asarray(words, dtype=np.uint32).reshape(-1, 6).tobytes(), dtype=header)
        assert len(mine) == len(exp), name
        for field in ('time', 'length', 'dt', 'channel', 'pulse_length', 'record_i', 'baseline'):
            assert np.array_equal(mine[field], exp[field]), (name, field, int(np.flatnonzero(mine[field] != exp[field])[0]))
        n += len(mine)
    assert n == N_RECORDS and empty >= 1
    assert any(rr - l + 1 <= 0 for g in families['tw0'][4] for l, rr, _ in g['itv'])


def test_noise_index_on_the_rows_of_the_fixture(exe, tmp_path):
    """the rows of the short-table families -- one, two and three table lengths long -- walked from every start in steps of 64, 256 and
    WFS_SPR: (ix + i) % noise_len at every sample"""
    lines, wraps = [], set()
    for name in ('n512', 'n513', 'n700'):
        a, cfg, fam, rows, index = fixture(name)
        for row in rows:
            lines.append(f'{fam.N} {len(row["data"])}')
            wraps.add(len(row['data']) // fam.N)
    assert wraps >= {1, 2, 3}
    path = tmp_path / 'noise_rows.txt'
    path.write_text('\n'.join(lines) + '\n')
    assert _run(exe, 'noise', str(path)) == [['noise_index', 'ok']]


def _code(name):
    return re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, name)).read())


def test_row_rules_are_written_once():
    """no kernel and no host function keeps a copy of a rule of wfs_rows.h"""
    sources = [n for n in os.listdir(CSRC) if n.endswith(('.h', '.hip'))]
    assert 'wfs_rows.h' in sources
    gone = ['2 * (i64)d.tw + 1', '+ 1 + 2 * (i64)d.tw', '- 1) / WFS_SPR', '- 1) / spr', '24 + 2 *', '>= (u32)d.noise_len ?', 'close_interval', '>= 63',
            '__builtin_elementwise_add_sat', 'thr > 0x7fffffffLL']
    for name in sources:
        if name == 'wfs_rows.h':
            continue
        src = _code(name)
        for text in gone:
            assert text not in src, (name, text)
        assert not re.search(r'(len\w*|0xfffff\))\s*\+ 3\) & ~', src), name             # the padded length of a row
        assert not re.search(r'\bi32\s+finish_value\b', src), name
    for name in ('wfs_kernels.h', 'wfs_tilegen.h'):
        assert '+ 3) & ~' not in _code(name), name
    rows = _code('wfs_rows.h')
    for text in ('2 * tw + 1', '- 1) / WFS_SPR', 'in >= noise_len ?', '+ 3) & ~3', '(len + hold) / (hold + 1)', '(l + 1) / 2 * 2'):
        assert rows.count(text) == 1, text
    eng = _code('wfs_engine.hip')
    body = eng[eng.index('int wfs_copy_interval_data('):]
    body = body[:body.index('WFS_CATCH')]
    assert 'REC_LENGTH_BYTE' in body and 'REC_DATA_BYTE' in body and not re.search(r'WFS_RECORD_BYTES\s*\+\s*\d', body) and not re.search(r'\+\s*(8|24)\s*\]', body)
    ker = _code('wfs_kernels.h')
    assert ker.count('zle_window(') == 2 and 'ZLE_FAST_HOLD' in ker and 'ZLE_FAST_HOLD' in eng
    assert 'row_span(' in ker[ker.index('void k_row_len('):ker.index('void k_row_len(') + 6000] and 'row_span(' in ker[ker.index('void k_sum_signal('):ker.index('void k_row_pulse(')]
    assert 'row_span(' in eng[eng.index('int wfs_copy_sum_signal('):eng.index('int wfs_copy_sum_signal(') + 3000]
