"""The owning device buffer and the typed array on top of it (wfsim_amd/csrc/wfs_devbuf.h) on the host alone: tests/host/devbuf_main.cpp is compiled against the
header with the host compiler and run; a counting malloc / free pair plays hipMalloc / hipFree, and a set of the live blocks
turns a double free into a failed case instead of a crash.

The program prints one line per case; every case also checks that the header's counters of live buffers agree with the
allocator's.  The same program is built a second time with the address and undefined-behaviour sanitizers: a double free or a
use after a move that the bookkeeping missed ends that run with a report."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['ensure_grows', 'scope_end_frees', 'capacity_rule', 'grow_frees_old_once', 'failed_alloc_leaves_empty', 'move',
         'move_scope_end', 'reset_twice', 'vector', 'vector_scope_end', 'struct', 'struct_scope_end',
         'arr_sizes', 'arr_grow', 'arr_move', 'arr_scope_end']


def _compiler():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    return cxx


def _build(tmp_path_factory, name, extra):
    cxx = _compiler()
    exe = str(tmp_path_factory.mktemp(name) / 'devbuf_main')
    subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror', *extra, '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'),
                           '-o', exe, os.path.join(ROOT, 'tests', 'host', 'devbuf_main.cpp')])
    return exe


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    return {ln[0]: ln[1:] for ln in lines}


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    return _run(_build(tmp_path_factory, 'devbuf', ['-O2']))


@pytest.mark.parametrize('case', CASES)
def test_case(results, case):
    assert results[case][0] == 'ok', results[case]


def test_nothing_left_at_the_end(results):
    last = dict(f.split('=') for f in results[CASES[-1]][1:])
    assert int(last['live']) == 0 and int(last['bytes']) == 0 and int(last['allocs']) == int(last['frees']) > 0


def test_under_sanitizers(tmp_path_factory):
    # the runtimes linked into the program: it then runs whatever else the environment loads into a process first
    static = ['-static-libsan'] if 'clang' in os.path.basename(_compiler()) else ['-static-libasan', '-static-libubsan']
    r = _run(_build(tmp_path_factory, 'devbuf_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static]))
    assert all(v[0] == 'ok' for v in r.values()), r


def _calls(src, name):
    """The argument lists of every call name(...) in src, split at the top-level commas."""
    out = []
    for m in re.finditer(r'\b%s\(' % name, src):
        depth, args, cur, i = 0, [], '', m.end() - 1
        while True:
            c = src[i]
            if c in '([{':
                depth += 1
                cur += c if depth > 1 else ''
            elif c in ')]}':
                depth -= 1
                if depth == 0:
                    break
                cur += c
            elif c == ',' and depth == 1:
                args.append(cur.strip())
                cur = ''
            else:
                cur += c
            i += 1
        out.append(args + [cur.strip()])
    return out


def test_element_types_stand_in_the_declarations():
    """wfs_engine.hip: a buffer's element type is named where it is declared and nowhere else.  A cast of a buffer (.as<T>) is left
    on the byte-typed ones alone, and no size handed to ensure / upload restates an element size."""
    src = re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_engine.hip')).read())
    casts = re.findall(r'([\w\[\]>\-\.\(\)]+)\.as<', src)
    assert casts and all(re.search(r'(sort_tmp|records_ab\[\w+\]|records_buf\(\))$', c) for c in casts), casts
    assert not re.search(r'\bDevBuf\s+(?!sort_tmp\b|records_ab\b|&records_buf\b)\w', re.sub(r'const DevBuf [&*]\w+', '', src))
    sized = _calls(src, 'ensure') + _calls(src, 'upload')
    assert len(sized) > 150
    for args in sized:
        assert not re.search(r'\*\s*[48]\b|\b[48]\s*\*|sizeof', args[-1]), args
    for args in _calls(src, 'ensure_each')[1:]:                 # (the first is the definition; the count stands in front of the arrays)
        assert not re.search(r'\*\s*[48]\b|\b[48]\s*\*|sizeof', args[1]), args
