"""The owning device buffer (wfsim_amd/csrc/wfs_devbuf.h) on the host alone: tests/host/devbuf_main.cpp is compiled against the
header with the host compiler and run; a counting malloc / free pair plays hipMalloc / hipFree, and a set of the live blocks
turns a double free into a failed case instead of a crash.

The program prints one line per case; every case also checks that the header's counters of live buffers agree with the
allocator's.  The same program is built a second time with the address and undefined-behaviour sanitizers: a double free or a
use after a move that the bookkeeping missed ends that run with a report."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['ensure_grows', 'scope_end_frees', 'capacity_rule', 'grow_frees_old_once', 'failed_alloc_leaves_empty', 'move',
         'move_scope_end', 'reset_twice', 'vector', 'vector_scope_end', 'struct', 'struct_scope_end']


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
