"""The bookkeeping of deferred packers (wfsim_amd/csrc/wfs_pack_fence.h) on the host alone: tests/host/pack_fence_main.cpp is compiled
against the header with the host compiler and run.  A counting engine plays the pack stream: a pack runs from the moment it is deferred
until a stream or the host waits for its arena's event, and a write, a free or a read of what it uses in between counts as a hazard.

The transitions: pending -> fenced once per run (however many places of the run ask) -> waited by a reader; a reader on a stream of
its own leaves the fence to the next run; a grow of a buffer the packers use waits on the host before the old block goes; a change of
mode waits and the serial run that follows defers nothing.  The program is built a second time with the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['idle', 'pending_fenced_read', 'stream_reader_keeps_fence', 'grow_while_pending', 'mode_change']


def _compiler():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    return cxx


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / 'pack_fence_main')
    subprocess.check_call([_compiler(), '-std=c++17', '-Wall', '-Werror', *extra, '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'),
                           '-o', exe, os.path.join(ROOT, 'tests', 'host', 'pack_fence_main.cpp')])
    return exe


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    return {ln[0]: ln[1:] for ln in lines}


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    return _run(_build(tmp_path_factory, 'pack_fence', ['-O2']))


@pytest.mark.parametrize('case', CASES)
def test_case(results, case):
    assert results[case][0] == 'ok', results[case]
    assert dict(f.split('=') for f in results[case][1:])['hazards'] == '0'


def test_under_sanitizers(tmp_path_factory):
    # the runtimes linked into the program: it then runs whatever else the environment loads into a process first
    static = ['-static-libsan'] if 'clang' in os.path.basename(_compiler()) else ['-static-libasan', '-static-libubsan']
    r = _run(_build(tmp_path_factory, 'pack_fence_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static]))
    assert all(v[0] == 'ok' for v in r.values()), r
