"""The wait loop of a step boundary (wfsim_amd/csrc/wfs_boundary.h) on the host alone: tests/host/boundary_wait_main.cpp is
compiled against the header with the host compiler and run; a std::thread plays the device, a counter plays hipStreamQuery.

* arrives: the word comes after the query has said not-ready twice -> ok, and the block stored before the word is visible
* never:   the query says finished and the word never changes -> "fall back", at the first query (one poll interval, 50 us)
* error:   the query returns an error -> the error is reported

The bounded time of `never` and `error` is asserted from the program's own clock: a few poll intervals of 50 us are far below the
1000 ms allowed; the process limit only ends a loop that hangs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('boundary') / 'boundary_wait_main')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-pthread', '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'),
                           '-o', exe, os.path.join(ROOT, 'tests', 'host', 'boundary_wait_main.cpp')])
    return exe


def _run(program, case):
    p = subprocess.run([program, case], capture_output=True, text=True, timeout=20)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    name, result, queries, ms = p.stdout.split()
    assert name == case
    return result, int(queries.split('=')[1]), float(ms.split('=')[1])


def test_word_arrives_while_not_ready(program):
    result, queries, ms = _run(program, 'arrives')
    assert result == 'ok' and queries >= 2 and ms < 1000.0


def test_stream_done_word_never_changes_falls_back(program):
    result, queries, ms = _run(program, 'never')
    assert result == 'fallback' and queries == 1 and ms < 1000.0


def test_query_error_is_reported(program):
    result, queries, ms = _run(program, 'error')
    assert result == 'error' and queries == 3 and ms < 1000.0
