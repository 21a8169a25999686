"""The LDS layouts and the window rules (wfsim_amd/csrc/wfs_layout.h) on the host alone: tests/host/layout_main.cpp is compiled against
the header with the host compiler and run.

Every kernel with dynamic LDS has a struct of byte offsets plus `total` there; the kernel takes its pointers from it and its launch
passes `total`.  The program checks every layout at the parameters its dispatch can produce (regions ascending, disjoint, aligned,
inside the total), holds the byte counts the launch sites reserved before the layouts existed as literals, and checks the largest total
of each kernel against the cap wfs_create grants.  Three totals were never rounded to 16 bytes by their launches -- k_photon_count
(multiple of 4), k_map_rows and k_photon_fill (multiples of 8) -- and stay as they were, to the byte; every other total is a multiple
of 16.  tile_window, row_slot and row_span are checked on values worked out by hand from pulse.py:118-127 and rawdata.py:242-259."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'wfsim_amd', 'csrc')
CASES = ['regions', 'totals_as_before', 'generic_totals_as_before', 'caps', 'bright_grant', 'tile_window', 'row_slot', 'row_span']


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('layout') / 'layout_main')
    subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror', '-O2', '-I', CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'host', 'layout_main.cpp')])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    return {ln[0]: ln[1:] for ln in lines}


@pytest.mark.parametrize('case', CASES)
def test_case(results, case):
    assert results[case] == ['ok'], results[case]


def _code(name):
    return re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, name)).read())


def test_layouts_and_windows_are_written_once():
    """no launch site keeps a byte formula of its own, the record size has one name, and the window of a tile is computed in one place"""
    eng = _code('wfs_engine.hip')
    assert 'TAP_LDS_BYTES' not in eng and 'ROW_LDS_FIXED' not in eng and 'GEN_COUNT_LDS' not in eng
    assert '* 244' not in eng
    sources = [n for n in os.listdir(CSRC) if n.endswith(('.h', '.hip'))]
    assert 'wfs_layout.h' in sources
    for name in sources:
        src = _code(name)
        assert 'tile_bounds' not in src, name
        assert ('store_before - d.samples_before' in src) == (name == 'wfs_layout.h'), name
    # every kernel with dynamic LDS reads a layout, and every launch with a byte count names one
    for name in ('wfs_kernels.h', 'wfs_tilegen.h'):
        src = _code(name)
        kernels = re.split(r'__global__', src)[1:]
        carving = [k for k in kernels if 'extern __shared__' in k.split('\n}\n')[0]]
        assert carving
        for k in carving:
            body = k.split('\n}\n')[0]
            assert re.search(r'\b(pulse_lds|sparse_lds|generic_lds|tile_lds|tile_gen_lds|bright_lds_layout|row_pulse_lds|order_lds|count_lds|map_rows_lds|gen_fill_lds)\(', body), body[:120]
    assert not re.search(r'k_pulse_sparse<256|K_PULSE_SPARSE_256', eng)
