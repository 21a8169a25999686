"""The noise-model state of a handle (wfsim_amd/csrc/wfs_noise.h) on the host alone: tests/host/noise_state_main.cpp is compiled
against the header with the host compiler and run.

The header holds what the three noise setters describe, nested by lifetime (the model, inside it the colour, inside that the slow
levels), the transitions between its states, one layout description for each of the two device buffers, and the setters' checks as
pure functions.  The program prints one line per case.  Its lists of the structs' members are structured bindings, so a member added
to the header and not to the lists fails the build, and a listed member that a reset leaves behind fails its case."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['fresh', 'fill_sets_every_member', 'model_set', 'model_cleared', 'model_set_drops_colour_and_levels', 'colour_set_drops_levels',
         'colour_cleared_drops_levels', 'slow_set_and_cleared', 'layout_colour_with_groups', 'layout_slow_on_colour',
         'layout_colour_without_groups', 'layout_levels_without_colour', 'packers_fill_the_layouts', 'model_refusals', 'colour_refusals',
         'slow_refusals', 'colour_bound_at_its_edge', 'slow_bound_at_its_edge']
TRANSITIONS = ['model_set', 'model_cleared', 'colour_set', 'colour_cleared', 'slow_set', 'slow_cleared']


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('noise_state') / 'noise_state_main')
    subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror', '-O2', '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'),
                           '-o', exe, os.path.join(ROOT, 'tests', 'host', 'noise_state_main.cpp')])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    return {ln[0]: ln[1:] for ln in lines}


@pytest.mark.parametrize('case', CASES)
def test_case(results, case):
    assert results[case] == ['ok'], results[case]


def test_the_engine_has_no_other_writer():
    """nothing in wfs_engine.hip writes a member of the noise state: it moves through the transitions of the header, one call of each,
    and the buffers they name are dropped with it"""
    src = open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_engine.hip')).read()
    src = re.sub(r'//[^\n]*', '', src)
    # the handle's member is reached as h->noise; any other name for it is a reference to const
    writes = r'\s*(=[^=]|\+=|-=|\+\+|--|\.(swap|clear|assign|resize|push_back|insert|erase)\b)'
    assert not re.search(r'\bnoise\.[\w.]+' + writes, src)
    for ref in re.findall(r'[^\n]*\bNoise(?:Model|Colour|Slow)State\s*&[^\n]*', src):
        assert re.search(r'\bconst\s+Noise(Model|Colour|Slow)State\s*&', ref), ref
    assert 'const_cast' not in src
    assert src.count('NoiseTransitions{') == 1          # wfs_handle::noise_state
    for name in TRANSITIONS:
        assert src.count(f'h->noise_moves(h->noise_state().{name}(') == 1 and src.count(f'.{name}(') == 1, name
    # the members the state replaced are gone
    assert not re.search(r'\b(nm_channels|nm_k|nm_values|h_nm_cells|nc_n_taps\s*=\s*0|h_nc_tapsum|clear_noise_colour)\b', src.replace('d.nc_n_taps', ''))


def test_layouts_are_written_once():
    """the offsets of the two buffers stand in the layout structs: neither the engine nor the packers repeat them"""
    eng = re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_engine.hip')).read())
    assert 'NC_TAP_STRIDE' not in eng and 'NC_TAP_PAD' not in eng and 'NS_MAX_LEVELS' not in eng
    hdr = re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_noise.h')).read())
    body = hdr[hdr.index('inline bool noise_colour_pack'):hdr.index('struct NoiseTransitions')]
    assert 'NC_TAP_STRIDE' not in body and 'NC_TAP_PAD' not in body
    assert len(re.findall(r'1\s*<<\s*29', hdr)) == 1 and not re.search(r'1\s*<<\s*29', eng)
