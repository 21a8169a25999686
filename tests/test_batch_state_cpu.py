"""The batch and run state of a handle (wfsim_amd/csrc/wfs_batch.h) on the host alone: tests/host/batch_state_main.cpp is compiled
against the header with the host compiler and run.

The header holds what a wfs_load_* call describes (BatchState), what wfs_run found (RunResult) and the transitions between their
states; the engine calls nothing else to change a batch's kind or a run's stage.  The program prints one line per case.  Its list of
the structs' members is a structured binding, so a member added to the header and not to the list fails the build, and a listed
member that a reset leaves behind fails its case."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['fresh', 'fill_sets_every_member', 'begin_commit_each_kind', 'begin_without_commit_leaves_none', 'new_load_clears_previous_batch',
         'ap_sets_false_after_photon_load', 'option_changed_after_generation', 'run_begins_resets_results',
         'view_changed_falls_back_from_complete']


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('batch_state') / 'batch_state_main')
    subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror', '-O2', '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'),
                           '-o', exe, os.path.join(ROOT, 'tests', 'host', 'batch_state_main.cpp')])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    return {ln[0]: ln[1:] for ln in lines}


@pytest.mark.parametrize('case', CASES)
def test_case(results, case):
    assert results[case] == ['ok'], results[case]


def test_the_engine_has_no_other_writer():
    """nothing in wfs_engine.hip assigns the batch's kind or the run's stage: both move through the transitions of the header"""
    import re
    src = open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_engine.hip')).read()
    assert not re.search(r'\b(batch|b)\.kind\s*=[^=]', src) and not re.search(r'\brun\.stage\s*=[^=]', src)
    for name in ('load_begins', 'load_commits'):
        assert src.count(f'state().{name}(') == 3, name          # one of each in each of the three loaders
