"""Kernel families (wfsim_amd/csrc/wfs_family.h) on the host alone: tests/host/family_main.cpp is compiled against the header with the host
compiler and run; plain function templates that return their own template arguments play the kernels.

The program prints one line per case.  The same program is built a second time with the address and undefined-behaviour sanitizers: a
read past a table that the bounds rule missed ends that run with a report.  The source checks below hold wfs_engine.hip to what the
families are for: one launch function, every family declared once, the LDS caps raised in one place."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['pick_6222', 'pick_222', 'pick_22', 'pick_2', 'pick_mapped', 'size_is_product', 'members_distinct', 'outside_is_null',
         'name_and_cap', 'capped_are_listed']


def _compiler():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    return cxx


def _build(tmp_path_factory, name, extra):
    cxx = _compiler()
    exe = str(tmp_path_factory.mktemp(name) / 'family_main')
    subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror', *extra, '-I', os.path.join(ROOT, 'wfsim_amd', 'csrc'),
                           '-o', exe, os.path.join(ROOT, 'tests', 'host', 'family_main.cpp')])
    return exe


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    return {ln[0]: ln[1:] for ln in lines}


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    return _run(_build(tmp_path_factory, 'family', ['-O2']))


@pytest.mark.parametrize('case', CASES)
def test_case(results, case):
    assert results[case][0] == 'ok', results[case]


def test_under_sanitizers(tmp_path_factory):
    # the runtimes linked into the program: it then runs whatever else the environment loads into a process first
    static = ['-static-libsan'] if 'clang' in os.path.basename(_compiler()) else ['-static-libasan', '-static-libubsan']
    r = _run(_build(tmp_path_factory, 'family_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static]))
    assert all(v[0] == 'ok' for v in r.values()), r


@pytest.fixture(scope='module')
def engine_src():
    """wfs_engine.hip without its comments"""
    return re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_engine.hip')).read())


def test_retired_spellings_are_gone(engine_src):
    """No K_*(F) macro, none of the launch and cap macros, no with_noise_kind / with_row_kind, no HIP_KERNEL_NAME."""
    for word in ('WFS_LAUNCH_F', 'WFS_BIG_LDS', 'with_noise_kind', 'with_row_kind', 'HIP_KERNEL_NAME'):
        assert word not in engine_src, word
    assert not re.findall(r'#\s*define\s+K_\w+', engine_src)


def test_one_launch_function(engine_src):
    """hipLaunchKernelGGL occurs once, inside the launch function; everything else goes through it."""
    assert engine_src.count('hipLaunchKernelGGL') == 1
    m = re.search(r'int launch_as\(wfs_handle \*h,[^\n]*\n\{\n(.*?)\n\}\n', engine_src, re.S)
    assert m and 'hipLaunchKernelGGL(k.fn,' in m.group(1), m
    assert '<<<' not in engine_src and 'hipModuleLaunchKernel' not in engine_src and 'hipLaunchKernel(' not in engine_src
    # a null member is refused in front of the launch, with the code of a state error
    body = m.group(1)
    assert body.index('if (!k.fn) return h->fail(WFS_E_STATE') < body.index('hipLaunchKernelGGL')
    assert len(re.findall(r'\blaunch(?:_untimed)?\(h, ', engine_src)) > 80        # (99 statements before the variants of one kernel became one)


def test_every_family_is_declared_once(engine_src):
    """One family per template kernel, each declared exactly once at namespace scope; no template kernel is named with explicit
    arguments anywhere else."""
    decl = re.findall(r'^const auto (K_\w+) = family<([\w, ]+)>\("(\w+)"', engine_src, re.M)
    names = [d[0] for d in decl]
    assert len(names) == len(set(names)) and len(engine_src.split('family<')) - 1 == len(decl)
    expected = {'K_S2_TILE': 'k_s2_tile', 'K_S2_TILE_GEN': 'k_s2_tile_gen', 'K_S2_BRIGHT': 'k_s2_bright', 'K_PHOTON_FILL': 'k_photon_fill',
                'K_PULSE': 'k_pulse_dense', 'K_PULSE_GENERIC': 'k_pulse_generic', 'K_PULSE_SPARSE': 'k_pulse_sparse',
                'K_PULSE_TINY': 'k_pulse_tiny', 'K_PULSE_WAVE': 'k_pulse_wave', 'K_ROW_PULSE': 'k_row_pulse', 'K_ROW_EMPTY': 'k_row_empty',
                'K_ZLE': 'k_zle', 'K_PACK': 'k_pack', 'K_AP_SEG': 'k_ap_seg', 'K_OPTICAL_BUCKET': 'k_optical_bucket',
                'K_NOISE_COLOUR_SAMPLES': 'k_noise_colour_samples', 'K_TILE_ORDER_BIG': 'k_tile_order_big'}
    assert {d[0]: d[2] for d in decl} == expected
    axes = {d[0]: d[1].replace(' ', '') for d in decl}
    assert axes['K_ROW_PULSE'] == 'NOISE_KINDS,2,2,2' and axes['K_PULSE'] == '2,2,2' and axes['K_S2_TILE'] == '2,2'
    # a kernel with explicit template arguments stands in a family's lambda and nowhere else
    inst = re.findall(r'^.*\bk_\w+<[^;\n]*>', engine_src, re.M)
    assert len(inst) == len(decl) - 1 and all('= family<' in ln or ln.lstrip().startswith('[](auto') for ln in inst), inst


def test_one_record_back_end_and_one_way_to_call_rocprim(engine_src):
    """Every rocPRIM operation is spelled once, inside a caller of two_step, which alone holds the sizing call, the scratch and the
    real call; the record order (k_invert_perm) and the packers of finished rows (k_pack_res) are launched in one place each, for the
    rows of a run and of a lone-hit pass alike; one scratch buffer."""
    for call in ('radix_sort_pairs(', 'radix_sort_keys(', 'segmented_radix_sort_pairs(', 'inclusive_scan('):
        assert len(re.findall(r'\b' + re.escape(call), engine_src)) == 1, call
    assert len(re.findall(r'\bk_invert_perm\b', engine_src)) == 1 and engine_src.count('PLAIN(k_invert_perm)') == 1
    assert len(re.findall(r'\bk_pack_res\b', engine_src)) == 1 and engine_src.count('PLAIN(k_pack_res)') == 1
    assert engine_src.count('DevBuf sort_tmp') == 1 and len(re.findall(r'\bDevBuf\b[^;()]*\bsort_tmp\b', engine_src)) == 1
    # the scratch is named in its declaration and in two_step, nowhere else; a null scratch is handed over in two_step alone
    m = re.search(r'int two_step\(wfs_handle \*h,[^\n]*\n\{\n(.*?)\n\}\n', engine_src, re.S)
    assert m and m.group(1).count('sort_tmp') == len(re.findall(r'\bsort_tmp\b', engine_src)) - 1 == 2
    assert m.group(1).count('call(nullptr, bytes)') == 1 and engine_src.count('(nullptr, bytes') == 1
    assert len(re.findall(r'\brocprim::', engine_src)) == 4 + 4            # the four operations; the four operators of the overlay's scans
    # the key bits in use come from wfs_rows.h: no loop over end_bit is left, and the record key shift is named
    assert 'end_bit++' not in engine_src and '<< 12' not in engine_src
    kernels = re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_kernels.h')).read())
    assert '<< REC_KEY_SHIFT) | (u64)(u32)q.channel' in kernels and 'key_base) << 12' not in kernels


def test_lds_caps_are_raised_in_one_place(engine_src):
    assert engine_src.count('hipFuncAttributeMaxDynamicSharedMemorySize') == 1
    assert engine_src.count('hipFuncSetAttribute') == 1 and engine_src.count('FamilyBase::each') == 1
