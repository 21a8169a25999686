"""The C-ABI library loads on a CPU-only machine and exports every symbol include/wfsim_amd.h declares; compute entry
points are not called here (no GPU).  Also: the product refuses to run without a GPU instead of falling back."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    txt = open(os.path.join(ROOT, 'include', 'wfsim_amd.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(wfs_[a-z_0-9]+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    from wfsim_amd import engine
    lib = engine.load_library()
    names = _declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/wfsim_amd.h but not exported by libwfsim_amd.so'
    assert set(engine.EXPORTS) == set(names)


def test_struct_layouts_match_header():
    from wfsim_amd.engine import WfsConfig, WfsCounts
    txt = open(os.path.join(ROOT, 'include', 'wfsim_amd.h')).read()
    body = re.search(r'typedef struct wfs_config \{(.*?)\} wfs_config;', txt, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(',')]
    assert [f[0] for f in fields] == [f[0] for f in WfsConfig._fields_]
    ctype = {'int32_t': ctypes.c_int32, 'double': ctypes.c_double, 'uint64_t': ctypes.c_uint64}
    assert [ctype[f[1]] for f in fields] == [f[1] for f in WfsConfig._fields_]
    assert ctypes.sizeof(WfsCounts) == 11 * 8


def test_parser_misses_nothing():
    from wfsim_amd import abi, engine
    names = _declared_functions()
    assert sorted(abi.FUNCTIONS) == names and sorted(engine.EXPORTS) == names
    assert len(engine.EXPORTS) == len(set(engine.EXPORTS))
    assert engine.WfsConfig is abi.WfsConfig and engine.WfsCounts is abi.WfsCounts


def _spell(d):
    return ('const ' if d.const else '') + d.base + (' ' + '*' * d.depth if d.depth else '') + (f'[{d.array}]' if d.array else '')


# written out by hand from the header: return type, then (parameter, type) in order
H, I32, I64, F64P, CF64P, I64P = ('h', 'wfs_handle *'), 'int32_t', 'int64_t', 'double *', 'const double *', 'int64_t *'
SPOT = {
    'wfs_create': ('int', [('cfg', 'const wfs_config *'), ('device', 'int'), ('out', 'wfs_handle **')]),
    'wfs_last_error': ('const char *', [('h', 'const wfs_handle *')]),
    'wfs_records_dev_ptr': ('const void *', [H]),
    'wfs_set_tables': ('int', [H, ('templates', CF64P), ('spe', CF64P), ('n_spe', I32), ('gains', CF64P), ('thr_truth', CF64P),
                               ('thr_zle', 'const int64_t *'), ('lum_x', CF64P), ('lum_t', CF64P), ('n_lum', I32),
                               ('noise', 'const int16_t *'), ('noise_len', I32), ('noise_channels', I32)]),
    'wfs_load_instructions': ('int', [H, ('n', I64), ('type', 'const int8_t *'), ('time', 'const int64_t *'), ('amp', 'const int32_t *'),
                                      ('gid', 'const uint32_t *'), ('cluster', 'const int32_t *'), ('tmin', 'const int64_t *'),
                                      ('p_hit', CF64P), ('drift_mean', CF64P), ('drift_spread', CF64P), ('sc_gain', CF64P),
                                      ('cdf_row', 'const int32_t *'), ('cdf_table', CF64P), ('n_cdf', I32),
                                      ('run_set', 'const int32_t *'), ('n_run_sets', I64), ('em_base', 'const uint32_t *')]),
    'wfs_copy_photons': ('int', [H, ('set_off', I64P), ('t', I64P), ('ch', 'int16_t *'), ('gain', F64P), ('dpe', 'uint8_t *'), ('capacity', I64)]),
    'wfs_copy_dark_counts': ('int', [H, ('channel', I32), ('thr', 'uint32_t[4]')]),
    'wfs_kernel_times': ('int', [H, ('names', 'char *'), ('names_cap', I64), ('ms', 'float *'), ('n_launches', 'int32_t *'), ('n_kernels', 'int32_t *')]),
    'wfs_host_register': ('int', [('ptr', 'void *'), ('bytes', I64)]),
}
NP = {'int8_t': 'int8', 'int16_t': 'int16', 'int32_t': 'int32', 'int64_t': 'int64', 'uint8_t': 'uint8', 'uint32_t': 'uint32',
      'int': 'intc', 'float': 'float32', 'double': 'float64'}


@pytest.mark.parametrize('name', sorted(SPOT))
def test_spot_signatures(name):
    """the parsed prototype, and the restype / argument kinds bound from it, against the hand-written expectation"""
    import numpy as np
    from wfsim_amd import abi, engine
    ret, params = SPOT[name]
    f = abi.FUNCTIONS[name]
    assert _spell(f.ret) == ret and [(d.name, _spell(d)) for d in f.params] == params
    fn = getattr(engine.load_library(), name)
    assert fn.restype is {'int': ctypes.c_int, 'const char *': ctypes.c_char_p, 'const void *': ctypes.c_void_p}[ret]
    assert len(fn.argtypes) == len(params)
    for arg, (pname, spelling) in zip(fn.argtypes, params):
        base = spelling.replace('const ', '').split(' ')[0].split('[')[0]
        pointer = '*' in spelling or '[' in spelling
        assert (arg.func, arg.decl.name, arg.pointer, arg.output) == (name, pname, pointer, pointer and 'const' not in spelling)
        assert arg.dtype == (np.dtype(NP[base]) if base in NP else None)


def test_struct_sizes():
    from wfsim_amd.engine import WfsConfig, WfsCounts
    assert ctypes.sizeof(WfsConfig) == 24 * 4 + 16 * 8 + 8
    assert ctypes.sizeof(WfsCounts) == 11 * 8
    assert all(t is ctypes.c_int64 for _, t in WfsCounts._fields_)


@pytest.mark.parametrize('text', ['int wfs_x(wfs_handle *h, size_t n);',                     # a type the binding does not know
                                  'int wfs_x(wfs_handle *h, int32_t);',                      # malformed: a parameter without a name
                                  'int wfs_x(wfs_handle *h, int32_t n;',
                                  'int wfs_x(wfs_handle h);',                                # an opaque struct by value
                                  'typedef struct wfs_s { int32_t a; long b; } wfs_s;',
                                  '#if 1\nint wfs_x(wfs_handle *h);\n#endif',
                                  'int wfs_x(wfs_handle *h) { return 0; }'])
def test_parser_fails_loudly(text):
    from wfsim_amd import abi
    head = '#include <stdint.h>\ntypedef struct wfs_handle wfs_handle; /* c */\n'
    assert list(abi.parse(head + 'int wfs_x(wfs_handle *h, const int32_t *a);').functions) == ['wfs_x']
    with pytest.raises(abi.WfsError):
        abi.parse(head + text)


def test_missing_header_names_the_path(tmp_path):
    from wfsim_amd import abi
    with pytest.raises(abi.WfsError, match='no_such_header.h'):
        abi.read_header(str(tmp_path / 'no_such_header.h'))


def test_argument_rules():
    """the rules of DESIGN 8f on the argtypes objects themselves: no library call"""
    import gc
    import weakref
    import numpy as np
    from wfsim_amd import abi
    h, left, right, first, ix = abi.argtypes('wfs_copy_groups')
    good = np.zeros(8, dtype=np.int64)
    assert left.from_param(good).value == good.ctypes.data
    with pytest.raises(TypeError, match=r'wfs_copy_groups: parameter left expects .*int64'):
        left.from_param(np.zeros(8, dtype=np.int32))
    with pytest.raises(TypeError, match='wfs_copy_groups: parameter right'):
        right.from_param(np.zeros(16, dtype=np.int64)[::2])             # not contiguous
    ro = np.zeros(8, dtype=np.int64)
    ro.flags.writeable = False
    with pytest.raises(TypeError, match='wfs_copy_groups: parameter first_record'):
        first.from_param(ro)
    for bad in ([0] * 8, 5, np.zeros(8, dtype=np.int64).view(np.float64), np.zeros(17, dtype=np.int8)[1:].view(np.int64)):
        with pytest.raises(TypeError, match='wfs_copy_groups: parameter ix_rand'):
            ix.from_param(bad)                                          # a list, a number, float64, unaligned: never converted
    thr = abi.argtypes('wfs_copy_dark_counts')[2]                       # uint32_t thr[4]: an output like any T *
    with pytest.raises(TypeError, match='wfs_copy_dark_counts: parameter thr'):
        thr.from_param(np.zeros(4, dtype=np.int32))
    assert thr.from_param(np.zeros(4, dtype=np.uint32)).value

    # inputs: converted, and the temporary lives exactly as long as what from_param returned
    gid = abi.argtypes('wfs_load_instructions')[5]                      # const uint32_t *
    src = np.arange(16, dtype=np.int64)[::2]
    p = gid.from_param(src)
    assert p.value != src.ctypes.data and p.array.dtype == np.uint32 and p.array.flags.c_contiguous
    assert np.array_equal(p.array, src) and (ctypes.c_uint32 * 8).from_address(p.value)[:] == list(src)
    alive = weakref.ref(p.array)
    gc.collect()
    assert alive() is not None
    del p
    gc.collect()
    assert alive() is None
    same = np.arange(8, dtype=np.uint32)
    assert gid.from_param(same).value == same.ctypes.data               # the right dtype and layout: no copy
    assert gid.from_param([1, 2, 3]).array.dtype == np.uint32
    with pytest.raises(TypeError, match='wfs_load_instructions: parameter gid'):
        gid.from_param(7)

    # NULL and the raw-address escape hatch
    for arg in (left, gid, thr, h, abi.argtypes('wfs_host_register')[0], abi.argtypes('wfs_get_counts')[1]):
        assert arg.from_param(None) is None
        raw = ctypes.c_void_p(good.ctypes.data)
        assert arg.from_param(raw) is raw
    # scalar outs and ctypes buffers
    n_cells = abi.argtypes('wfs_copy_noise_model')[5]                   # int32_t *n_cells
    ref = ctypes.byref(ctypes.c_int32())
    assert n_cells.from_param(ref) is ref
    assert abi.argtypes('wfs_kernel_times')[3].from_param((ctypes.c_float * 64)()) is not None
    with pytest.raises(TypeError, match='wfs_dark_count_photons: parameter count'):
        abi.argtypes('wfs_dark_count_photons')[7].from_param(ctypes.byref(ctypes.c_int32()))        # int64_t *count
    # void * / char *
    ptr = abi.argtypes('wfs_host_register')[0]
    assert ptr.from_param(good.ctypes.data).value == good.ctypes.data and ptr.from_param(good).value == good.ctypes.data
    assert abi.argtypes('wfs_kernel_times')[1].from_param(ctypes.create_string_buffer(16)) is not None
    for bad in (ro, np.zeros(16, dtype=np.int64)[::2], 'text'):
        with pytest.raises(TypeError, match='wfs_host_register: parameter ptr'):
            ptr.from_param(bad)
    # handles and structs
    with pytest.raises(TypeError, match='wfs_copy_groups: parameter h'):
        h.from_param(good)
    cfg, counts = abi.argtypes('wfs_create')[0], abi.argtypes('wfs_get_counts')[1]
    assert cfg.from_param(ctypes.byref(abi.WfsConfig())) is not None and counts.from_param(ctypes.byref(abi.WfsCounts())) is not None
    with pytest.raises(TypeError, match='wfs_get_counts: parameter out'):
        counts.from_param(ctypes.byref(abi.WfsConfig()))
    assert abi.argtypes('wfs_create')[2].from_param(ctypes.byref(ctypes.c_void_p())) is not None

    # scalars: Python and numpy numbers, bools, ctypes instances
    n, amp_bin = abi.argtypes('wfs_load_instructions')[1], abi.argtypes('wfs_set_ap_element')[7]
    for v in (2 ** 40, np.int64(2 ** 40), np.uint64(2 ** 40), ctypes.c_int64(2 ** 40)):
        r = n.from_param(v)
        assert type(r) is ctypes.c_int64 and r.value == 2 ** 40
    assert n.from_param(True).value == 1 and n.from_param(np.bool_(True)).value == 1 and n.from_param(np.int8(-3)).value == -3
    for v in (0.25, np.float32(0.25), 1, np.int32(1), ctypes.c_double(0.25)):
        r = amp_bin.from_param(v)
        assert type(r) is ctypes.c_double and r.value == float(getattr(v, 'value', v))
    for bad in ('3', None, np.zeros(1), [1]):
        with pytest.raises(TypeError, match='wfs_load_instructions: parameter n '):
            n.from_param(bad)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    import wfsim_amd
    from wfsim_amd.engine import WfsError
    with pytest.raises(WfsError):
        wfsim_amd.RawData(wfsim_amd.xenonnt_test_config())


def test_product_does_not_import_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'wfsim_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.h')):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle', src, flags=re.M), f
                assert 'liboracle' not in src and 'wfsim_oracle' not in src.replace('oracle/wfsim_oracle.c', ''), f
