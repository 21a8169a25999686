"""include/wfsim_amd.h, parsed once: the struct layouts, the export list and the signature of every entry point of the ctypes
binding come from the header and are stated nowhere else in Python.  ``bind(lib)`` sets restype and argtypes on a loaded
library; the argtypes check and convert every argument before the library is entered, for ``Engine`` and for raw ``lib.wfs_x(...)``
calls alike.  Not checked: the LENGTH of any buffer, and what a ``void *`` / ``char *`` points to."""
import collections
import ctypes as C
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'wfsim_amd.h')


class WfsError(RuntimeError):
    pass


SCALARS = {'int': C.c_int, 'int8_t': C.c_int8, 'int16_t': C.c_int16, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint8_t': C.c_uint8,
           'uint16_t': C.c_uint16, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64, 'float': C.c_float, 'double': C.c_double}
OPAQUE = ('void', 'char')           # pointed to only; their contents are the caller's business
# one parameter, struct field or return type: `const base *...* name[array]`
Decl = collections.namedtuple('Decl', 'name base depth const array')
Func = collections.namedtuple('Func', 'name ret params')
Header = collections.namedtuple('Header', 'handles structs functions')        # opaque struct names, {name: [Decl]}, {name: Func}
_DECL = re.compile(r'(const\s+)?(\w+)\s*(\**)\s*(\w*)\s*(?:\[(\d+)\])?$')


def _decl(text, known, where):
    m = _DECL.match(text.strip())
    if not m or m.group(2) not in known or (m.group(2) not in SCALARS and not m.group(3)):          # only numbers go by value
        raise WfsError(f'{HEADER}: cannot parse "{text.strip()}" in {where} (types known here: {", ".join(sorted(known))})')
    return Decl(m.group(4), m.group(2), len(m.group(3)), bool(m.group(1)), int(m.group(5)) if m.group(5) else None)


def parse(text):
    """Header(handles, structs, functions) of a header text.  Raises WfsError on any declaration it cannot parse or type it does not know:
    nothing is skipped."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^\s*#\s*ifdef\s+__cplusplus\b.*?^\s*#\s*endif\b', ' ', text, flags=re.S | re.M)          # extern "C" { and its }
    for line in re.findall(r'^\s*#.*$', text, flags=re.M):
        if not re.match(r'\s*#\s*(ifndef|define|include|endif)\b', line):
            raise WfsError(f'{HEADER}: preprocessor line not understood: {line.strip()}')
    text = re.sub(r'^\s*#.*$', ' ', text, flags=re.M)
    hdr = Header([], {}, {})
    known = set(SCALARS) | set(OPAQUE)
    top, pos = re.compile(r'\s*((?:[^;{}]|\{[^{}]*\})+);'), 0          # a top-level declaration ends at a ';' outside braces
    while text[pos:].strip():
        m = top.match(text, pos)
        if not m:
            raise WfsError(f'{HEADER}: declaration not understood: "{" ".join(text[pos:].split())[:120]}"')
        pos, d = m.end(), ' '.join(m.group(1).split())
        s = re.match(r'typedef struct (\w+) (?:\{(.*)\} )?(\w+)$', d)
        f = re.match(r'(.*?)\b(\w+) ?\((.*)\)$', d)
        if s and s.group(1) == s.group(3):
            if s.group(2) is None:
                hdr.handles.append(s.group(1))
            else:           # `type a, b` declares both with the type of the first
                fields = [_decl(q if k == 0 else decl.split()[0] + ' ' + q, set(SCALARS), 'struct ' + s.group(1))
                          for decl in s.group(2).split(';') if decl.strip() for k, q in enumerate(decl.split(','))]
                if not all(q.name and not q.depth and not q.const for q in fields):
                    raise WfsError(f'{HEADER}: struct {s.group(1)} may hold plain numbers only')
                hdr.structs[s.group(1)] = fields
            known.add(s.group(1))
        elif f and f.group(2).startswith('wfs_') and f.group(2) not in hdr.functions:
            ret = _decl(f.group(1), known, f.group(2))
            params = [_decl(q, known, f.group(2)) for q in f.group(3).split(',')]
            if ret.name or ret.array or not all(q.name for q in params):
                raise WfsError(f'{HEADER}: cannot parse the prototype of {f.group(2)}')
            hdr.functions[f.group(2)] = Func(f.group(2), ret, params)
        else:
            raise WfsError(f'{HEADER}: declaration not understood: "{d[:120]}"')
    return hdr


def _struct(name, fields):
    return type(name, (C.Structure,), dict(_fields_=[(f.name, SCALARS[f.base] * f.array if f.array else SCALARS[f.base]) for f in fields]))


# ---- argument rules (the table of DESIGN 8f) --------------------------------------------------------------------------------------
_CDATA = (C._SimpleCData, C.Array, C._Pointer)
_BYREF = type(C.byref(C.c_int()))


class Arg:
    """argtypes entry of one parameter: ctypes calls ``from_param`` and keeps what it returns alive until the C call has returned"""

    def __init__(self, func, decl):
        self.func, self.decl = func, decl
        self.ctype = SCALARS.get(decl.base)
        self.dtype = np.dtype(self.ctype) if self.ctype else None
        self.pointer = bool(decl.depth or decl.array)
        self.output = self.pointer and not decl.const
        self.size = C.sizeof(STRUCTS[decl.base]) if decl.base in STRUCTS else self.dtype.itemsize if self.dtype else 1

    def error(self, x, expected):
        what = f'{x.dtype} ndarray (flags {"C" if x.flags.c_contiguous else "-"}{"A" if x.flags.aligned else "-"}{"W" if x.flags.writeable else "-"})' \
            if isinstance(x, np.ndarray) else type(x).__name__
        return TypeError(f'{self.func}: parameter {self.decl.name} expects {expected}, got {what}')

    def from_param(self, x):
        d = self.decl
        if not self.pointer:
            if isinstance(x, C._SimpleCData):
                x = x.value
            if not isinstance(x, (int, float, np.number, np.bool_)):
                raise self.error(x, 'a number')
            return self.ctype(float(x) if self.dtype.kind == 'f' else int(x))
        if x is None or isinstance(x, C.c_void_p):          # NULL; c_void_p: the caller has dropped to raw addresses, unchecked
            return x
        if d.base in HANDLES or d.base in STRUCTS:          # wfs_handle *: the c_void_p above; wfs_handle **, struct *: byref of the object
            if isinstance(x, _BYREF) and (d.depth == 2 if d.base in HANDLES else C.sizeof(x._obj) == self.size):
                return x
            raise self.error(x, 'a c_void_p' if d.base in HANDLES and d.depth == 1 else f'byref of a {d.base}{" *" * (d.depth - 1)} or a c_void_p')
        if isinstance(x, _BYREF) or isinstance(x, _CDATA):           # scalar outs (byref(c_int32())), ctypes arrays and pointers
            if not isinstance(x, C._Pointer) and C.sizeof(x._obj if isinstance(x, _BYREF) else x) < self.size:
                raise self.error(x, f'at least one {d.base}')
            return x if isinstance(x, (_BYREF, C._Pointer)) else C.byref(x)
        if self.dtype is None:              # void *, char *: an address, whatever is behind it
            if isinstance(x, (int, np.integer)):
                return C.c_void_p(int(x))
            if not (isinstance(x, np.ndarray) and x.flags.c_contiguous and (d.const or x.flags.writeable)):
                raise self.error(x, f'a C-contiguous{"" if d.const else " writeable"} ndarray, an int address, a ctypes buffer or a c_void_p')
        elif self.output:                   # written by the library: never converted, never copied
            if not (isinstance(x, np.ndarray) and x.dtype == self.dtype and x.flags.c_contiguous and x.flags.aligned and x.flags.writeable):
                raise self.error(x, f'a C-contiguous, aligned, writeable ndarray of dtype {self.dtype} (or a ctypes object, or a c_void_p)')
        else:                               # read by the library: converted like any array-like
            x = np.asarray(x, dtype=self.dtype, order='C')
            if x.ndim == 0:
                raise self.error(x, f'an array of {self.dtype}, not one number')
        p = C.c_void_p(x.ctypes.data)
        p.array = x                         # the array (a converted temporary, perhaps) lives as long as the pointer does
        return p


def read_header(path=HEADER):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise WfsError(f'{path} not found: the ctypes binding takes every signature from it ({e})')


HANDLES, _structs, FUNCTIONS = parse(read_header())
STRUCTS = {name: _struct(name, fields) for name, fields in _structs.items()}
WfsConfig, WfsCounts = STRUCTS['wfs_config'], STRUCTS['wfs_counts']
EXPORTS = list(FUNCTIONS)


def restype(ret):
    if ret.depth:
        return C.c_char_p if ret.base == 'char' else C.c_void_p
    return SCALARS[ret.base]


def argtypes(name):
    """the Arg of every parameter of an entry point (what ``bind`` installs; usable without a library)"""
    return [Arg(name, d) for d in FUNCTIONS[name].params]


def bind(lib):
    """restype and argtypes of every declared entry point on a loaded library; AttributeError if the library lacks one"""
    class Entry(lib._FuncPtr):
        _flags_, _restype_ = lib._FuncPtr._flags_, lib._FuncPtr._restype_

        def __call__(self, *args):          # ctypes wraps what from_param raises in ctypes.ArgumentError: hand the TypeError on
            try:
                return super().__call__(*args)
            except C.ArgumentError as e:
                raise TypeError(str(e)) from None

    for name, f in FUNCTIONS.items():
        fn = Entry((name, lib))
        fn.restype, fn.argtypes = restype(f.ret), argtypes(name)
        setattr(lib, name, fn)
    return lib
