"""The packers on a stream of their own (wfs_engine.hip run_records, wfs_pack_fence.h): wfs_run returns once the counts are known,
k_pack_desc / k_pack_res / k_pack of batch k run under the front end of batch k + 1, which fences them in front of its first write to
what they read; every reader of the records waits for the arena's ready event.  None of it may change a byte.

The comparison, in every case: records (tobytes()), counts and truth() of the default engine == those of an engine created under
WFS_PACK_SYNC=1 (the packers on the main stream, in front of the last boundary) == those of a fresh engine per batch (created under
WFS_PACK_SYNC=1 as well: one run, nothing before or after it).  The batches are those of tests/test_gpu_step_boundaries.py, the
smallest that take the tile path (s2), the block generator with resident rows, k_pack_res and noise (mixed), and an optical load
(nveto); 's2_1' is one instruction with ids of its own, so that the tile buffers of the run before are larger than it needs.

No timing is asserted anywhere."""
import contextlib
import ctypes as C
import functools
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_step_boundaries import MIXED, _assert_same, _result
from wfsim_amd import workloads as W
from wfsim_amd.engine import Engine, device_allocations
from wfsim_amd.ministrax import raw_record_dtype
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ['default', 'sync']


@contextlib.contextmanager
def _pack_sync(mode):
    """WFS_PACK_SYNC as wfs_create reads it: '1' for 'sync', unset for 'default'"""
    old = os.environ.pop('WFS_PACK_SYNC', None)
    if mode == 'sync':
        os.environ['WFS_PACK_SYNC'] = '1'
    try:
        yield
    finally:
        os.environ.pop('WFS_PACK_SYNC', None)
        if old is not None:
            os.environ['WFS_PACK_SYNC'] = old


def _config(case):
    if case.startswith('s2'):
        return W.bench_config(seed=3)
    if case == 'nveto':
        return W.nveto_config(seed=31)
    return W.mixed_config(seed=3)


def _engine(case, mode, sort=False):
    cfg = _config(case)
    with _pack_sync(mode):
        eng = Engine(cfg, Resource(cfg))
    if sort:
        eng.set_record_order(True)
    return eng


def _load_and_run(eng, case):
    """loads the batch and runs it; the counts, and nothing read"""
    cfg = _config(case)
    if case == 'nveto':
        ins, channels, timings = W.optical_instructions(200, 1000.0, 3)
        order, key, cluster = schedule(ins, cfg)
        eng.load_optical(ins[order], order.astype(np.uint32), cluster, key, channels, timings, int(1e6))
        return eng.run()
    if case == 's2':
        ins, gid0 = W.s2_batch(3, electrons=2000), 0
    elif case == 's2_1':
        ins, gid0 = W.s2_batch(1, first_gid=100, electrons=2000), 100
    else:
        n = int(case[len('mixed'):])
        ins, gid0 = W.mixed_batch(n, MIXED[n]), MIXED[n]
    order, key, cluster = schedule(ins, cfg)
    s_ins = ins[order]
    ip = instruction_params(s_ins, cfg, Resource(cfg), device_maps=eng.device_maps)
    eng.load_instructions(s_ins, (gid0 + order).astype(np.uint32), cluster, key, ip)
    return eng.run()


@functools.lru_cache(maxsize=None)
def _fresh(case, sort=False):
    """one batch on a fresh engine with the serial order; computed once per batch and shared, never changed"""
    eng = _engine(case, 'sync', sort)
    r = _result(eng, _load_and_run(eng, case))
    eng.close()
    return r


def _sequence(mode, cases, read_each, sort=False):
    """the batches one after the other on one engine; results of every run (read_each) or of the last alone"""
    eng = _engine(cases[0], mode, sort)
    out = []
    for k, case in enumerate(cases):
        counts = _load_and_run(eng, case)
        if read_each or k == len(cases) - 1:
            out.append((case, _result(eng, counts)))
        else:
            assert counts == _fresh(case, sort)['counts']        # (the counts do not wait for the packers)
    eng.close()
    return out


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['s2', 'mixed20', 'nveto'])
def test_run_after_run_records_untouched(case, mode):
    """three runs, records() only after the last: the fence of run 2 and 3 is all that orders the packers of run 1 and 2"""
    eng = _engine(case, mode)
    _load_and_run(eng, case)
    for _ in range(2):
        counts = eng.run()
    _assert_same(_result(eng, counts), _fresh(case))
    eng.close()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('read_each', [True, False])
def test_fence_tile_path(mode, read_each):
    """s2 (3 instructions), at once one instruction, then 3 again: the tile buffers are reused, too large and again exactly filled
    under a pack that may be pending"""
    for case, got in _sequence(mode, ['s2', 's2_1', 's2'], read_each):
        _assert_same(got, _fresh(case))


@pytest.mark.parametrize('mode', MODES)
def test_grow_under_pending_pack(mode):
    """mixed 20 -> 3 -> 40 with nothing read in between: the buffers the packers of the 3 read grow for the 40"""
    (case, got), = _sequence(mode, ['mixed20', 'mixed3', 'mixed40'], False)
    _assert_same(got, _fresh('mixed40'))


def test_every_reader_same_bytes():
    """records(), records_into, records_into_async + wait_records after one run; then run -> async copy -> run -> async copy, each
    copy checked after its wait_records.  (copy_records_to_device into a torch tensor: test_torch_reader_and_lifetime_in_a_fresh_process)"""
    eng = _engine('s2', 'default')
    ref = {c: _fresh(c)['records'] for c in ('s2', 's2_1')}
    n = {c: _fresh(c)['counts']['n_records'] for c in ref}
    bufs = [np.zeros(max(n.values()) + 8, dtype=raw_record_dtype()) for _ in range(3)]
    assert all(eng.pin(b) for b in bufs)
    _load_and_run(eng, 's2')
    eng.run()                                                   # (a pack is pending behind the one being read)
    got_async = eng.records_into_async(bufs[0])
    eng.wait_records()
    assert got_async.tobytes() == ref['s2']
    assert eng.records_into(bufs[1]).tobytes() == ref['s2'] and eng.records().tobytes() == ref['s2']
    for b in bufs:
        b[:] = 0
    # the chain of a consumer that copies batch k out under batch k + 1
    _load_and_run(eng, 's2')
    a = eng.records_into_async(bufs[0])
    _load_and_run(eng, 's2_1')
    eng.wait_records()
    assert a.tobytes() == ref['s2']
    b = eng.records_into_async(bufs[1])
    _load_and_run(eng, 's2')
    eng.wait_records()
    assert b.tobytes() == ref['s2_1']
    c = eng.records_into_async(bufs[2])
    eng.wait_records()
    assert c.tobytes() == ref['s2'] and a.tobytes() == ref['s2'] and b.tobytes() == ref['s2_1']
    eng.close()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['s2', 'mixed20'])
def test_sorted_records(case, mode):
    """sort_records: the key, sort and permutation stage stays on the main stream, the packers read rec_dest from the pack stream"""
    ref = _fresh(case, sort=True)
    assert ref['records'] != _fresh(case)['records'] and len(ref['records']) == len(_fresh(case)['records'])
    eng = _engine(case, mode, sort=True)
    _load_and_run(eng, case)
    _assert_same(_result(eng, eng.run()), ref)
    eng.close()


@pytest.mark.parametrize('case', ['s2', 'mixed20'])
def test_profiled_step_is_serial(case):
    """set_profiling(True) behind a deferred pack: the profiled step lists the packers as before, with unchanged bytes; back to the
    default, the next run defers again"""
    eng = _engine(case, 'default')
    _load_and_run(eng, case)
    eng.set_profiling(True)
    got = _result(eng, eng.run())
    times = eng.kernel_times()
    assert 'k_pack' in times and 'k_pack_desc' in times, times
    if case == 'mixed20':
        assert 'k_pack_res' in times, times
    _assert_same(got, _fresh(case))
    eng.set_profiling(False)
    _assert_same(_result(eng, eng.run()), _fresh(case))
    eng.close()


def test_caller_stream_is_serial():
    """an engine given a stream (wfs_set_stream) after a deferred run: same bytes.  The stream comes from the HIP runtime the library
    itself is linked against."""
    hip = C.CDLL('libamdhip64.so.7')
    stream = C.c_void_p(0)
    eng = _engine('s2', 'default')
    _load_and_run(eng, 's2')
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    eng.set_stream(stream.value)
    for case in ('s2_1', 's2'):
        _assert_same(_result(eng, _load_and_run(eng, case)), _fresh(case))
    eng.close()
    assert hip.hipStreamDestroy(stream) == 0


def test_destroy_with_a_pack_pending_and_table_setter():
    """create, load, run, destroy without reading: every buffer goes back (compared with the figure at the start of the test, as
    tests/test_gpu_handle_lifetime.py does: the exact zero is asserted in a fresh process below).  Then a table setter right after a
    run, followed by another run: the bytes of a fresh engine with those tables."""
    gc.collect()
    baseline = device_allocations()
    eng = _engine('mixed20', 'default')
    _load_and_run(eng, 'mixed20')
    assert device_allocations()[0] > baseline[0]
    eng.close()
    assert device_allocations() == baseline

    def set_noise(e, noise):
        t = e.tables
        nl, nc = noise.shape
        e._check(e.lib.wfs_set_tables(e._h, *[C.c_void_p(t[k].ctypes.data) for k in ('templates', 'spe')], C.c_int32(t['spe'].shape[0]),
                                      *[C.c_void_p(t[k].ctypes.data) for k in ('gains', 'thr_truth', 'thr_zle', 'lum_x', 'lum_t')], C.c_int32(len(t['lum_x'])),
                                      C.c_void_p(noise.ctypes.data), C.c_int32(nl), C.c_int32(nc)))

    out = {}
    for mode in ('default', 'fresh'):
        eng = _engine('mixed20', 'default' if mode == 'default' else 'sync')
        assert eng.tables['noise'] is not None
        noise = np.ascontiguousarray(-eng.tables['noise'][::-1])           # another table of the same shape
        if mode == 'default':
            before = _result(eng, _load_and_run(eng, 'mixed20'))
            _load_and_run(eng, 'mixed20')                                    # (its packers read the old table while the setter is called)
            set_noise(eng, noise)
            out[mode] = _result(eng, eng.run())
            _assert_same(before, _fresh('mixed20'))
        else:
            set_noise(eng, noise)
            out[mode] = _result(eng, _load_and_run(eng, 'mixed20'))
        eng.close()
    _assert_same(out['default'], out['fresh'])
    assert out['default']['records'] != _fresh('mixed20')['records']


def test_torch_reader_and_lifetime_in_a_fresh_process():
    """copy_records_to_device into a torch tensor == records() (torch.cuda has to be initialised before the HIP library, hence a
    process of its own); and in that process, which holds no other engine: create, load, run, destroy without reading leaves
    wfs_device_allocations at 0 buffers and 0 bytes."""
    code = """
import torch
torch.cuda.init()
import numpy as np
from tests.test_gpu_deferred_pack import _engine, _load_and_run
from wfsim_amd.engine import device_allocations
eng = _engine('s2', 'default')
_load_and_run(eng, 's2')
counts = eng.run()
n = counts['n_records']
dev = torch.zeros(n * 244, dtype=torch.uint8, device='cuda')
eng.copy_records_to_device(dev.data_ptr(), n)
got = dev.cpu().numpy().tobytes()
assert n > 0 and got == eng.records().tobytes()
eng.close()
eng = _engine('s2', 'default')
_load_and_run(eng, 's2')
eng.close()
assert device_allocations() == (0, 0), device_allocations()
print('torch reader ok', n)
"""
    env = {k: v for k, v in os.environ.items() if k != 'WFS_PACK_SYNC'}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0 and 'torch reader ok' in r.stdout, r.stderr[-2000:]
