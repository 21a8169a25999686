"""The binding's argument rules (wfsim_amd/abi.py) on the device, with the two-instruction S1 + S2 batch of smoke():
inputs of another dtype or layout are converted for the call, outputs of another dtype or without write access are refused in Python
before the library is entered, and the batch-scoped state of the Engine is replaced whole by every load."""
import functools

import numpy as np
import pytest

from tests.helpers import make_engine
from wfsim_amd import workloads as W
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _batch():
    cfg = xenonnt_test_config(seed=11)
    ins = np.zeros(2, dtype=instruction_dtype)
    ins['type'], ins['time'], ins['z'], ins['amp'], ins['recoil'] = [1, 2], [1_000_000, 1_000_000], -10.0, [1500, 300], 7
    order, key, cluster = schedule(ins, cfg)
    return cfg, ins[order], order.astype(np.uint32), cluster, key, instruction_params(ins[order], cfg, Resource(cfg))


def _strided(a, dtype):
    """the values of ``a`` as every second element of an array of ``dtype``"""
    wide = np.full(2 * len(a), -1, dtype=dtype)
    wide[::2] = a
    view = wide[::2]
    assert not view.flags.c_contiguous or len(a) < 2
    return view


def test_inputs_of_another_dtype_and_layout_give_the_same_records():
    cfg, ins, gid, cluster, key, ip = _batch()
    eng = make_engine(cfg)
    eng.load_instructions(ins, gid, cluster, key, ip)
    counts = eng.run()
    assert counts['n_records'] > 0
    records = eng.records().copy()
    eng.load_instructions(ins, _strided(gid, np.int64), _strided(cluster, np.int64), _strided(key, np.int64), ip)
    assert eng.run() == counts
    assert eng.records().tobytes() == records.tobytes()
    # int64 where the header says int32_t / uint32_t, handed over as they are and as plain lists
    eng.load_instructions(ins, gid.astype(np.int64), [int(c) for c in cluster], np.asarray(key, dtype=np.int64), ip)
    assert eng.run() == counts
    assert eng.records().tobytes() == records.tobytes()
    eng.close()


def test_outputs_of_another_dtype_are_refused_before_the_library():
    cfg, ins, gid, cluster, key, ip = _batch()
    eng = make_engine(cfg)
    eng.load_instructions(ins, gid, cluster, key, ip)
    g = eng.run()['n_groups']
    assert g > 0
    groups, records = eng.groups(), eng.records().copy()
    ok = [np.zeros(g, dtype=np.int64) for _ in range(3)]
    narrow = np.full(g, -7, dtype=np.int32)                 # half the bytes the library would write
    with pytest.raises(TypeError, match='wfs_copy_groups.*left'):
        eng.lib.wfs_copy_groups(eng._h, narrow, *ok)
    read_only = np.full(g, -7, dtype=np.int64)
    read_only.flags.writeable = False
    with pytest.raises(TypeError, match='wfs_copy_groups.*left'):
        eng.lib.wfs_copy_groups(eng._h, read_only, *ok)
    with pytest.raises(TypeError, match='wfs_copy_groups.*ix_rand'):
        eng.lib.wfs_copy_groups(eng._h, *ok, narrow)
    assert np.all(narrow == -7) and np.all(read_only == -7) and not any(a.any() for a in ok)          # nothing was written anywhere
    again = eng.groups()
    assert all(np.array_equal(again[k], groups[k]) for k in groups)
    assert eng.records().tobytes() == records.tobytes()
    # the same buffers with the header's dtype are filled
    left = np.zeros(g, dtype=np.int64)
    assert eng.lib.wfs_copy_groups(eng._h, left, *ok) == 0 and np.array_equal(left, groups['left']) and np.array_equal(ok[0], groups['right'])
    eng.close()


def test_two_loads_on_one_engine_replace_the_batch_state():
    """load_instructions with run sets (numbered against their order of appearance: the library's rows are [1, 0]), then load_optical on
    the same engine: truth(), photons() and counts['n_pulse_sets'] of the optical batch are the library's own rows"""
    cfg, ins, gid, cluster, key, ip = _batch()
    eng = make_engine(cfg)
    eng.load_instructions(ins, gid, cluster, key, ip)
    eng.run()
    plain = eng.truth()[0].copy()
    eng.load_instructions(ins, gid, cluster, key, ip, run_set=np.array([1, 0]))
    counts = eng.run()
    assert eng._batch.set_rows.tolist() == [1, 0] and counts['n_pulse_sets'] == 2
    assert np.array_equal(eng.truth()[0], plain[[1, 0]]) and np.all(plain[:, 0] > 0)
    oins, channels, timings = W.optical_instructions(20, 1000.0, 3)
    order, okey, ocluster = schedule(oins, cfg)
    args = (oins[order], order.astype(np.uint32), ocluster, okey, channels, timings, int(1e6))
    eng.load_optical(*args)
    assert eng._batch.set_rows is None and eng._batch.n_run_sets is None and eng._batch.n_loaded == 20
    counts = eng.run()
    fresh = make_engine(cfg)
    fresh.load_optical(*args)
    fresh_counts = fresh.run()
    assert counts == fresh_counts and counts['n_pulse_sets'] == eng._lib_sets == fresh._lib_sets >= 20
    assert eng._caller_sets(eng._lib_sets) is None
    acc, ts = eng.truth()
    assert len(acc) == eng._lib_sets and acc[:, 0].sum() > 0
    assert np.array_equal(acc, fresh.truth()[0]) and np.array_equal(ts, fresh.truth()[1], equal_nan=True)
    ph, fresh_ph = eng.photons(), fresh.photons()
    assert len(ph['set_off']) == eng._lib_sets + 1 and all(np.array_equal(ph[k], fresh_ph[k]) for k in ph)
    assert len(eng.electron_stats()) == 20
    eng.close()
    fresh.close()
