"""Full readout: the zero-gain anchors of tests/full_readout.py on the oracle alone.

The GPU tests compare the engine in full-readout mode with the oracle on anchored input.  What that pin rests on is checked here without
a GPU: the anchors leave every designed window, its ix_rand and its rows with pulses untouched, give every row slot a row of the union
range, and the chosen inputs reach the seams the GPU test relies on.  The counts below are conditions on the inputs, not measurements.
"""
import numpy as np
import pytest

from tests import full_readout as FR
from tests import noise_slow as NS
from tests.helpers import with_fma
from tests.noise_model import oracle_rows
from tests.test_gpu_noise_model import _off_config, _oracle_photons
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.noise_model import noise_colour, noise_pmf, noise_slow


def _config(channels, tw):
    base = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20 if channels == 801 else 0, trigger_window=tw, seed=1234 + channels), False)
    return dict(base, enable_noise=True, noise_model={'sigma': FR.sigmas(channels)})


@pytest.fixture(scope='module', params=[(494, 50), (801, 20)], ids=['494-tw50', '801-tw20'])
def case(request):
    channels, tw = request.param
    cfg = _config(channels, tw)
    p = kernel_params(cfg)
    windows = FR.windows_of(p)
    sets, calls, anchored = FR.photon_input(cfg, p, windows)
    pmf, vmin = noise_pmf(cfg, 801)
    model = NS.slow_model(pmf, vmin, noise_colour(cfg, 801), noise_slow(cfg, 801))
    orc, tab_cfg, ix, rows = FR.model_expectation(cfg, model, int(p['seed']), calls, anchored)
    plain_off = _oracle_photons(_off_config(cfg), calls).results()
    plain = _oracle_photons(tab_cfg, calls, ix).results()
    o_off = _oracle_photons(_off_config(cfg), anchored).results()
    return dict(cfg=cfg, p=p, windows=windows, calls=calls, o=orc.results(), o_off=o_off, plain=plain, plain_off=plain_off, rows=rows, tab_cfg=tab_cfg, ix=ix, channels=channels)


def test_anchors_leave_the_windows_alone(case):
    o, plain = case['o'], case['plain']
    assert len(o['dg_left']) == len(case['windows'])
    for k in ('dg_left', 'dg_right', 'dg_ix_rand'):
        assert np.array_equal(o[k], plain[k]), k
    # ... and a table whose start index is DRAWN: the range of the draw (rawdata.py:407-417) is the union range with or without them
    noise = np.random.default_rng(5).integers(-9, 10, size=(9000, 494)).astype(np.int16)
    cfg = dict({k: v for k, v in case['cfg'].items() if k != 'noise_model'}, noise_data=noise)
    sets, calls, anchored = FR.photon_input(cfg, case['p'], case['windows'])
    a, b = _oracle_photons(cfg, calls).results(), _oracle_photons(cfg, anchored).results()
    assert np.array_equal(a['dg_ix_rand'], b['dg_ix_rand']) and a['dg_ix_rand'].max() > 0
    # without noise (which counts from the row's first sample) the rows with pulses hold the same samples where they had some
    o, plain = case['o_off'], case['plain_off']
    full = {(w, ch): (first, n) for w, ch, first, n in oracle_rows(o)}
    off, poff = o['row_data_off'], plain['row_data_off']
    assert off[0] == 0 and poff[0] == 0 and len(off) == len(o['row_ch']) + 1
    index = {(w, ch): r for r, (w, ch, _, _) in enumerate(oracle_rows(o))}
    for r, (w, ch, first, n) in enumerate(oracle_rows(plain)):
        f0, fn = full[(w, ch)]
        assert f0 <= first and first + n <= f0 + fn
        q = index[(w, ch)]
        assert np.array_equal(o['row_data'][off[q] + first - f0:off[q] + first - f0 + n], plain['row_data'][poff[r]:poff[r + 1]])


def test_every_slot_has_a_row_of_the_union_range(case):
    o, p = case['o'], case['p']
    n_tpc, n_top, he = int(p['n_tpc']), int(p['n_top']), int(p['he_first'])
    slots = list(range(n_tpc)) + list(range(he, he + n_top))
    tw = int(p['trigger_window'])
    for w in range(len(o['dg_left'])):
        a, b = int(o['dg_row_off'][w]), int(o['dg_row_off'][w + 1])
        assert o['row_ch'][a:b].tolist() == slots
        lo = min(r[2] for r in oracle_rows(case['plain_off']) if r[0] == w)
        hi = max(r[2] + r[3] for r in oracle_rows(case['plain_off']) if r[0] == w)
        assert np.all(o['dg_left'][w] + o['row_left'][a:b] == lo) and np.all(o['dg_left'][w] + o['row_right'][a:b] == hi - 1)
        assert o['dg_right'][w] == hi - 1 and o['dg_left'][w] in (lo, lo - 1) and lo + tw <= hi - 1 - tw


def test_inputs_reach_the_seams(case):
    o, p = case['o'], case['p']
    rows = case['rows']
    first, length = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    assert set((first % 4).tolist()) == {0, 1, 2, 3} and set((length % 4).tolist()) == {0, 1, 2, 3}
    assert 256 in length and 257 in length and length.max() > 2048
    assert np.any((first < FR.T34) & (first + length > FR.T34)) and first.max() > FR.T34
    empty = {(r[0], r[1]): r for r in FR.pulse_less(case['plain_off'], o)}
    assert len(empty) == len(rows) - len(oracle_rows(case['plain_off'])) > 0.8 * len(rows)
    with_itv = {}
    for w, ch, l, r in zip(o['zl_digit'].tolist(), o['zl_ch'].tolist(), o['zl_left'].tolist(), o['zl_right'].tolist()):
        if (w, ch) in empty:
            with_itv.setdefault((w, ch), []).append((l, r))
    n_tpc = int(p['n_tpc'])
    tpc_empty = [k for k in empty if k[1] < n_tpc]
    assert len(with_itv) >= 20 and len([k for k in tpc_empty if k not in with_itv]) >= 20
    assert all(k[1] != FR.QUIET for k in with_itv)                   # sigma 0: a flat row
    at_start = [k for k, v in with_itv.items() if any(l == empty[k][2] for l, _ in v)]                 # (clipped at the row's first sample, which is even relative to the row)
    at_end = [k for k, v in with_itv.items() if any(empty[k][2] + empty[k][3] - 1 - r <= 1 for _, r in v)]
    assert at_start and at_end                                       # an interval clipped at either end of its row (the even landing can move the right end down by one)


def test_a_batch_is_sized_by_row_slots_and_window_length():
    """RawData bounds a batch by its expected records (ChunkRawRecords: half its record buffer): with the key every instruction costs
    row slots x the record fragments of a window on top, so the first batch of a full-readout run is not sized for a tenth of its records"""
    import types
    from wfsim_amd.dtypes import instruction_dtype
    from wfsim_amd.rawdata import RawData, full_readout_records
    ins = np.zeros(200, dtype=instruction_dtype)
    ins['type'], ins['amp'], ins['time'] = np.tile([1, 2], 100), np.tile([3000, 1500], 100), 1_000_000 * (1 + np.arange(200) // 2)
    cluster = np.arange(200) // 2
    for channels, slots in ((494, 494), (801, 494 + 253)):
        cfg = _config(channels, 50)
        p = kernel_params(cfg)
        extra = full_readout_records(cfg, p, ins)
        window = 2 * 50 + int(p['store_before']) + int(p['store_after']) + int(p['tlen'])
        assert np.array_equal(extra[ins['type'] == 1], np.full(100, slots * np.ceil((window + 30) / 110)))
        assert np.array_equal(extra[ins['type'] == 2], np.full(100, slots * np.ceil((window + 300) / 110)))
        stops = {}
        for on in (False, True):
            stub = types.SimpleNamespace(config=dict(cfg, full_readout=on), engine=types.SimpleNamespace(params=p), max_batch_quanta=10 ** 12,
                                         record_budget=400_000, _rec_scale=1.0, cut_period=None, cut_origin=0)
            stub._expected_quanta = lambda s, stub=stub: RawData._expected_quanta(stub, s)
            rec = RawData._expected_records(stub, ins)
            assert np.array_equal(rec - RawData._expected_records(types.SimpleNamespace(config=cfg, _expected_quanta=stub._expected_quanta), ins), extra if on else 0 * extra)
            stops[on] = RawData._batch_end(stub, 0, np.cumsum(RawData._expected_quanta(stub, ins)), cluster, rec_csum=np.cumsum(rec))
            if on:
                assert rec[:stops[True]].sum() <= 400_000 + 2 * rec.max() < rec.sum()      # bounded by the records full readout expects
        assert stops[False] == 200 and stops[True] % 2 == 0 and stops[True] < 0.7 * stops[False]
