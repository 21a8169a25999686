"""Per-channel SPE rows on the reference and on the CPU oracle (tests/golden/spe_channels.npz; families, designed photon lists and the
law in tests/spe_channels.py; made by tests/golden/make_golden.py spe_channels).  CPU only.

A real SPE file has one column per PMT, so `row = channel` is the lookup production uses; the bundled configuration and every golden
chain have ONE column, and the chains replay photons with preassigned gains, which skips the lookup altogether.  Here:
  * the host table builder equals the reference's _Pulse__uniform_to_pe_arr row by row with ==, from dict(charge=, pdfs=), from a CSV
    and with 500 columns on 494 PMTs;
  * every photon of the reference's own Pulse calls (gains NOT preassigned) obeys the law gain == G[c] row[c][k], k >= 1, a double PE the
    float sum of two such terms -- under `delta` the gain names the row it was read from;
  * the oracle replays those calls (recorded gains injected) to the reference's pulses, rows and ZLE tuples;
  * the oracle's OWN generators (S1, S2 electron by electron, S2 tile by tile, supplied photons) obey the law photon by photon, and the
    truth areas are the sums of those gains over G;
  * three wrong row rules, compiled into copies of the oracle, each break the law -- the check has the power it claims.

Measured on the commit that adds the fixture (pytest -s prints them): per family 3 Pulse calls, 3002 photons on 494 channels (2879 on
live PMTs), 1020 (delta) and 1068 (shaped) double PEs, 577 pulses, 863 rows; the oracle's generators: 4 batches per family, 15 751
photons (S1 2879, S2 electron by electron 1944, S2 tile by tile 4394, supplied 6534), every channel hit.
First failing case of each mutation (batch s1, the first batch; photons in channel order):
  row_0          delta: photon 8, the first one on channel 1 (2871 of 2879 photons fail: all but those of channel 0)
  row_ch_plus_1  delta: photon 0 on channel 0 (2875 of 2879)
  stride_2000    delta: photon 36 on channel 5, the first one whose index k is not above its channel number -- position 2000 c + k is
                 index k - c of row c, or the tail of row c - 1 (405 of 2879); shaped: the same photon (17 of 2879: the law asks for a
                 MEMBER of the row, and index k - c of the right row is one; only index 0 and the other row's tail are not -- the device
                 tests compare every gain with the oracle's with ==, which sees a shifted index as well)
"""
import contextlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import spe_channels as SC
from tests.helpers import golden, make_oracle, replay_chain_on_oracle, with_fma
from wfsim_amd import tables as T
from wfsim_amd.config import kernel_params
from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

MS = 1_000_000
TRUTH_INT = ['n_photon', 'n_pe', 'n_photon_trigger', 'n_pe_trigger']
TRUTH_F64 = ['raw_area', 'raw_area_trigger']
_cache = {}


def fixture(family):
    if family not in _cache:
        g = golden('spe_channels.npz')
        assert tuple(str(x) for x in g['families']) == SC.FAMILIES
        _cache[family] = {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(family + '/')}
    return _cache[family]


def table_of(cfg):
    res = Resource(cfg)
    return T.spe_scaling_table(res.spe_charge, res.spe_pdfs)


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('form', ['pdfs', 'csv', 'wide'])
@pytest.mark.parametrize('family', SC.FAMILIES)
def test_table_equals_the_reference(family, form, tmp_path):
    """spe_scaling_table == the reference's table, every row: through dict(charge=, pdfs=) (on the axis as the reference parsed it), through
    a CSV path (Resource reads it with pandas, as the reference does) and with 500 columns on 494 PMTs; the design holds on it"""
    d = fixture(family)
    n = SC.N_WIDE if form == 'wide' else SC.N_TPC
    pad = SC.write_csv(family, str(tmp_path / 'spe.csv'), n) if form == 'csv' else SC.as_dict(family, n, charge=d['charge'])
    res = Resource(SC.config(family, photon_area_distribution=pad))
    assert res.spe_pdfs.shape == (n, len(d['charge'])) and np.array_equal(res.spe_charge, d['charge'])
    tab = T.spe_scaling_table(res.spe_charge, res.spe_pdfs)
    assert tab.shape == (n, SC.N_GRID) and tab.dtype == np.float64
    assert np.array_equal(tab, d['table'][:n])
    SC.assert_design(family, res.spe_pdfs, tab, d['charge'])
    # the axis a CSV gives back is the bundled one to the last ulp or so
    assert np.allclose(d['charge'], SC.charge_axis()[0], rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------------------------- the reference's photons
@pytest.mark.parametrize('family', SC.FAMILIES)
def test_reference_photons_obey_the_law(family):
    """every stored photon, no tolerance: the channel -> row rule on a run of the reference.  delta: the gain IS the channel's value
    times G, or that term twice for a double PE"""
    import json
    d = fixture(family)
    G = SC.gains()
    settings = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spe_channels_config.json')))
    assert settings['gains'] == G.tolist() and settings['p_double_pe_emision_high'] == SC.P_DPE_HIGH and settings['n_columns'] == len(d['table'])
    assert settings['special_columns'] == dict(zero=SC.ZERO_CH, first_positive_bin=SC.FIRST_CH, last_bin=SC.LAST_CH, gain_zero=SC.DEAD_CH)
    law = SC.Law(d['table'][:SC.N_TPC], G)
    assert not d['call_has_gains'].any() and len(d['call_kind']) == len(SC.reference_cases())
    bad = law.violations(d['ph_ch'], d['ph_dpe'], d['ph_gain'])
    assert len(bad) == 0, (family, len(bad), bad[:5], d['ph_ch'][bad[:5]], d['ph_gain'][bad[:5]])
    hit = np.bincount(d['ph_ch'], minlength=SC.N_TPC)
    assert hit.min() >= 1 and all(hit[c] >= 50 for c in SC.SPECIAL + SC.EDGE_CHANNELS)
    live = G[d['ph_ch']] > 0
    assert np.all(d['ph_gain'][~live] == 0) and (~live).sum() == hit[SC.DEAD_CH]
    a = int(d['call_ph_off'][-2])
    assert d['call_p_dpe'][-1] == SC.P_DPE_HIGH and d['ph_dpe'][a:].mean() > 0.5 and d['ph_dpe'][:a].any() and not d['ph_dpe'][:a].all()
    if family == 'delta':
        v = SC.delta_values(SC.N_TPC, d['charge'])
        term = G[d['ph_ch']] * v[d['ph_ch']]
        assert np.array_equal(d['ph_gain'], np.where(d['ph_dpe'], term + term, term))
        assert np.all(d['ph_gain'][d['ph_ch'] == SC.ZERO_CH] == 0) and len(set(v.tolist())) == SC.N_TPC
    else:
        # the photons of a channel spread over its row: the law is not met by a constant
        assert len(np.unique(d['ph_gain'][(d['ph_ch'] == 493) & ~d['ph_dpe']])) > 20
    print(f'\n{family}: {len(d["call_kind"])} calls, {len(d["ph_t"])} photons ({int(live.sum())} on live PMTs), {int(d["ph_dpe"].sum())} double PEs, '
          f'{int((hit > 0).sum())} channels, {len(d["pl_ch"])} pulses, {len(d["row_ch"])} rows, {len(d["zle_ch"])} intervals')


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
@pytest.mark.parametrize('family', SC.FAMILIES)
def test_oracle_replays_the_reference_calls(family, fma):
    """the recorded gains injected: pulse bounds, photon counts, windows, rows and ZLE tuples equal the fixture, the integer truth
    columns too, the area sums at rtol 1e-12 (as tests/test_pulse_edges_reference.py checks its fixtures)"""
    d = fixture(family)
    cfg = with_fma(SC.config(family, photon_area_distribution=SC.as_dict(family, SC.N_TPC, charge=d['charge'])), fma)
    orc = make_oracle(cfg)
    r = replay_chain_on_oracle(orc, d)
    for a, b in [('pl_ch', 'pl_ch'), ('pl_left', 'pl_left'), ('pl_right', 'pl_right'), ('pl_nph', 'pl_photons'), ('dg_left', 'dg_left'), ('dg_right', 'dg_right'),
                 ('row_ch', 'row_ch'), ('row_left', 'row_left'), ('row_right', 'row_right'), ('row_data', 'row_data')]:
        assert np.array_equal(r[a], d[b]), a
    for k in ['digit', 'ch', 'left', 'right', 'data_off', 'data']:
        assert np.array_equal(r['zl_' + k], d['zle_' + k]), k
    assert SC.DEAD_CH not in d['pl_ch'] and SC.ZERO_CH in d['pl_ch'] and len(d['dg_left']) == len(SC.GROUPS)
    tr = r['truth'].reshape(-1, 12)
    for j, f in enumerate(TRUTH_INT):
        assert np.array_equal(tr[:, j], d['call_truth_' + f].astype(np.float64)), f
        assert np.array_equal(tr[:, 6 + j], d['call_truth_' + f + '_bottom'].astype(np.float64)), f + '_bottom'
    for j, f in enumerate(TRUTH_F64):
        assert np.allclose(tr[:, 4 + j], d['call_truth_' + f], rtol=1e-12, atol=0), f
        assert np.allclose(tr[:, 10 + j], d['call_truth_' + f + '_bottom'], rtol=1e-12, atol=0), f + '_bottom'


# ---------------------------------------------------------------------------------------------------------------- the oracle's generators
def instructions(rows):
    ins = np.zeros(len(rows), dtype=instruction_dtype)
    for i, r in enumerate(rows):
        for k, v in r.items():
            ins[i][k] = v
        ins[i]['event_number'] = i
        ins[i]['recoil'] = 7
    return ins


def optical_instruction(cfg, group, time=MS):
    """one optical instruction over the supplied photons of a group (tests/spe_channels.py): (instructions, channels, timings, shapes)"""
    ch, tt, shape_of = SC.supplied_photons(group, len(cfg['gains']), int(cfg.get('sample_duration', 10)), time)
    ins = np.zeros(1, dtype=instruction_dtype + optical_extra_dtype)
    ins['type'], ins['time'], ins['amp'], ins['_first'], ins['_last'] = 1, time, len(ch), 0, len(ch)
    return ins, ch, tt, shape_of


def oracle_on_instructions(cfg, rows, resource=None, ap=None):
    """the oracle's generators on a batch of S1 / S2 instructions: everything a device run of the same batch needs as well"""
    ins = instructions(rows)
    res = resource or Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    orc = make_oracle(cfg, ap, resource=res)
    orc.simulate(s_ins, gid, ip)
    return dict(orc=orc, o=orc.results(), s_ins=s_ins, gid=gid, cluster=cluster, key=key, ip=ip, res=res, cfg=cfg)


def oracle_on_supplied_photons(cfg, group):
    ins, ch, tt, shape_of = optical_instruction(cfg, group)
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), ch, tt, int(1e6))
    return dict(orc=orc, o=orc.results(), ins=ins, channels=ch, timings=tt, shapes=shape_of, cfg=cfg)


SUPPLIED_OVERRIDES = dict(pmt_transit_time_spread=0.0, pmt_transit_time_mean=0.0)          # the designed lists reach the pulse kernels as they are


def generator_batches(family):
    """name -> a thunk that runs the oracle: S1 + S2 electron by electron, S2 tile by tile, supplied photons on the 494 channels"""
    block = SC.config(family, tile_local_generation=False, seed=41)
    tile = SC.config(family, s2_secondary_sc_gain=100.0, tile_local_min_photons=0, seed=42)
    optical = SC.config(family, seed=43, **SUPPLIED_OVERRIDES)
    assert kernel_params(block)['tile_gen'] == 0 and kernel_params(tile)['tile_gen'] == 1
    return dict(
        s1=lambda: oracle_on_instructions(block, [dict(type=1, time=MS, x=0, y=0, z=-30, amp=30000)]),
        s2_per_electron=lambda: oracle_on_instructions(block, [dict(type=2, time=MS, x=0, y=0, z=-8, amp=120)]),
        s2_tiles=lambda: oracle_on_instructions(tile, [dict(type=2, time=MS, x=0, y=0, z=-8, amp=60)]),
        supplied=lambda: oracle_on_supplied_photons(optical, 'dense_128_res'))


def law_failures(o, cfg):
    """(photons that break the law, calls whose truth areas are not the sums of the law's gains over G, photons in all)"""
    G = np.asarray(cfg['gains'], dtype=np.float64)
    law = SC.Law(table_of(cfg), G)
    bad = law.violations(o['ph_ch'], o['ph_dpe'], o['ph_gain'])
    bottom = np.asarray(cfg['channels_bottom'])
    tr = o['truth'].reshape(-1, 12)
    bad_calls = []
    for k, (a, b) in enumerate(zip(o['call_ph_off'][:-1], o['call_ph_off'][1:])):
        ok = np.isclose(tr[k, 4], law.area(o['ph_ch'][a:b], o['ph_gain'][a:b]), rtol=1e-9, atol=0) \
            and np.isclose(tr[k, 10], law.area(o['ph_ch'][a:b], o['ph_gain'][a:b], bottom), rtol=1e-9, atol=0)
        live = G[o['ph_ch'][a:b]] > 0
        ok = ok and tr[k, 0] == live.sum() and tr[k, 1] == live.sum() + o['ph_dpe'][a:b][live].sum()
        if not ok:
            bad_calls.append(k)
    return bad, bad_calls, len(o['ph_t'])


@pytest.mark.parametrize('family', SC.FAMILIES)
def test_oracle_generators_obey_the_law(family):
    """S1, S2 on the per-electron path, S2 on the tile path, supplied photons: every photon obeys the law, truth raw_area (all and
    bottom) is the sum of the law's gains over G at rtol 1e-9, n_photon / n_pe count the photons of live PMTs"""
    total, hit = 0, np.zeros(SC.N_TPC, dtype=np.int64)
    for name, run in generator_batches(family).items():
        r = run()
        o = r['o']
        bad, bad_calls, n = law_failures(o, r['cfg'])
        assert n > 1000 and not len(bad) and not bad_calls, (family, name, n, bad[:5], o['ph_ch'][bad[:5]], o['ph_gain'][bad[:5]], bad_calls)
        per = np.bincount(o['ph_ch'], minlength=SC.N_TPC)
        assert all(per[c] > 0 for c in SC.EDGE_CHANNELS + (SC.ZERO_CH,)) and o['ph_dpe'].any(), (name, per[list(SC.EDGE_CHANNELS)])
        if name != 'supplied':
            assert (per > 0).sum() >= 450 and per[SC.DEAD_CH] == 0         # (s1.py:149 / s2.py:647: no light on a turned-off PMT)
        print(f'\n{family} / {name}: {n} photons, {int(o["ph_dpe"].sum())} double PEs, {int((per > 0).sum())} channels')
        total += n
        hit += per
        r['orc'].close()
    assert (hit > 0).sum() == SC.N_TPC            # (the supplied photons reach the turned-off PMT too: they carry no gain)
    print(f'{family}: {total} photons in all')


# ---------------------------------------------------------------------------------------------------------------- power
ROW_RULE = 'int sc = c->n_spe_channels > ch ? ch : 0;'
ROW_STRIDE = 's->spe + (i64)sc * 2001;'
MUTATIONS = dict(
    row_0=(ROW_RULE, 'int sc = 0;'),
    row_ch_plus_1=(ROW_RULE, 'int sc = ch + 1 < c->n_spe_channels ? ch + 1 : c->n_spe_channels - 1;'),
    stride_2000=(ROW_STRIDE, 's->spe + (i64)sc * 2000;'))


@contextlib.contextmanager
def oracle_library(path):
    """oracle.oracle bound to another build of the library for the length of the block"""
    import oracle.oracle as O
    saved = (O._lib, O.LIB_PATH)
    O._lib, O.LIB_PATH = None, path
    try:
        O.lib()
        yield
    finally:
        O._lib, O.LIB_PATH = saved


@pytest.mark.parametrize('mutation', sorted(MUTATIONS))
def test_a_wrong_row_rule_breaks_the_law(mutation, tmp_path):
    """the oracle's C with the row rule broken at its three sites (one_photon, the tile loop of gen_s2, orc_optical), built in a
    temporary directory: every generator batch fails the `delta` law, and the stride of 2000 fails `shaped` as well.  First failing
    cases: see the head of this file"""
    import oracle.oracle as O
    old, new = MUTATIONS[mutation]
    src = open(os.path.join(O.HERE, 'wfsim_oracle.c')).read()
    assert src.count(old) == 3, (mutation, src.count(old))
    (tmp_path / 'wfsim_oracle.c').write_text(src.replace(old, new))
    shutil.copy(os.path.join(O.HERE, 'Makefile'), tmp_path / 'Makefile')
    subprocess.check_call(['make', '-C', str(tmp_path), '-s'])
    O.lib()                                  # (the real library is loaded and stays the one everybody else gets)
    with oracle_library(str(tmp_path / '_build' / 'liboracle.so')):
        for family in SC.FAMILIES if mutation == 'stride_2000' else ('delta',):
            for name, run in generator_batches(family).items():
                r = run()
                bad, bad_calls, n = law_failures(r['o'], r['cfg'])
                r['orc'].close()
                assert len(bad) > 0, (mutation, family, name)
                if mutation != 'stride_2000':          # (a wrong row is wrong for every photon but those of the rows that agree)
                    assert len(bad) > n // 2, (mutation, family, name, len(bad), n)
                print(f'\n{mutation} / {family} / {name}: {len(bad)} of {n} photons break the law, first: photon {bad[0]} on channel {r["o"]["ph_ch"][bad[0]]}')
    # and the real library still obeys it
    r = generator_batches('delta')['supplied']()
    assert not len(law_failures(r['o'], r['cfg'])[0])
