"""Per-channel SPE rows in every kernel that looks a gain up (MI355X only).

Every pulse kernel picks its row with d.spe + (n_spe > 1 ? ch : 0) * 2001: k_pulse_dense (wfs_kernels.h k_pulse), k_pulse_generic,
k_pulse_tiny (tiny_tile_prepare), k_pulse_wave (wave_tile_pulse), k_pulse_sparse, k_row_pulse (through the tiny and the wave
functions), k_s2_tile and k_s2_bright (wfs_tilegen.h, the row staged into LDS), and the host read-back behind Engine.photons().  The bundled configuration has ONE row, so no other test runs the branch a
real SPE file (one column per PMT) takes.  tests/spe_channels.py holds the two families of columns (`delta`: the gain names its row;
`shaped`: full step functions), tests/test_spe_channels_reference.py pins the CPU oracle on the reference under both.  Here every case
runs under both families and is compared with the oracle as tests/test_gpu_generation.py::_compare does -- photons (t, ch, dpe, gain),
digitise windows, record bytes, n_pe -- plus the 12 truth columns of every call, paired by set index, and the 6 per-PMT truth columns
of every hit channel at rtol 1e-9.  Engine.photons() resolves the gain codes on the HOST, so records and truth are what show the
kernels' own lookups; under `delta` one check needs no oracle: per-PMT raw_area == per-PMT n_pe x the channel's value.
Which kernel ran is asserted from kernel_times() / tile_kernels(); every launch is checked on the spot (WFS_CHECK_LAUNCHES=1).

Power, measured once on the commit that adds this file: seven scratch builds of the library, each with ONE lookup site reading row 0
(in bounds), against these 62 tests.  k_pulse: 24 fail (every dense group, the dense groups of the 120- and 500-column cases, the
bright tiles on the photon-array routes); k_pulse_generic: the 14 generic cases; tiny_tile_prepare (k_pulse_tiny): 12 (the tiny groups,
the other channel counts, the block generator, the afterpulse parents); wave_tile_pulse: 8 (the wave groups through k_pulse_wave, the
sparse groups through k_row_pulse on resident rows); k_pulse_sparse: the 4 sparse groups; k_s2_tile: 12 (its own cases, the ordinary
tiles of the bright cases, the afterpulse parents); k_s2_bright: the 2 cases that take it.  No site goes unnoticed.
"""
import numpy as np
import pytest

from tests import pulse_edges as PE
from tests import spe_channels as SC
from tests.helpers import ap_tables_from_golden, assert_tiles_in_oracle_order, make_engine, optical_chain_config, pulse_edges_config, with_fma
from tests.test_gpu_generation import _call_sets
from tests.test_spe_channels_reference import MS, SUPPLIED_OVERRIDES, oracle_on_instructions, oracle_on_supplied_photons, table_of
from wfsim_amd import tables as T
from wfsim_amd.config import N_ROWS, current_2_adc
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu
FMA = pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fused'])
FAMILY = pytest.mark.parametrize('family', SC.FAMILIES)


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')


def _per_pmt_of_call(cfg, o, call):
    """pulse.py:229-271 per channel of one Pulse call from the oracle's photons in their order inside the channel: [n_tpc][6]"""
    a, b = o['call_ph_off'][call], o['call_ph_off'][call + 1]
    G = np.asarray(cfg['gains'], dtype=np.float64)
    dt = int(cfg.get('sample_duration', 10))
    cmax = T.pmt_current_templates(cfg).max(axis=1)
    thr = T.thresholds(cfg, N_ROWS)[0]
    c2a = current_2_adc(cfg)
    out = np.zeros((len(G), 6))
    for ch in np.unique(o['ph_ch'][a:b]):
        if G[ch] == 0:
            continue                  # (pulse.py:89, 237: nothing is made of the photons of a turned-off PMT)
        sel = o['ph_ch'][a:b] == ch
        t, gain, dpe = o['ph_t'][a:b][sel], o['ph_gain'][a:b][sel], o['ph_dpe'][a:b][sel]
        above = gain * cmax[t % dt] * c2a > thr[ch]
        n, n_dpe = len(t), int(dpe.sum())
        out[ch] = [n, n + n_dpe, above.sum(), above.sum() + above[:n_dpe].sum(), gain.sum() / G[ch], gain[above].sum() / G[ch]]
    return out


def _compare(family, cfg, orc, o, eng, counts, sets, must_hit=None):
    """device against oracle, set by set (sets[k]: the device pulse set of oracle call k); returns the photons of the primary calls.
    Every tile in the oracle's order (tests/helpers.py: assert_tiles_in_oracle_order) -- supplied photons (load_optical) too: DESIGN.md 4
    leaves their order inside a channel unpinned against the REFERENCE (numpy's unstable argsort), device and oracle both keep the input's."""
    G = np.asarray(cfg['gains'], dtype=np.float64)
    n_ch = len(G)
    ph = eng.photons()
    # (supplied photons on a turned-off PMT: the oracle lists them, with gain 0, the device may drop them on entry -- nothing is made of them)
    assert counts['n_photons'] in (len(o['ph_t']), int((G[o['ph_ch']] > 0).sum())) and len(sets) == len(o['call_kind'])
    for k, i in enumerate(sets):
        a, b = o['call_ph_off'][k], o['call_ph_off'][k + 1]
        c, e = ph['set_off'][i], ph['set_off'][i + 1]
        mo, mg = np.flatnonzero(G[o['ph_ch'][a:b]] > 0), np.flatnonzero(G[ph['ch'][c:e]] > 0)
        assert len(mo) == len(mg), f'call {k}, set {i}: {len(mo)} vs {len(mg)} photons on live PMTs'
        ko = mo[np.lexsort((o['ph_gain'][a:b][mo], o['ph_t'][a:b][mo], o['ph_ch'][a:b][mo]))]
        kg = mg[np.lexsort((ph['gain'][c:e][mg], ph['t'][c:e][mg], ph['ch'][c:e][mg]))]
        for f, g in [('ph_ch', 'ch'), ('ph_t', 't'), ('ph_dpe', 'dpe'), ('ph_gain', 'gain')]:
            assert np.array_equal(o[f][a:b][ko], ph[g][c:e][kg]), (k, i, f)
    assert_tiles_in_oracle_order(eng, o, sets, live=G > 0)
    g = eng.groups()
    keep = g['right'] >= g['left']
    assert np.array_equal(g['left'][keep], o['dg_left']) and np.array_equal(g['right'][keep], o['dg_right'])
    assert eng.records().tobytes() == orc.pack_records().tobytes()
    assert counts['n_pe'] == orc.n_pe
    # ---- truth: the 12 columns of every call, the 6 per-PMT columns of every channel (hit or not)
    acc, ts = eng.truth()
    tr = o['truth'].reshape(-1, 12)
    per_pmt = eng.truth_per_pmt()
    assert len(tr) == len(sets) and per_pmt.shape == (len(acc), n_ch, 6)
    law = SC.Law(table_of(cfg), G)
    v = SC.delta_values(n_ch)
    n_primary = 0
    for k, i in enumerate(sets):
        assert np.allclose(acc[i], tr[k], rtol=1e-9, atol=0), (k, i, acc[i], tr[k])
        ref = _per_pmt_of_call(cfg, o, k)
        assert np.allclose(per_pmt[i], ref, rtol=1e-9, atol=0), (k, i, np.argwhere(~np.isclose(per_pmt[i], ref, rtol=1e-9, atol=0))[:5])
        if o['call_kind'][k] == 3:
            continue                  # (afterpulse gains are G x the drawn amplitude: they bypass the SPE table)
        n_primary += 1
        c, e = ph['set_off'][i], ph['set_off'][i + 1]
        # the host read-back on its own: every gain the device reports obeys the law
        bad = law.violations(ph['ch'][c:e], ph['dpe'][c:e], ph['gain'][c:e])
        assert not len(bad), (k, i, len(bad), ph['ch'][c:e][bad[:5]], ph['gain'][c:e][bad[:5]])
        if family == 'delta':
            # oracle-independent: the kernel that made the truth read the channel's own row
            hit = np.flatnonzero(per_pmt[i][:, 0] > 0)
            assert np.allclose(per_pmt[i][hit, 4], per_pmt[i][hit, 1] * v[hit], rtol=1e-9, atol=0), (k, i)
            assert len(hit) == len(np.unique(ph['ch'][c:e][G[ph['ch'][c:e]] > 0]))
    assert not acc[np.setdiff1d(np.arange(len(acc)), sets)].any()
    primary = np.concatenate([np.arange(ph['set_off'][i], ph['set_off'][i + 1]) for k, i in enumerate(sets) if o['call_kind'][k] != 3])
    hit = np.bincount(ph['ch'][primary], minlength=n_ch)
    for c in (0, n_ch - 1, SC.ZERO_CH) + ((252, 253) if n_ch == SC.N_TPC else ()) + tuple(must_hit or ()):
        assert hit[c] > 0 or c == SC.DEAD_CH, f'no photon on channel {c}'
    return dict(photons=int(counts['n_photons']), channels=int((hit > 0).sum()), dpe=int(ph['dpe'][primary].sum()))


def _engine(cfg, resource=None):
    eng = make_engine(cfg, resource=resource)
    eng.set_profiling(True)
    return eng


def _device_on_instructions(r, cfg=None):
    """the batch of an oracle_on_instructions() result on a fresh engine"""
    eng = _engine(cfg or r['cfg'], r['res'])
    eng.load_instructions(r['s_ins'], r['gid'], r['cluster'], r['key'], r['ip'])
    return eng, eng.run()


def _device_on_supplied_photons(r, cfg=None):
    cfg = cfg or r['cfg']
    eng = _engine(cfg)
    order, key, cluster = schedule(r['ins'], cfg)
    assert np.array_equal(order, np.arange(len(r['ins'])))
    eng.load_optical(r['ins'], order.astype(np.uint32), cluster, key, r['channels'], r['timings'], int(1e6))
    return eng, eng.run()


def _tile_kernels(kt):
    return sorted(k for k in kt if k in PE.TILE_KERNELS)


def _log(what, family, kt, m, extra=''):
    print(f'\n{what} / {family}: {m["photons"]} photons ({m["dpe"]} double PEs) on {m["channels"]} channels; kernels {_tile_kernels(kt) + [k for k in ("k_row_pulse", "k_photon_fill", "k_s2_tile", "k_s2_tile_gen", "k_s2_bright", "k_optical_finish") if k in kt]}{extra}')


# ---------------------------------------------------------------------------------------------------------------- supplied photons
@FMA
@pytest.mark.parametrize('group', sorted(SC.SUPPLIED_GROUPS))
@FAMILY
def test_supplied_photons_on_each_pulse_kernel(family, group, fma, monkeypatch):
    """load_optical on the 494-channel configuration (k_optical_finish draws the gain codes), transit spread 0: per-channel photon lists
    on both sides of every tile-class boundary, one group per kernel -- k_pulse_tiny, k_pulse_sparse, k_pulse_wave, k_pulse_dense with
    128 and 256 threads, photons resident in registers and windowed -- on the accumulator rows; then with row_resident on, 1024- and
    256-sample segments: k_row_pulse makes the rows of the tiny, sparse and wave groups, the dense groups keep k_pulse_dense; the same
    record bytes"""
    cfg = with_fma(SC.config(family, seed=51, row_resident=False, **SUPPLIED_OVERRIDES), fma)
    r = oracle_on_supplied_photons(cfg, group)
    eng, counts = _device_on_supplied_photons(r)
    kt = eng.kernel_times()
    cls = group.split('_')[0]
    assert 'k_optical_finish' in kt and _tile_kernels(kt) == [PE.KERNEL_OF_CLASS[cls]], (group, sorted(kt))
    ph = eng.photons()
    shapes = SC.tile_shapes(ph['set_off'], ph['t'], ph['ch'], 10)[0]
    shapes.pop(SC.DEAD_CH, None)          # (whether the device lists the photons of the turned-off PMT is its business)
    assert shapes == {c: s for c, s in r['shapes'].items() if c != SC.DEAD_CH} and all(PE.tile_class(*s) == cls for s in shapes.values()), (group, shapes)
    if cls == 'dense':
        mx_n, mx_nb = max(s[0] for s in shapes.values()), max(s[1] for s in shapes.values())
        assert PE.dense_variant(mx_nb, mx_n)[:2] == SC.DENSE_VARIANT[group], (group, mx_n, mx_nb)
    m = _compare(family, cfg, r['orc'], r['o'], eng, counts, [0], must_hit=SC.supplied_channels())
    records = eng.records().tobytes()
    ran = {}
    for mode in ('res', 'res256'):
        if mode == 'res256':
            monkeypatch.setenv('WFS_RES_MAX_LEN', '256')
        cfg_r = dict(cfg, row_resident=True)
        eng_r, counts_r = _device_on_supplied_photons(r, cfg_r)
        kt_r = eng_r.kernel_times()
        if cls != 'dense':
            assert 'k_row_pulse' in kt_r and not _tile_kernels(kt_r), (group, mode, sorted(kt_r))          # every row of the group is made by k_row_pulse
        else:
            assert 'k_row_pulse' not in kt_r and _tile_kernels(kt_r) == ['k_pulse_dense'], (group, mode, sorted(kt_r))      # (dense tiles keep the accumulator rows)
        assert eng_r.records().tobytes() == records, (group, mode)
        _compare(family, cfg_r, r['orc'], r['o'], eng_r, counts_r, [0])
        ran[mode] = sorted(k for k in kt_r if k in PE.TILE_KERNELS or k == 'k_row_pulse')
    _log(f'supplied {group} {"fused" if fma else "exact"}', family, kt, m, f'; row_resident on: {ran}')


@pytest.mark.parametrize('group', sorted(SC.SUPPLIED_GROUPS))
@FAMILY
def test_supplied_photons_on_the_generic_kernel(family, group):
    """the same lists with 5 ns samples and 3 + 37 template samples: every tile of every group through k_pulse_generic"""
    base = pulse_edges_config('pulse_edges_geometry.npz')
    cfg = SC.config(family, base=base, seed=52, **SUPPLIED_OVERRIDES)
    r = oracle_on_supplied_photons(cfg, group)
    eng, counts = _device_on_supplied_photons(r)
    kt = eng.kernel_times()
    assert _tile_kernels(kt) == ['k_pulse_generic'] and 'k_row_pulse' not in kt, sorted(kt)
    m = _compare(family, cfg, r['orc'], r['o'], eng, counts, [0], must_hit=SC.supplied_channels())
    _log(f'generic geometry {group}', family, kt, m)


@pytest.mark.parametrize('n_columns', [120, SC.N_WIDE])
@FAMILY
def test_other_channel_counts(family, n_columns):
    """120 nVeto channels with 120 rows (the configuration of the optical chains, its channel 7 dead), and 500 columns on 494 channels
    (n_spe > n_tpc): the tiny and the 256-thread dense group (the row staged in LDS) against the oracle"""
    base = optical_chain_config('main') if n_columns == 120 else None
    cfg = SC.config(family, n_columns, base=base, seed=53, row_resident=False, **SUPPLIED_OVERRIDES)
    assert len(cfg['gains']) == min(n_columns, SC.N_TPC) and table_of(cfg).shape[0] == n_columns
    for group in ('tiny', 'dense_256_res'):
        r = oracle_on_supplied_photons(cfg, group)
        eng, counts = _device_on_supplied_photons(r)
        kt = eng.kernel_times()
        assert 'k_optical_finish' in kt and _tile_kernels(kt) == [PE.KERNEL_OF_CLASS[group.split('_')[0]]], (group, sorted(kt))
        m = _compare(family, cfg, r['orc'], r['o'], eng, counts, [0], must_hit=SC.supplied_channels(len(cfg['gains'])))
        _log(f'{n_columns} columns {group}', family, kt, m)


def test_fewer_rows_than_channels_are_refused():
    """2 <= n_spe < n_tpc: wfs_set_tables returns from its host check, before anything is uploaded or launched"""
    from wfsim_amd.engine import WfsError
    with pytest.raises(WfsError, match='n_spe must be 1 or >= n_tpc'):
        make_engine(SC.config('delta', 100))


# ---------------------------------------------------------------------------------------------------------------- generated photons
@FAMILY
def test_block_generator(family):
    """one S1 of 3000 PE and one S2 of 5 electrons: k_photon_fill makes the photons, the pulse kernels look the gains up (386 photons:
    the seed is the first from 54 up with which channels 0, 252, 253, 493 and the all-zero column are hit, found with the oracle)"""
    cfg = SC.config(family, seed=90)
    r = oracle_on_instructions(cfg, [dict(type=1, time=MS, x=0, y=0, z=-30, amp=3000), dict(type=2, time=3 * MS, x=0, y=0, z=-8, amp=5)])
    eng, counts = _device_on_instructions(r)
    kt = eng.kernel_times()
    assert 'k_photon_fill' in kt and 'k_s2_tile' not in kt and not eng.tile_kernels().any(), sorted(kt)
    m = _compare(family, cfg, r['orc'], r['o'], eng, counts, _call_sets(r['o'], r['s_ins'], cfg))
    _log('block generator', family, kt, m)


@FMA
@FAMILY
def test_s2_tile(family, fma):
    """one S2 of 300 electrons, s2_secondary_sc_gain 100, every tile generated and pulsed by k_s2_tile (the row comes through
    global_load_lds into the workgroup's LDS)"""
    cfg = with_fma(SC.config(family, s2_secondary_sc_gain=100.0, tile_local_min_photons=0, seed=55), fma)
    r = oracle_on_instructions(cfg, [dict(type=2, time=MS, x=0, y=0, z=-8, amp=300)])
    eng, counts = _device_on_instructions(r)
    kt = eng.kernel_times()
    kind = eng.tile_kernels()
    assert 'k_s2_tile' in kt and 'k_photon_fill' not in kt and not _tile_kernels(kt), sorted(kt)
    assert (kind == 1).sum() >= 490 and not (kind > 1).any()
    m = _compare(family, cfg, r['orc'], r['o'], eng, counts, _call_sets(r['o'], r['s_ins'], cfg))
    _log(f's2 tile {"fused" if fma else "exact"}', family, kt, m)


HOT = {0: 0.05, 17: 0.05, 300: 0.01, 493: 0.05}
_bright = {}


def _bright_oracle(family):
    """the hot-pattern case of tests/test_gpu_bright_tiles.py with hot channels 0, 17, 300 and 493 and an S2 of 6000 electrons: the
    oracle's run, once per family (which kernel makes a tile is the device's business)"""
    if family not in _bright:
        from tests.test_gpu_bright_tiles import _pattern
        cfg = SC.config(family, s2_secondary_sc_gain=100.0, tile_local_min_photons=0, seed=56)
        res = Resource(cfg)
        p = _pattern(HOT)
        res.s2_pattern_map = (lambda pos, **kw: np.repeat(p[None, :], len(pos), axis=0))
        _bright[family] = oracle_on_instructions(cfg, [dict(type=2, time=MS, x=0, y=0, z=-8, amp=6000)], resource=res)
    return _bright[family]


@pytest.mark.parametrize('route', ['bright', 'photon_array', 'no_bins'])
@FAMILY
def test_bright_tiles(family, route, monkeypatch):
    """tiles above 2048 photons on channels 0, 17, 300 and 493: k_s2_bright (the row staged into LDS); with tile_local_bright off, and
    with WFS_BRIGHT_MAX_BINS=0, the same tiles through k_s2_tile_gen and k_pulse_dense"""
    r = _bright_oracle(family)
    cfg = dict(r['cfg'], tile_local_bright=route != 'photon_array')
    if route == 'no_bins':
        monkeypatch.setenv('WFS_BRIGHT_MAX_BINS', '0')
    eng, counts = _device_on_instructions(r, cfg)
    kt = eng.kernel_times()
    kind = eng.tile_kernels()
    assert np.all(kind[0, list(HOT)] == (3 if route == 'bright' else 2)) and (kind == 1).sum() >= 480, kind[0, list(HOT)]
    if route == 'bright':
        assert 'k_s2_bright' in kt and 'k_s2_tile' in kt and 'k_s2_tile_gen' not in kt and 'k_pulse_dense' not in kt, sorted(kt)
    else:
        assert 'k_s2_tile_gen' in kt and 'k_pulse_dense' in kt and 'k_s2_tile' in kt and 'k_s2_bright' not in kt, sorted(kt)
    m = _compare(family, cfg, r['orc'], r['o'], eng, counts, _call_sets(r['o'], r['s_ins'], cfg), must_hit=list(HOT))
    _log(f'bright tiles {route}', family, kt, m)


@FAMILY
def test_pmt_afterpulses(family):
    """PMT afterpulses on, an S1 and a tile-generated S2: the parents' gains come from their channel's row, the afterpulses' are G x the
    drawn amplitude and bypass the table -- both as the oracle has them, the afterpulse sets included"""
    ap = ap_tables_from_golden()
    cfg = SC.config(family, s2_secondary_sc_gain=100.0, tile_local_min_photons=0, seed=57, enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    r = oracle_on_instructions(cfg, [dict(type=1, time=MS, x=0, y=0, z=-30, amp=3000), dict(type=2, time=3 * MS, x=0, y=0, z=-8, amp=300)], ap=ap)
    eng, counts = _device_on_instructions(r)
    kt = eng.kernel_times()
    o = r['o']
    assert (o['call_kind'] == 3).sum() == 2 and 'k_s2_tile' in kt and 'k_photon_fill' in kt, sorted(kt)
    n_ap = sum(int(o['call_ph_off'][k + 1] - o['call_ph_off'][k]) for k in np.flatnonzero(o['call_kind'] == 3))
    assert n_ap > 100
    m = _compare(family, cfg, r['orc'], o, eng, counts, _call_sets(o, r['s_ins'], cfg))
    _log('PMT afterpulses', family, kt, m, f'; {n_ap} afterpulses')


def test_identical_columns_give_the_one_row_records():
    """494 identical columns (n_spe = 494, every kernel indexes by channel) and the one shared column (n_spe = 1): the same record
    bytes, photons and truth, on a batch that holds an S1 (block generator) and two tile-generated S2s"""
    charge, pdf = SC.charge_axis()
    one = SC.config('delta', s2_secondary_sc_gain=100.0, tile_local_min_photons=0, seed=58, photon_area_distribution=dict(charge=charge, pdf=pdf, n_channels=SC.N_TPC))
    many = dict(one, photon_area_distribution=dict(charge=charge, pdfs=np.repeat(pdf[None, :], SC.N_TPC, axis=0), n_channels=SC.N_TPC))
    assert table_of(one).shape[0] == 1 and table_of(many).shape[0] == SC.N_TPC
    rows = [dict(type=1, time=MS, x=0, y=0, z=-30, amp=3000), dict(type=2, time=3 * MS, x=0, y=0, z=-8, amp=300), dict(type=2, time=5 * MS, x=0, y=0, z=-8, amp=1)]
    out = []
    for cfg in (one, many):
        r = oracle_on_instructions(cfg, rows)
        eng, counts = _device_on_instructions(r)
        kt = eng.kernel_times()
        assert 'k_s2_tile' in kt and 'k_photon_fill' in kt
        ph = eng.photons()
        out.append((eng.records().tobytes(), ph['gain'].tobytes(), ph['t'].tobytes(), eng.truth()[0].tobytes(), eng.truth_per_pmt().tobytes()))
        assert out[-1][0] == r['orc'].pack_records().tobytes() and counts['n_records'] > 500
    assert out[0] == out[1]
