"""Bright tiles of tile-generated S2s -- more than 2048 photons on one (instruction, channel) -- made by k_s2_bright (wfs_tilegen.h):
photons and pulse in one workgroup of 1024 threads, the tile's whole H table in LDS, no photon array (MI355X only).

Every case is a handful of instructions with s2_secondary_sc_gain = 100 under a constant hit pattern whose one or two hot channels
steer the tile sizes, compared with the CPU oracle as tests/test_gpu_generation.py does: photons, digitise windows, record bytes, n_pe.
Which kernel made a tile is read back with Engine.tile_kernels() (0 none, 1 k_s2_tile, 2 generation only + pulse kernels,
3 k_s2_bright).  Photon q of a tile has the same Philox coordinates whichever kernel draws it, so the oracle is the comparand as it is.

Sizes at z = -8 cm (bundled config): the surviving electrons of an S2 arrive within ~4 us, the S2 delay table has 8192 cells, so the
H table of a tile spans ~1200 start bins (~100 KB with its margins) and fits; at z = -90 cm the electrons spread over ~12 us, ~2000
start bins, which does not fit the 128 KB the kernel may take: such tiles keep the photon-array route (class 2).
"""
import numpy as np
import pytest

from tests.helpers import ap_tables_from_golden, make_engine, make_oracle
from tests.test_gpu_generation import MS, _assert_truth_rows, _compare, _instructions
from wfsim_amd import tables as T
from wfsim_amd.config import N_ROWS, current_2_adc, xenonnt_test_config
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import schedule

pytestmark = pytest.mark.gpu
NCH = 494
BRIGHT = 2048          # TILE_MAX_PHOTONS
PASS = 8192            # photons a pass of k_s2_bright makes (1024 threads x 8)


def _pattern(hot):
    """a constant hit pattern: the channels of `hot` take the given shares of the light, the others share the rest"""
    p = np.full(NCH, (1.0 - sum(hot.values())) / (NCH - len(hot)))
    for ch, share in hot.items():
        p[ch] = share
    return p


def _run(cfg, rows, p, ap=None, oracle=True, profiling=False):
    cfg = dict(cfg)
    cfg.setdefault('tile_local_min_photons', 0)
    if ap is not None:
        cfg.update(enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    ins = _instructions(rows)
    res = Resource(cfg)
    res.s2_pattern_map = (lambda pos, **kw: np.repeat(p[None, :], len(pos), axis=0))      # a plain callable: host rows
    order, key, cluster = schedule(ins, cfg)
    s_ins, gid = ins[order], order.astype(np.uint32)
    ip = instruction_params(s_ins, cfg, res)
    orc = o = None
    if oracle:
        orc = make_oracle(cfg, ap, resource=res)
        orc.simulate(s_ins, gid, ip)
        o = orc.results()
    eng = make_engine(cfg, resource=res)
    if profiling:
        eng.set_profiling(True)
    eng.load_instructions(s_ins, gid, cluster, key, ip)
    counts = eng.run()
    return orc, o, eng, counts, s_ins


def _tile_photons(eng, n_ins):
    """photons per (instruction, channel) of the primary sets, from the device's photon arrays"""
    ph = eng.photons()
    return np.stack([np.bincount(ph['ch'][ph['set_off'][i]:ph['set_off'][i + 1]], minlength=NCH) for i in range(n_ins)])


def _expected_kinds(s_ins, n_tile):
    """every tile of an S2 above 2048 photons by k_s2_bright, the others with photons by k_s2_tile; S1s are not tile-generated"""
    kind = np.where(n_tile > BRIGHT, 3, np.where(n_tile > 0, 1, 0))
    kind[s_ins['type'] != 2] = 0
    return kind.astype(np.int8)


def _oracle_truth_per_pmt(cfg, o, call, ch):
    """pulse.py:229-271 for one channel of one Pulse call from the oracle's photons, in their order inside the channel (generation order)"""
    a, b = o['call_ph_off'][call], o['call_ph_off'][call + 1]
    sel = o['ph_ch'][a:b] == ch
    t, gain, dpe = o['ph_t'][a:b][sel], o['ph_gain'][a:b][sel], o['ph_dpe'][a:b][sel]
    cmax = T.pmt_current_templates(cfg).max(axis=1)
    thr = T.thresholds(cfg, N_ROWS)[0][ch]
    above = gain * cmax[t % 10] * current_2_adc(cfg) > thr
    n, n_dpe = len(t), int(dpe.sum())
    G = cfg['gains'][ch]
    return np.array([n, n + n_dpe, above.sum(), above.sum() + above[:n_dpe].sum(), gain.sum() / G, gain[above].sum() / G])


THREE_SIZES = [dict(type=2, time=MS, x=0, y=0, z=-8, amp=6000), dict(type=2, time=3 * MS, x=1, y=1, z=-20, amp=900),
               dict(type=1, time=5 * MS, x=0, y=0, z=-30, amp=2000)]
THREE_SIZES_PATTERN = {17: 0.05, 300: 0.01}          # the first S2 then holds tiles of ~22000, ~4400 and ~900 photons


def test_bright_tiles_take_the_fused_kernel(monkeypatch):
    """One S2 with tiles of three sizes, a small S2 and an S1: tile_kernels() says 3 for every tile above 2048 photons and 1 for the other
    tiles with photons; k_s2_bright ran, the generation-only kernel and the dense pulse kernel did not; device == oracle photon by photon,
    records byte for byte; truth rows equal in all 12 columns and the per-PMT truth of the hot channels in all 6 (n_pe_trigger counts
    the photons above threshold among the FIRST n_dpe of the tile in generation order, pulse.py:255: the kernel keeps the ballots of its
    passes and counts them once the tile's n_dpe is known).  Every launch checked on the spot."""
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0), seed=77)
    orc, o, eng, counts, s_ins = _run(cfg, THREE_SIZES, _pattern(THREE_SIZES_PATTERN), profiling=True)
    kt = eng.kernel_times()
    n_tile = _tile_photons(eng, len(s_ins))
    assert n_tile[0, 17] > 20000 and BRIGHT < n_tile[0, 300] < 10000 and np.median(n_tile[0]) < BRIGHT
    kind = eng.tile_kernels()
    assert kind.shape == (len(s_ins), NCH) and kind.dtype == np.int8
    assert np.array_equal(kind, _expected_kinds(s_ins, n_tile))
    assert (kind == 3).sum() == 3 and kind[0, 17] == kind[0, 300] == kind[1, 17] == 3 and (kind == 1).sum() > 900      # (the small S2 holds ~3300 photons on channel 17)
    assert kt['k_s2_bright'][1] == 1 and 'k_s2_tile' in kt and 'k_s2_tile_gen' not in kt and 'k_pulse_dense' not in kt, sorted(kt)
    _compare(orc, o, eng, counts, s_ins)
    _assert_truth_rows(eng, o, s_ins)
    per_pmt = eng.truth_per_pmt()
    for ch in (17, 300, 5):          # (channel 5: a tile of k_s2_tile next to them)
        ref = _oracle_truth_per_pmt(eng.config, o, 0, ch)
        assert ref[3] > ref[2] > 0
        assert np.allclose(per_pmt[0, ch], ref, rtol=1e-9), (ch, per_pmt[0, ch], ref)


def test_pass_boundaries():
    """A dozen S2s whose hot channel holds from just above 2048 photons to three passes of the workgroup (8192 photons each), with
    tiles ending right behind a pass boundary (16386 = 2 x 8192 + 2) and photon numbers that are no multiple of four (a Philox call makes
    four photons).  Seed and amplitudes were chosen on the CPU, from the oracle's counts."""
    amps = [57, 58, 60, 70, 110, 180, 221, 223, 300, 442, 445, 600]
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0), seed=94)
    rows = [dict(type=2, time=MS * (i + 1), x=0, y=0, z=-8, amp=a) for i, a in enumerate(amps)]
    orc, o, eng, counts, s_ins = _run(cfg, rows, _pattern({17: 0.5}))
    n_hot = np.array([np.sum(o['ph_ch'][o['call_ph_off'][k]:o['call_ph_off'][k + 1]] == 17) for k in range(len(amps))])
    assert np.any((n_hot > BRIGHT) & (n_hot < 2200)) and np.any(n_hot > 2 * PASS) and np.any((n_hot > BRIGHT) & (n_hot % 4 != 0)), n_hot
    assert np.any((n_hot > PASS) & (n_hot < PASS + 1024)) and np.any((n_hot > 2 * PASS) & (n_hot < 2 * PASS + 4)), n_hot
    kind = eng.tile_kernels()
    assert np.array_equal(kind, _expected_kinds(s_ins, _tile_photons(eng, len(s_ins))))
    assert (kind == 3).sum() == len(amps) and set(np.where(kind == 3)[1]) == {17}
    _compare(orc, o, eng, counts, s_ins)
    _assert_truth_rows(eng, o, s_ins)


def test_fallback_by_the_fit_rule(monkeypatch):
    """A shallow S2 (z = -8 cm: ~1200 start bins) and a deep one (z = -90 cm: the electron cloud is ~12 us wide, ~2000 start bins) side by
    side, the budget lowered to 1400 start bins (WFS_BRIGHT_MAX_BINS): the bright tiles of the shallow S2 take k_s2_bright, those of the
    deep one the generation-only kernel and the dense pulse kernel, in the same batch; == oracle.  With the knob at its minimum every
    bright tile takes the photon-array route, and the records are the same bytes."""
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0), seed=12)
    rows = [dict(type=2, time=MS, x=0, y=0, z=-8, amp=2000), dict(type=2, time=3 * MS, x=0, y=0, z=-90, amp=6000),
            dict(type=1, time=5 * MS, x=0, y=0, z=-30, amp=500)]
    p = _pattern({17: 0.05, 300: 0.04})
    monkeypatch.setenv('WFS_BRIGHT_MAX_BINS', '1400')
    orc, o, eng, counts, s_ins = _run(cfg, rows, p)
    n_tile = _tile_photons(eng, len(s_ins))
    kind = eng.tile_kernels()
    bright = n_tile > BRIGHT
    assert bright[0].sum() == 2 and bright[1].sum() == 2
    assert np.all(kind[0][bright[0]] == 3) and np.all(kind[1][bright[1]] == 2), (kind[0][bright[0]], kind[1][bright[1]])
    assert np.all(kind[~bright & (n_tile > 0) & (s_ins['type'] == 2)[:, None]] == 1)
    _compare(orc, o, eng, counts, s_ins)
    _assert_truth_rows(eng, o, s_ins)
    first = eng.records().tobytes()
    monkeypatch.setenv('WFS_BRIGHT_MAX_BINS', '0')
    _, _, eng0, _, _ = _run(cfg, rows, p, oracle=False)
    kind0 = eng0.tile_kernels()
    assert not (kind0 == 3).any() and np.all(kind0[bright] == 2)
    assert eng0.records().tobytes() == first


def test_bright_tiles_sharing_a_row():
    """Two bright S2s 3 us apart on the same hot channel and an S1 inside their window: one digitise window, the rows of the hot channel
    collect several pulses, so the tiles of k_s2_bright are added into the row's accumulators (k_tile_add) instead of being read in place"""
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0), seed=5)
    rows = [dict(type=2, time=MS, x=0, y=0, z=-8, amp=500), dict(type=2, time=MS + 3000, x=0, y=0, z=-8, amp=700),
            dict(type=1, time=MS + 63_000, x=0, y=0, z=-30, amp=3000)]          # (the electrons of z = -8 cm arrive 60 .. 67 us after the interaction)
    orc, o, eng, counts, s_ins = _run(cfg, rows, _pattern({17: 0.1}), profiling=True)
    assert len(o['dg_left']) == 1
    kind = eng.tile_kernels()
    assert (kind == 3).sum() == 2 and np.all(kind[s_ins['type'] == 2, 17] == 3)
    kt = eng.kernel_times()
    assert 'k_tile_add' in kt and 'k_s2_bright' in kt and 'k_s2_tile_gen' not in kt, sorted(kt)
    _compare(orc, o, eng, counts, s_ins)
    _assert_truth_rows(eng, o, s_ins)


# (the cases of the default route keep the ids they had before the second parameter)
@pytest.mark.parametrize('scale,tile_local_bright', [pytest.param(1.0, True, id='1.0'), pytest.param(4.0, True, id='4.0'),
                                                     pytest.param(1.0, False, id='1.0-photon_array'), pytest.param(4.0, False, id='4.0-photon_array')])
def test_pmt_afterpulses_of_bright_tiles(scale, tile_local_bright):
    """PMT afterpulses on: every photon of a bright tile is screened inside its pass and the candidates leave as one key-ordered
    stretch per tile (k_ap_seg places the afterpulse tile in generation order).  The hot tile of ~22000 photons has more candidates
    than the workgroup's stage holds (AP_STAGE = 128) -- with the afterpulse probabilities x 4 so has the one of ~4400 --: the excess
    takes the overflow path.  Device == oracle photon by photon, the afterpulse sets included.  tile_local_bright = False: the same
    tiles through the generation-only kernel (k_s2_tile_gen, passes of 2048 photons, 256 threads), which screens and flushes with the
    same steps."""
    ap = ap_tables_from_golden()
    for name in ap:
        ap[name] = dict(ap[name], delaytime_cdf=ap[name]['delaytime_cdf'] * scale)
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0, tile_local_bright=tile_local_bright), seed=78)
    orc, o, eng, counts, s_ins = _run(cfg, THREE_SIZES, _pattern(THREE_SIZES_PATTERN), ap=ap)
    kind = eng.tile_kernels()
    assert kind.shape == (len(s_ins), NCH)
    if tile_local_bright:
        assert (kind == 3).sum() == 3 and not (kind == 2).any()
    else:
        assert (kind == 2).sum() == 3 and not (kind == 3).any()
    ph = eng.photons()
    n = len(s_ins)
    big = int(np.argmax(np.diff(ph['set_off'])[:n]))
    ap_hot = int(np.sum(ph['ch'][ph['set_off'][n + big]:ph['set_off'][n + big + 1]] == 17))
    assert ap_hot > 128, ap_hot          # (afterpulses of the hot tile alone: more than the stage holds)
    _compare(orc, o, eng, counts, s_ins)
    _assert_truth_rows(eng, o, s_ins)


@pytest.mark.parametrize('fma', [True, False])
def test_both_arithmetic_forms(fma):
    """fused_multiply_add on (one rounding per template * gain term) and off (numpy's two): the gather of k_s2_bright from its persistent
    table gives the record bytes of the oracle in the same mode"""
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0, fused_multiply_add=fma), seed=79)
    rows = [dict(type=2, time=MS, x=0, y=0, z=-8, amp=1500), dict(type=1, time=3 * MS, x=0, y=0, z=-30, amp=500)]
    orc, o, eng, counts, s_ins = _run(cfg, rows, _pattern({17: 0.2, 300: 0.03}))
    assert (eng.tile_kernels() == 3).sum() == 2
    _compare(orc, o, eng, counts, s_ins)


def test_switch_selects_the_photon_array_route():
    """config tile_local_bright = False: no tile takes k_s2_bright, the records are the bytes of the default run"""
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0), seed=80)
    rows = [dict(type=2, time=MS, x=0, y=0, z=-8, amp=1500), dict(type=2, time=3 * MS, x=3, y=0, z=-12, amp=300)]
    p = _pattern({17: 0.2, 300: 0.03})
    _, _, eng_on, _, s_ins = _run(cfg, rows, p, oracle=False)
    _, _, eng_off, _, _ = _run(dict(cfg, tile_local_bright=False), rows, p, oracle=False, profiling=True)
    k_on, k_off = eng_on.tile_kernels(), eng_off.tile_kernels()
    assert (k_on == 3).sum() == 3 and not (k_off == 3).any()          # (channels 17 and 300 of the first S2, channel 17 of the second)
    assert np.array_equal(k_off, np.where(k_on == 3, 2, k_on))
    kt = eng_off.kernel_times()
    assert 'k_s2_tile_gen' in kt and 'k_s2_bright' not in kt
    assert eng_off.records().tobytes() == eng_on.records().tobytes()
    assert np.array_equal(eng_off.truth()[0][:, :4], eng_on.truth()[0][:, :4])


def test_per_instruction_model_tables():
    """s2_luminescence_model = 'garfield': every instruction draws its delays from the table of its own position and PMT array
    (FTile.tab, not the default S2 table); a hot channel in the top and one in the bottom array"""
    from tests.helpers import golden
    from tests.test_delay_models_cpu import model_resources
    cfg = dict(xenonnt_test_config(s2_secondary_sc_gain=100.0, s2_luminescence_model='garfield', s2_time_model='zero_delay',
                                   **model_resources(golden('dists_models.npz'))), seed=81)
    rows = [dict(type=2, time=MS, x=3, y=-2, z=-8, amp=1500), dict(type=2, time=3 * MS, x=-20, y=11, z=-6, amp=1200),
            dict(type=1, time=5 * MS, x=0, y=0, z=-30, amp=500)]
    orc, o, eng, counts, s_ins = _run(cfg, rows, _pattern({17: 0.2, 300: 0.1}))
    assert eng.models.active
    kind = eng.tile_kernels()
    assert (kind == 3).sum() == 4 and np.all(kind[s_ins['type'] == 2][:, [17, 300]] == 3)
    _compare(orc, o, eng, counts, s_ins)
    _assert_truth_rows(eng, o, s_ins)
