"""Random instruction mixes under PEAKED hit patterns: the case generator behind tests/test_hot_patterns_cpu.py and
tests/test_gpu_hot_patterns.py, the photons per tile of an oracle run, and the seams of the bright-tile code a case reaches.

The random cases of the other files draw under the flat DummyMap pattern, where no tile passes TILE_MAX_PHOTONS = 2048.  Here the
pattern is position dependent, so one case holds tiles from nothing to several 10^4 photons: k_s2_bright and its passes, k_s2_tile_gen,
the fit rule, k_tile_add of a bright tile into a shared row, the dense pulse kernel and the large order classes behind the block
generator, the afterpulse overflow of a bright tile -- next to the switches the random files vary (run sets, resident rows, noise, HE
rows and the sum row).

A TILE is the photons of one Pulse call on one channel.  A BRIGHT tile is a tile of more than 2048 photons of a tile-generated S2 (an
S2 that is alone in its Pulse call and passes fuse_eligible, wfs_tilegen.h / oracle/wfsim_oracle.c): the tiles k_tile_counts hands to
k_s2_bright or, when the H table does not fit, to k_s2_tile_gen.  Everything here is computed on the CPU, from the oracle alone.
"""
import os

import numpy as np

from tests.helpers import ap_tables_from_golden, golden, make_oracle
from wfsim_amd import workloads as W
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype
from wfsim_amd.physics import instruction_params
from wfsim_amd.resource import Resource
from wfsim_amd.scheduler import run_sets, schedule

NCH, N_TOP = W.N_TPC, W.N_TOP
BRIGHT = 2048          # TILE_MAX_PHOTONS: photons a workgroup of k_s2_tile keeps; a pass of k_s2_tile_gen
PASS = 8192            # photons a pass of k_s2_bright makes (wfs_tilegen.h BRIGHT_PASS)
AP_BIG = 4096          # a tile whose afterpulse candidates pass the workgroup's stage; TILE_ORDER_MAX of the order classes
SHALLOW_CM, DEEP_CM = 15.0, 70.0

SEEDBASE = 8200
BASE = xenonnt_test_config()
N_SEEDS = int(os.environ.get('WFS_RANDOM_HOT', 24))
MAX_PHOTONS, MAX_PHOTONS_AP4 = 1.3e6, 8.0e5          # expected photons of a case (afterpulse arrays hold P / 8 + 65536 candidates)

# the seeds of the tests that run a case several times (tests/test_hot_patterns_cpu.py checks what they are chosen for)
KNOB_SEEDS = [3, 4, 8, 13, 14, 17]             # bright tiles, shallow and deep ones in one case
BATCH_SEEDS = [0, 4, 6, 8, 14, 16, 20, 22]     # the map in the config
SHARD_SEEDS = [4, 12, 16, 22]
EAP_SEEDS = [4, 8, 16, 18]
CARRY_SEEDS = [4, 8, 16]                       # of BATCH_SEEDS: a bright S2 in a window that is still open where a batch of several windows ends
CARRY_DESIGNED = [8, 16]                       # (4 as drawn; 8 and 16 with the four instructions of `batch_case` behind the drawn ones)

# the rows of the coverage table and how many of the default seeds must reach each
COVERAGE = {
    'tile_2048_8192': 6, 'tile_above_8192': 4, 'tile_above_16384': 4, 'tile_behind_pass_boundary': 2, 'tile_not_multiple_of_4': 4,
    'ap_tile_generated_s2_4096': 3, 'ap_s1_4096': 3, 'ap_shared_call_s2_4096': 3,
    'bright_deep': 3, 'bright_shallow': 3, 'bright_shallow_and_deep': 2, 'bright_shared_row': 4, 'bright_bottom_with_sum_row': 2,
    'bright_noise': 2, 'bright_row_resident': 2, 'bright_row_not_resident': 2, 'bright_fma': 2, 'bright_no_fma': 2,
    'no_tile_above_2048': 3,
}


# ---------------------------------------------------------------------------------------------------------------- the cases
def _hot_rows(rng, ins, bottom):
    """one pattern row per instruction: one or two hot channels with shares 0.002 .. 0.5 (log-uniform), the others share the rest;
    the first hot channel in the top array or (bottom: the sum row is on) in the bottom array"""
    p = np.zeros((len(ins), NCH))
    for i in range(len(ins)):
        hot = {int(rng.integers(N_TOP, NCH) if bottom and rng.random() < 0.8 else rng.integers(0, N_TOP)): float(np.exp(rng.uniform(np.log(0.002), np.log(0.5))))}
        if rng.random() < 0.4:
            c2 = int(rng.integers(0, NCH))
            if c2 not in hot:
                hot[c2] = float(np.exp(rng.uniform(np.log(0.002), np.log(0.2))))
        p[i] = (1.0 - sum(hot.values())) / (NCH - len(hot))
        for c, share in hot.items():
            p[i, c] = share
    return p


# A quarter of the table's rows are conjunctions of two or three independent draws (afterpulses AND run sets AND a large S2 pair ...) that
# 24 free cases reach once or twice.  So 14 of every 24 seeds have a THEME: one or two switches and one or two instructions are set,
# everything else stays drawn.  Even seeds (the map on the device) and odd seeds (host rows) keep their themes apart.
#   shared_ap   run sets and PMT afterpulses on, instructions 0 / 1 a pair of large S2s 1 mm apart: they share a Pulse call
#   dim         secondary gain 1.5 or 4 and no S2 above 2500 electrons: nothing above 2048 photons, the ordinary path
#   s1_ap       PMT afterpulses on, instruction 0 an S1 of 1.5 x 10^6 quanta with 5 .. 50 % of its light on one channel
#   bottom_sum  HE rows and the sum row on, instruction 0 a tile-generated S2 of 9000 electrons with 5 .. 30 % of its light on a bottom channel
THEMES = {0: 'shared_ap', 6: 'shared_ap', 12: 'shared_ap', 18: 'shared_ap', 2: 'dim', 10: 'dim', 20: 'dim',
          1: 's1_ap', 7: 's1_ap', 13: 's1_ap', 19: 's1_ap', 3: 'bottom_sum', 11: 'bottom_sum', 17: 'bottom_sum'}


def hot_case(seed):
    """(config, instructions, PMT afterpulse tables or None, noise or None, knobs), deterministic in `seed`.

    knobs: the environment of the engine, {'WFS_BRIGHT_MAX_BINS': '1400' | '0'} or {} (read when the engine is made).
    Pattern: even seeds carry workloads.synthetic_s2_pattern_map(n_grid=31) in the config (evaluated on the device); odd seeds carry
    config['hot_rows'] = dict(xy, p): one row per instruction for a host callable on the Resource (`resource_of`), S1s included."""
    rng = np.random.default_rng(SEEDBASE + seed)
    on_device = seed % 2 == 0
    theme = THEMES.get(seed % 24)
    kw = dict(s2_secondary_sc_gain=float(rng.choice([1.5, 4.0, 21.3, 100.0], p=[.05, .05, .3, .6])), seed=int(rng.integers(1, 10 ** 6)))
    kw['fused_multiply_add'] = bool(rng.random() < 0.5)
    kw['tile_local_bright'] = bool(rng.random() < 0.8)
    kw['tile_local_generation'] = bool(rng.random() < 0.9) or theme == 'bottom_sum'
    kw['tile_local_min_photons'] = int(rng.choice([0, 0, 64]))
    u = rng.random()
    if u < 0.6:                                                  # resident rows forced on / off, else the batch decides
        kw['row_resident'] = bool(u < 0.3)
    if rng.random() < 0.4 or theme == 'shared_ap':
        kw['save_full_truth'] = False                            # run sets: S1s / S2s close in time share a Pulse call
    ap, scale = None, float(rng.choice([1.0, 4.0]))
    if rng.random() < 0.35 or theme in ('shared_ap', 's1_ap'):
        ap = ap_tables_from_golden()
        for name in ap:
            ap[name] = dict(ap[name], delaytime_cdf=ap[name]['delaytime_cdf'] * scale)
        kw.update(enable_pmt_afterpulses=True, uniform_to_pmt_ap=ap)
    sum_row = bool(rng.random() < 0.3) or theme == 'bottom_sum'
    if sum_row:
        kw.update(high_energy_deamplification_factor=20, emit_sum_signal=True)
    noise = None
    if rng.random() < 0.3:
        noise = golden('noise.npz')['noise']
        if sum_row and rng.random() < 0.5:                       # with a column for the sum channel
            noise = np.concatenate([noise, rng.integers(-9, 10, size=(len(noise), 801 - noise.shape[1])).astype(np.int16)], axis=1)
        kw.update(enable_noise=True, noise_data=noise)
    knobs = {}
    u = rng.random()
    if u < 0.45:
        knobs['WFS_BRIGHT_MAX_BINS'] = '1400' if u < 0.3 else '0'
    if theme == 'dim':
        kw['s2_secondary_sc_gain'] = float(rng.choice([1.5, 4.0]))
    # ---- instructions: the time steps and amplitudes of test_gpu_random_mixes._random_case, amplitudes extended
    n = int(rng.integers(3, 26))
    ins = np.zeros(n, dtype=instruction_dtype)
    ins['type'] = rng.choice([1, 2], n, p=[0.4, 0.6])
    ins['time'] = np.cumsum(rng.choice([200, 3_000, 40_000, 500_000, 3_000_000], n)).astype(np.int64) + 1_000_000
    r, phi = 45 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    ins['x'], ins['y'] = r * np.cos(phi), r * np.sin(phi)
    depth = rng.choice(3, n, p=[0.3, 0.4, 0.3])                  # shallow (the bright tiles fit), anywhere, deep (they do not)
    ins['z'] = -np.where(depth == 0, rng.uniform(0.5, SHALLOW_CM, n), np.where(depth == 1, rng.uniform(0.5, 95, n), rng.uniform(DEEP_CM, 95, n)))
    s1 = ins['type'] == 1
    ins['amp'] = np.where(s1, rng.choice([0, 1, 40, 700, 5000, 30000, 400_000, 1_500_000], n, p=[.1, .1, .12, .14, .14, .1, .2, .1]),
                          rng.choice([0, 1, 7, 60, 400, 2500, 9000], n, p=[.06, .08, .1, .14, .2, .2, .22]))
    twin = rng.random(n) < 0.25                                  # a companion 1 mm / a few 100 ns behind its predecessor: shared Pulse calls, shared rows
    follow, gap = rng.random(n) < 0.15, rng.integers(500, 3000, n)          # a follower: its key lies just beyond right_raw_extension behind its predecessor's,
    fixed = []                                                   # instructions a theme sets: the photon cap below leaves them alone
    if theme == 'shared_ap':
        ins['type'][:2], ins['amp'][:2], twin[1], fixed = 2, [9000, 2500], True, [0, 1]
    elif theme == 's1_ap':
        ins['type'][0], ins['amp'][0], twin[1], fixed = 1, 1_500_000, False, [0]
    elif theme == 'bottom_sum':
        ins['type'][0], ins['amp'][0], twin[1], fixed = 2, 9000, False, [0]
        kw['s2_secondary_sc_gain'] = 100.0
    for i in range(1, n):
        if twin[i]:
            for f in ('type', 'x', 'y'):
                ins[f][i] = ins[f][i - 1]
            ins['z'][i] = min(ins['z'][i - 1] + float(rng.uniform(-0.1, 0.1)), -0.5)
            ins['time'][i] = ins['time'][i - 1] + int(rng.choice([50, 200, 600]))
            if i not in fixed:
                ins['amp'][i] = rng.choice([400_000, 30000, 700] if ins['type'][i] == 1 else [9000, 2500, 400])
    v, rext = float(BASE['drift_velocity_liquid']), int(BASE['right_raw_extension'])      # so it is another cluster inside the predecessor's digitise window
    for i in range(1, n):
        if follow[i] and not twin[i]:
            key = [int(ins['time'][k]) + (int(-ins['z'][k] / v) if ins['type'][k] == 2 else 0) for k in (i - 1, i)]
            ins['time'][i] += key[0] + rext + int(gap[i]) - key[1]
    if theme == 'dim':
        ins['amp'][(ins['type'] == 2) & (ins['amp'] > 2500)] = 2500
    # the case stays small: the largest amplitudes step down until the expected photons fit (S1: 0.1 photons per quantum)
    cap = MAX_PHOTONS_AP4 if (ap is not None and scale == 4.0) else MAX_PHOTONS
    w = np.where(ins['type'] == 1, 0.1, 0.8 * kw['s2_secondary_sc_gain'])
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    ladder = {1: [1_500_000, 400_000, 30000, 5000], 2: [9000, 2500, 400]}
    while float(np.sum(ins['amp'] * w)) > cap:
        can = free & np.array([int(a) in ladder[int(t)][:-1] for a, t in zip(ins['amp'], ins['type'])])
        if not can.any():
            break
        i = int(np.argmax(ins['amp'] * w * can))
        steps = ladder[int(ins['type'][i])]
        ins['amp'][i] = steps[steps.index(int(ins['amp'][i])) + 1]
    ins['recoil'], ins['event_number'] = 7, np.arange(n)
    if on_device:
        kw['s2_pattern_map'] = W.synthetic_s2_pattern_map(n_grid=31)
    else:
        p = _hot_rows(rng, ins, sum_row)
        if theme in ('s1_ap', 'bottom_sum'):                     # the themed instruction's hot channel and share
            c = int(rng.integers(N_TOP, NCH)) if theme == 'bottom_sum' else int(rng.integers(0, NCH))
            share = float(np.exp(rng.uniform(np.log(0.05), np.log(0.3 if theme == 'bottom_sum' else 0.5))))
            p[0], p[0, c] = (1.0 - share) / (NCH - 1), share
        kw['hot_rows'] = dict(xy=np.array([ins['x'], ins['y']], dtype=np.float64).T, p=p)
    for i, amp in DESIGNED.get(seed, []):                        # (designed amplitudes: chosen from the oracle's counts, see DESIGNED)
        ins['amp'][i] = amp
    return xenonnt_test_config(**kw), ins, ap, noise, knobs


# Amplitudes chosen on the CPU from the oracle's counts, as tests/test_gpu_bright_tiles.py::test_pass_boundaries chose its own: with them
# instruction `index` of case `seed` holds a bright tile that ends within 4 photons behind a multiple of 2048 (a pass of k_s2_tile_gen)
# or of 8192 (a pass of k_s2_bright).  {seed: [(index, amplitude)]}
DESIGNED = {4: [(13, 8954)], 14: [(7, 8856)], 22: [(4, 8879)]}          # tiles of 2052, 2052 and 8195 photons


def batch_case(seed):
    """hot_case(seed) for the batch-cut test.  A window is carried across a cut when a batch of several windows ends inside it: a closed
    window, then a bright S2 whose window is still open where the batch ends because another cluster follows within
    right_raw_extension of its last pulse.  Among 54 drawn cases one holds that (seed 4), so the seeds of CARRY_DESIGNED get it behind their
    drawn instructions: a small S1 (its own window); 1 ms later a cluster of a tiny S1 and, 50 us behind it, an S2 of 9000 electrons
    at z = -5 cm (the batch bound is passed with the S2 for every max_batch_quanta the test uses, and a batch never ends inside a
    cluster -- RawData._batch_end -- so the batch ends behind the S2); and a small S1 whose key lies right_raw_extension + 2 us behind
    the S2's key -- a cluster of its own, inside the S2's window (the S2's photons arrive for longer than 2 us)."""
    cfg, ins, ap, noise, knobs = hot_case(seed)
    if seed not in CARRY_DESIGNED:
        return cfg, ins, ap, noise, knobs
    v, rext = float(cfg['drift_velocity_liquid']), int(cfg['right_raw_extension'])
    t0 = int(ins['time'].max()) + 5_000_000
    more = np.zeros(4, dtype=instruction_dtype)
    more['type'], more['amp'], more['z'] = [1, 1, 2, 1], [700, 40, 9000, 700], [-20.0, -20.0, -5.0, -20.0]
    more['x'], more['y'] = [0.0, 0.0, 10.0, 0.0], [0.0, 0.0, -5.0, 0.0]
    key_s2 = t0 + 1_000_000 + int(5.0 / v)
    more['time'] = [t0, key_s2 - 50_000, t0 + 1_000_000, key_s2 + rext + 2000]
    more['recoil'], more['event_number'] = 7, len(ins) + np.arange(4)
    return cfg, np.concatenate([ins, more]), ap, noise, knobs


def resource_of(cfg):
    """the Resource of a case: config['hot_rows'] becomes a host callable for both pattern maps (the row of the nearest listed position)"""
    res = Resource(cfg)
    hot = cfg.get('hot_rows')
    if hot is not None:
        xy, p = hot['xy'], hot['p']

        def pattern(pos, **kw):
            pos = np.asarray(pos, dtype=np.float64)[:, :2]
            return p[np.argmin(np.sum((pos[:, None, :] - xy[None, :, :]) ** 2, axis=2), axis=1)]
        res.s1_pattern_map = res.s2_pattern_map = pattern
    return res


def scheduled(cfg, ins, res, device_maps=()):
    """dict: the sorted instructions, their run-wide ids, clusters, keys, instruction parameters, the Pulse call of every instruction
    numbered in processing order (`call`: the oracle's primary calls in their order) and what Engine.load_instructions takes as run_set"""
    order, key, cluster = schedule(ins, cfg)
    s_ins = ins[order]
    call, n_calls = run_sets(s_ins, key, cluster, cfg)
    return dict(s_ins=s_ins, gid=order.astype(np.uint32), cluster=cluster, key=key, ip=instruction_params(s_ins, cfg, res, device_maps=device_maps),
                call=call, n_calls=n_calls, run_set=None if cfg.get('save_full_truth', True) else call)


def run_oracle(cfg, ap, res, s):
    orc = make_oracle(cfg, ap, resource=res)
    orc.simulate(s['s_ins'], s['gid'], s['ip'])
    return orc, orc.results()


def tile_generated(cfg, s):
    """bool per sorted instruction: the rule of fuse_eligible (wfs_tilegen.h, oracle/wfsim_oracle.c) and k_fuse_decide on the rows of s['ip']"""
    p = kernel_params(cfg)
    s_ins, ip = s['s_ins'], s['ip']
    if not p['tile_gen'] or p['gain_spread'] != 0.0:
        return np.zeros(len(s_ins), dtype=bool)
    alone = np.bincount(s['call'], minlength=s['n_calls'])[s['call']] == 1
    row = ip['cdf_table'][ip['cdf_row']]
    pmax = np.max(np.diff(row, axis=1, prepend=0.0), axis=1)
    lam = s_ins['amp'].astype(np.float64) * ip['sc_gain'] * pmax
    return alone & (s_ins['type'] == 2) & (s_ins['amp'] > 0) & (ip['sc_gain'] > 0) & (lam >= float(p['tile_gen_min'])) & (lam < 1.0e9)


def tile_sizes(o):
    """photons per (Pulse call, channel) of Oracle.results(): int64 [calls][channel], PMT-afterpulse calls (call_kind 3) included"""
    off = o['call_ph_off']
    return np.stack([np.bincount(o['ph_ch'][a:b], minlength=NCH) for a, b in zip(off[:-1], off[1:])]) if len(off) > 1 else np.zeros((0, NCH), np.int64)


def primary_calls(o):
    """index among the oracle's calls of every primary Pulse call, in processing order"""
    return np.flatnonzero(o['call_kind'] != 3)


def bright_tiles(cfg, s, o):
    """(bool [primary call][channel]: bright tiles, bool [primary call]: the call is a tile-generated S2, [primary call] -> instruction)"""
    n = tile_sizes(o)[primary_calls(o)]
    first = np.array([np.flatnonzero(s['call'] == q)[0] for q in range(s['n_calls'])], dtype=np.int64)
    tg = tile_generated(cfg, s)[first] if len(first) else np.zeros(0, bool)
    return (n > BRIGHT) & tg[:, None], tg, first


def seams(cfg, ins, o):
    """the rows of COVERAGE this case reaches, from the oracle's results alone (o: Oracle.results() of the case on its host rows)"""
    s = scheduled(cfg, ins, resource_of(cfg))
    sizes = tile_sizes(o)
    prim = primary_calls(o)
    n = sizes[prim]
    bright, tg, first = bright_tiles(cfg, s, o)
    kind = o['call_kind'][prim]
    members = np.bincount(s['call'], minlength=s['n_calls'])
    out = set()
    nb = n[bright]
    if np.any(nb <= PASS): out.add('tile_2048_8192')
    if np.any(nb > PASS): out.add('tile_above_8192')
    if np.any(nb > 2 * PASS): out.add('tile_above_16384')
    if np.any(((nb % PASS >= 1) & (nb % PASS <= 4)) | ((nb % BRIGHT >= 1) & (nb % BRIGHT <= 4))): out.add('tile_behind_pass_boundary')
    if np.any(nb % 4 != 0): out.add('tile_not_multiple_of_4')
    if kernel_params(cfg)['enable_pmt_ap']:
        big = (n > AP_BIG).any(axis=1)
        if np.any(big & tg): out.add('ap_tile_generated_s2_4096')
        if np.any(big & (kind == 1)): out.add('ap_s1_4096')
        if np.any(big & (kind == 2) & (members > 1)): out.add('ap_shared_call_s2_4096')
    has = bright.any(axis=1)
    z = np.abs(s['s_ins']['z'][first]) if len(first) else np.zeros(0)
    if np.any(has & (z > DEEP_CM)): out.add('bright_deep')
    if np.any(has & (z < SHALLOW_CM)): out.add('bright_shallow')
    if np.any(has & (z > DEEP_CM)) and np.any(has & (z < SHALLOW_CM)): out.add('bright_shallow_and_deep')
    if has.any():
        if shared_row_windows(o, bright): out.add('bright_shared_row')
        if cfg.get('emit_sum_signal', False) and bright[:, N_TOP:].any(): out.add('bright_bottom_with_sum_row')
        if kernel_params(cfg)['enable_noise']: out.add('bright_noise')
        if cfg.get('row_resident', 'auto') is True: out.add('bright_row_resident')
        if cfg.get('row_resident', 'auto') is False: out.add('bright_row_not_resident')
        out.add('bright_fma' if cfg.get('fused_multiply_add', True) else 'bright_no_fma')
    if not np.any(n > BRIGHT): out.add('no_tile_above_2048')
    return out


def pulse_calls(o):
    """the oracle's call of every pulse: a call makes one pulse per channel it has photons on, in channel order"""
    per_call = (tile_sizes(o) > 0).sum(axis=1)
    assert per_call.sum() == len(o['pl_ch'])
    return np.repeat(np.arange(len(per_call)), per_call)


def shared_row_windows(o, bright):
    """digitise windows in which a bright tile shares its channel with another pulse (its row collects several pulses: k_tile_add)"""
    call_of = pulse_calls(o)
    q_of = np.cumsum(o['call_kind'] != 3) - 1                   # call -> primary call
    out = []
    for w in range(len(o['dg_left'])):
        a, b = int(o['dg_first_pulse'][w]), int(o['dg_first_pulse'][w] + o['dg_n_pulses'][w])
        ch = o['pl_ch'][a:b]
        several = np.bincount(ch, minlength=NCH)[ch] > 1
        is_bright = (o['call_kind'][call_of[a:b]] != 3) & bright[q_of[call_of[a:b]], ch]
        if np.any(several & is_bright):
            out.append(w)
    return out


def bright_windows(o, bright):
    """digitise windows that hold a bright tile"""
    call_of = pulse_calls(o)
    q_of = np.cumsum(o['call_kind'] != 3) - 1
    is_bright = (o['call_kind'][call_of] != 3) & bright[q_of[call_of], o['pl_ch']]
    w_of = np.searchsorted(o['dg_first_pulse'], np.arange(len(call_of)), side='right') - 1
    return sorted(set(w_of[is_bright].tolist()))


def oracle_case(seed):
    """a case through the oracle on its host rows: (cfg, ins, ap, noise, knobs, scheduled, oracle, results)"""
    cfg, ins, ap, noise, knobs = hot_case(seed)
    res = resource_of(cfg)
    s = scheduled(cfg, ins, res)
    orc, o = run_oracle(cfg, ap, res, s)
    return cfg, ins, ap, noise, knobs, s, orc, o


def one_engine_sequence():
    """(config, afterpulse tables, knobs, [(name, instructions)]): six batches for ONE engine under the config of case 12 (gain 100, run sets,
    PMT afterpulses, WFS_BRIGHT_MAX_BINS = 1400: shallow bright tiles take k_s2_bright, deep ones k_s2_tile_gen).  Bright tiles; none
    above 2048 photons; bright tiles next to a shared Pulse call with a tile beyond TILE_ORDER_MAX (the huge order class); two
    single-quantum instructions; two instructions without a quantum (no photon at all); bright tiles again."""
    cfg, _, ap, _, knobs = hot_case(12)
    dim = hot_case(22)[1].copy()               # the batch before it once more, dimmed: its large S2s hold no electron (so they are not
    dim['amp'] = np.where((dim['type'] == 2) & (dim['amp'] >= 2500), 0, np.minimum(dim['amp'], 60))      # tile-generated any more), the others 60 quanta at most
    tiny = hot_case(22)[1][:2].copy()
    tiny['type'], tiny['amp'] = [1, 2], 1
    empty = tiny.copy()
    empty['amp'] = 0
    return cfg, ap, knobs, [('bright', hot_case(22)[1]), ('none', dim), ('bright_and_huge', hot_case(0)[1]), ('tiny', tiny), ('empty', empty),
                            ('bright_again', hot_case(6)[1])]
