"""Designed cases at the seams of the block photon generator's front end, and the seam table of every case computed on the CPU from
the oracle alone: the inputs of tests/test_block_seams_cpu.py (which seam each case reaches) and tests/test_gpu_block_seams.py (device
against oracle, every tile in the oracle's order).

The block rule restated here (wfs_kernels.h: k_block_emitters, k_block_ranges, generic_is_tail, k_tile_order_scan):
  * photons are numbered in generation order: the instructions as loaded, emitter by emitter; an S1 is one emitter (its hits), an S2
    `amp` emitters (its candidate electrons, the lost ones and the Poisson zeros included);
  * block b holds photons [2048 b, 2048 (b + 1)) (GEN_BLOCK);
  * a block is FAST iff its first and last photon belong to one instruction and e_hi - e_lo + 2 <= 512 (GEN_WIN; e_lo / e_hi: the
    emitters of its first / last photon), otherwise GENERIC;
  * an instruction is FULLSORT iff its Pulse call holds several instructions, or a generic block lies strictly inside it
    (ins_ph0[i] < p0 and ins_ph0[i + 1] > p1): its tiles are ordered as a whole;
  * otherwise its tile is [head | ranges of its fast blocks | tail]: the photons of a generic block are HEAD when the instruction begins
    in that block (ins_ph0[i] >= p0) and TAIL when it began before it.  Head and tail are ordered on their own, per channel.
    Consequences the table relies on: a head or a tail holds at most 2048 photons (it lies in one block), and a tail never comes
    without ranges (the block of an instruction's first photon is fast, or its photons there are head).
Photons per candidate emitter come from the oracle's `em_nph`; the channels of ONE instruction per case in generation order from
Oracle.sample_channels, whose stream is that of the instruction with run-wide id PROBE_GID.
"""
import numpy as np

from tests import hot_patterns as H
from tests.helpers import ap_tables_from_golden
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype

NCH = H.NCH
GEN_BLOCK, GEN_WIN = 2048, 512
ORDER_INLINE, ORDER_WAVE, ORDER_MAX = 12, 64, 4096          # TILE_ORDER_INLINE, a wave, TILE_ORDER_MAX
PROBE_GID = 777777                                          # the stream of Oracle.sample_channels
MS = 1_000_000
HOT = 17                                                    # the channel of the one-channel rows


# ---------------------------------------------------------------------------------------------------------------- the cases
def _ins(rows):
    ins = np.zeros(len(rows), dtype=instruction_dtype)
    for i, r in enumerate(rows):
        for k, v in r.items():
            if k in ins.dtype.names:
                ins[i][k] = v
        ins[i]['event_number'], ins[i]['recoil'] = i, 7
        if 'time' not in r:
            ins[i]['time'] = MS * (i + 1)          # 1 ms apart: loaded order = listed order, whatever the drift time
        if 'z' not in r:
            ins[i]['z'] = -5.0
        ins[i]['x'], ins[i]['y'] = 0.5 * (i % 40) - 10.0, 0.5 * (i // 40) - 10.0      # one position per instruction: one pattern row each
    return ins


def _case(rows, seed, block=True, ap=False, run_sets=False, flat=False, **kw):
    """rows: dicts of instruction fields plus, optionally, 'gain' / 'p' (ip['sc_gain'] / ip['p_hit'] of that instruction), 'row'
    ({channel: share}: a peaked pattern row, the other channels share the rest; {HOT: 1.0}: all light on one channel) and 'probe'."""
    ins = _ins(rows)
    p = np.full((len(rows), NCH), 1.0 / NCH)
    for i, r in enumerate(rows):
        hot = r.get('row')
        if hot:
            p[i] = (1.0 - sum(hot.values())) / max(NCH - len(hot), 1)
            for c, share in hot.items():
                p[i, c] = share
    cfg = dict(seed=seed, s2_secondary_sc_gain=20.0, tile_local_generation=not block)
    if not flat:
        cfg['hot_rows'] = dict(xy=np.array([ins['x'], ins['y']], dtype=np.float64).T, p=p)
    if run_sets:
        cfg['save_full_truth'] = False
    tables = None
    if ap:
        tables = ap_tables_from_golden()
        for name in tables:
            tables[name] = dict(tables[name], delaytime_cdf=tables[name]['delaytime_cdf'] * 4.0)
        cfg.update(enable_pmt_afterpulses=True, uniform_to_pmt_ap=tables)
    cfg.update(kw)
    over = [(i, f, r[k]) for i, r in enumerate(rows) for k, f in (('gain', 'sc_gain'), ('p', 'p_hit')) if k in r]
    probe = [i for i, r in enumerate(rows) if r.get('probe')]
    assert len(probe) <= 1
    return dict(cfg=xenonnt_test_config(**cfg), ins=ins, ap=tables, overrides=over, probe=probe[0] if probe else None, block=block)


def s1(amp, exact=True, **kw):
    """an S1; exact: p_hit = 1, so that its photons = amp"""
    return dict(dict(type=1, amp=amp, **({'p': 1.0} if exact else {})), **kw)


def s2(amp, gain=None, p=None, **kw):
    r = dict(type=2, amp=amp, **kw)
    if gain is not None: r['gain'] = gain
    if p is not None: r['p'] = p
    return r


ONE = {HOT: 1.0}


def _pairs(sizes, t0):
    """run sets of two exact one-channel S1s 40 ns apart, 1 ms between the sets: fullsort tiles of exactly a + b photons"""
    rows = []
    for q, (a, b) in enumerate(sizes):
        rows += [s1(a, row=ONE, time=t0 + MS * q), s1(b, row=ONE, time=t0 + MS * q + 40)]
    return rows


def cases():
    """{name: case}.  Seeds and the amplitudes marked 'found' were chosen on the CPU from the oracle's counts
    (tests/test_block_seams_cpu.py asserts what they were chosen for)."""
    c = {}
    c['single_photon'] = _case([s1(1)], seed=1)
    c['below_one_block'] = _case([s1(700), s2(20), s1(0), s2(30, gain=9.0)], seed=2)
    c['exact_blocks'] = _case([s1(2048), s1(4096)], seed=3)                       # 3 blocks, ranges only
    # R0 & 3: exact S1s put the first photon of the next instruction at every residue mod 4; S2s ride between them
    c['quad_phase'] = _case([s1(1), s1(5001), s1(5001), s1(5001), s1(5000), s2(300, p=1.0), s1(2), s2(300, p=1.0), s1(3), s2(300, p=1.0), s1(5000, exact=False)],
                            seed=4)
    # lost electrons (p = 0.3: runs of >= 8 photon-less emitters inside a window) and Poisson zeros (gain 5, every electron alive)
    c['window_zeros'] = _case([s1(100), s2(1500, gain=20.0, p=0.3), s2(1500, gain=5.0, p=1.0), s1(50)], seed=5)
    # gain 4: ~512 emitters per block -- fast and generic blocks side by side inside one instruction (fullsort), nwin 512 and 513
    c['window_limit'] = _case([s1(300), s2(20000, gain=4.0, p=1.0), s1(300)], seed=WINDOW_LIMIT_SEED)
    # >= 300 S2s of one electron: blocks of > 100 instructions, many instructions per 256-emitter block; photon-less ones between
    many = [s2(0)]
    for q in range(330):
        many.append(s2(1, gain=15.0, p=1.0))
        if q % 50 == 10: many.append(s2(0))
        if q % 50 == 20: many.append(s2(3, p=0.0))          # all electrons lost
        if q % 50 == 30: many.append(s1(0))
        if q % 50 == 40: many.append(s1(40, p=0.0))
    many += [s1(5, exact=False), s1(0)]
    c['many_instructions'] = _case(many, seed=7)
    # wide blocks (gain 1.5: ~1365 emitters per block): strictly inside (fullsort), at the first photon (head), at the last (tail)
    c['wide_inside'] = _case([s1(500), s2(6000, gain=1.5, p=1.0), s1(100)], seed=8)
    c['wide_at_first_photon'] = _case([s1(2048), s2(1800, gain=1.5, p=1.0)], seed=9)
    c['wide_at_last_photon'] = _case([s1(WIDE_LAST_PAD), s2(2500, gain=1.5, p=1.0)], seed=10)       # found: pad + photons of the S2 = 4096
    # tile layouts of single-instruction sets
    c['layouts'] = _case([s1(300), s2(500, p=0.9), s1(300), s1(2148), s1(50), s1(2000), s1(100), s1(60)], seed=11)
    # head / tail sizes, exact: one-channel S1s inside generic blocks (heads), behind a fast block (tails)
    heads = [s1(n, row=ONE) for n in (2, 12, 13, 64, 65, 700)]
    tails = []
    for n in (2, 12, 13, 64, 65, 1500):
        tails += [s1(4096 - sum(r['amp'] for r in heads + tails) % 2048 + n, row=ONE), s1(1, row=ONE)]
    c['head_tail_sizes'] = _case(heads + tails, seed=12)
    # fullsort tiles of exact sizes (run sets of two one-channel S1s), 4096 and 4097 on either side of TILE_ORDER_MAX
    c['fullsort_sizes'] = _case(_pairs([(1, 1), (5, 7), (6, 7), (30, 34), (30, 35), (1000, 2000), (2000, 2096), (2000, 2097), (9000, 3000)], MS),
                                seed=13, run_sets=True)
    # (block, channel) segments of a probed S1: eight channels at ~64.5 photons per block, one far above, the others 0 .. 12
    seg_row = {c_: 64.5 / 2048 for c_ in range(100, 108)}
    seg_row[HOT] = 0.4
    c['segments'] = _case([s1(300), s1(2048 * 40, row=seg_row, probe=True), s1(200)], seed=SEGMENT_SEED)
    # run sets: an S1 set and an S2 set of three, a photon-less middle instruction, a large and a small instruction
    t = 10 * MS
    c['run_sets'] = _case([s1(900, exact=False, time=MS), s1(700, exact=False, time=MS + 40), s1(500, exact=False, time=MS + 80),
                           s2(160, time=3 * MS), s2(140, time=3 * MS + 100), s2(130, time=3 * MS + 200),
                           s1(400, time=5 * MS), s1(0, time=5 * MS + 40), s1(300, time=5 * MS + 80),
                           s2(150, time=7 * MS), s2(40, p=0.0, time=7 * MS + 100), s2(120, time=7 * MS + 200),
                           s2(3000, time=t), s2(3, p=1.0, time=t + 100)], seed=14, run_sets=True)
    # emitter front end: S2s ending on multiples of 256 emitters, amp 0 first / middle / last, S1s behind the last S2, S1 quads
    c['emitter_front_end'] = _case([s2(0), s2(256), s2(512), s2(0), s2(7)] + [s1(a, exact=False) for a in (1, 3, 4, 5, 255, 256, 257, 1023)] + [s1(0)], seed=15)
    # PMT afterpulses: afterpulse tiles of one-channel S1 parents in every order class, the layouts case once more
    par = [s1(n, row=ONE) for n in [AP_SMALL] * 40 + [AP_MID] * 80 + [3000, 12000] + AP_BIG]
    c['ap_sizes'] = _case(par, seed=AP_SEED, ap=True)
    c['ap_layouts'] = _case([s1(300), s2(500, p=0.9), s1(300), s1(2148), s1(50), s2(700, gain=1.5, p=1.0), s1(60)], seed=17, ap=True)
    return c


# found on the CPU (tests/test_block_seams_cpu.py checks them)
WINDOW_LIMIT_SEED = 6
WIDE_LAST_PAD = 385
SEGMENT_SEED = 16
AP_SEED, AP_SMALL, AP_MID, AP_BIG = 20, 62, 322, [23500, 23800, 24100]


# ---------------------------------------------------------------------------------------------------------------- through the oracle
def prepared(case):
    """(config, resource, scheduled batch): the overrides of ip applied, the probe's run-wide id set; both sides receive this batch"""
    cfg = case['cfg']
    res = H.resource_of(cfg)
    s = H.scheduled(cfg, case['ins'], res)
    ev = s['s_ins']['event_number']
    ip = dict(s['ip'], sc_gain=np.array(s['ip']['sc_gain'], dtype=np.float64), p_hit=np.array(s['ip']['p_hit'], dtype=np.float64))
    for i, f, v in case['overrides']:
        ip[f][ev == i] = v
    gid = s['gid'].copy()
    if case['probe'] is not None:
        gid[ev == case['probe']] = PROBE_GID
    return cfg, res, dict(s, ip=ip, gid=gid)


def oracle_case(case):
    cfg, res, s = prepared(case)
    orc, o = H.run_oracle(cfg, case['ap'], res, s)
    return cfg, res, s, orc, o


def emitters(s_ins):
    """candidate emitters of every loaded instruction (S1: one, S2: amp) and their offsets"""
    n_em = np.where(s_ins['type'] == 1, 1, np.maximum(s_ins['amp'], 0)).astype(np.int64)
    return n_em, np.concatenate([[0], np.cumsum(n_em)])


def _longest_zero_run(x):
    best = run = 0
    for v in x:
        run = run + 1 if v == 0 else 0
        best = max(best, run)
    return best


def block_table(o, s_ins, cfg):
    """The block rule on the oracle's photons per emitter: dict of
    n_photons, n_blocks, ins_ph0 [n + 1], ins_nph [n], multi [n] (the Pulse call holds several instructions), fullsort [n],
    head / tail [n] (photons), n_fast [n] (fast blocks of the instruction), and per block: fast, e_lo, e_hi, nwin, ins_lo, ins_hi (the
    instructions of its first / last photon), r0 (fast: first photon of the block inside its instruction), zeros / zero_run (photon-less
    emitters inside [e_lo, e_hi] and the longest run of them)."""
    from wfsim_amd.scheduler import run_sets, schedule
    n = len(s_ins)
    n_em, em_off = emitters(s_ins)
    nph = np.asarray(o['em_nph'], dtype=np.int64)
    assert len(nph) == em_off[-1], (len(nph), em_off[-1])
    em_ins = np.repeat(np.arange(n), n_em)
    ph_off = np.concatenate([[0], np.cumsum(nph)])               # first photon of every emitter (+ the total)
    ins_ph0 = ph_off[em_off]
    P = int(ph_off[-1])
    nb = -(-P // GEN_BLOCK)
    order, key, cluster = schedule(s_ins, cfg)
    assert np.array_equal(order, np.arange(n))                   # (the instructions are given as loaded: sorted)
    call, n_calls = run_sets(s_ins, key, cluster, cfg)
    multi = np.bincount(call, minlength=n_calls)[call] > 1
    t = dict(n_photons=P, n_blocks=nb, ins_ph0=ins_ph0, ins_nph=np.diff(ins_ph0), multi=multi, call=call, em_off=em_off, nph=nph)
    blk = {k: np.zeros(nb, dtype=np.int64) for k in ('e_lo', 'e_hi', 'nwin', 'ins_lo', 'ins_hi', 'r0', 'zeros', 'zero_run', 'p0', 'p1')}
    fast = np.zeros(nb, dtype=bool)
    fullsort = multi.copy()
    head, tail, n_fast = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for b in range(nb):
        p0, p1 = b * GEN_BLOCK, min((b + 1) * GEN_BLOCK, P)
        e_lo = int(np.searchsorted(ph_off[:-1], p0, side='right')) - 1        # the last emitter that starts at or before the photon: the one that holds it
        e_hi = int(np.searchsorted(ph_off[:-1], p1 - 1, side='right')) - 1
        i0, i1 = int(em_ins[e_lo]), int(em_ins[e_hi])
        fast[b] = i0 == i1 and e_hi - e_lo + 2 <= GEN_WIN
        z = nph[e_lo:e_hi + 1] == 0
        for k, v in (('e_lo', e_lo), ('e_hi', e_hi), ('nwin', e_hi - e_lo + 2), ('ins_lo', i0), ('ins_hi', i1), ('r0', p0 - ins_ph0[i0]),
                     ('zeros', int(z.sum())), ('zero_run', _longest_zero_run(nph[e_lo:e_hi + 1]) if z.any() else 0), ('p0', p0), ('p1', p1)):
            blk[k][b] = v
        if fast[b]:
            n_fast[i0] += 1
            continue
        if i0 == i1 and ins_ph0[i0] < p0 and ins_ph0[i0 + 1] > p1:
            fullsort[i0] = True
        for i in range(i0, i1 + 1):                              # the instructions with photons in this generic block
            k = min(p1, ins_ph0[i + 1]) - max(p0, ins_ph0[i])
            if k > 0:
                if ins_ph0[i] >= p0: head[i] += k
                else: tail[i] += k
    t.update(blk, fast=fast, fullsort=fullsort, head=np.where(fullsort, 0, head), tail=np.where(fullsort, 0, tail), n_fast=n_fast)
    return t


def generation_channels(orc, s, t, i):
    """channels of the photons of loaded instruction i in generation order, or None: the probe's from Oracle.sample_channels, those of an
    instruction whose row puts all light on one channel from the row"""
    row = s['ip']['cdf_table'][s['ip']['cdf_row'][i]]
    n = int(t['ins_nph'][i])
    p = np.diff(row, prepend=0.0)
    if p.max() == 1.0:
        return np.full(n, int(np.argmax(p)), dtype=np.int64)
    if s['gid'][i] == PROBE_GID:
        return orc.sample_channels(row, n).astype(np.int64)
    return None


def ordered_sizes(orc, o, s, t):
    """sizes of what gets ordered, from the oracle: dict of int arrays
    head_tail: photons per channel of the heads and tails of the instructions whose channels are known (generation_channels);
    fullsort: the tiles of the primary calls whose instructions are fullsort; afterpulse: the tiles of the PMT-afterpulse calls;
    segment: photons per (fast block, channel) of the instructions whose channels are known, zeros included."""
    sizes = H.tile_sizes(o)
    prim = H.primary_calls(o)
    ht, seg = [], []
    for i in range(len(s['s_ins'])):
        if t['fullsort'][i] and not t['n_fast'][i]:
            continue
        ch = generation_channels(orc, s, t, i)
        if ch is None or not len(ch):
            continue
        assert np.array_equal(np.bincount(ch, minlength=NCH), sizes[prim[t['call'][i]]]) or t['multi'][i]      # the same photons as the call's
        if not t['fullsort'][i]:
            if t['head'][i]: ht.append(np.bincount(ch[:t['head'][i]], minlength=NCH))
            if t['tail'][i]: ht.append(np.bincount(ch[len(ch) - t['tail'][i]:], minlength=NCH))
        for b in np.flatnonzero(t['fast'] & (t['ins_lo'] == i)):
            a = int(t['p0'][b] - t['ins_ph0'][i])
            seg.append(np.bincount(ch[a:a + int(t['p1'][b] - t['p0'][b])], minlength=NCH))
    fs_calls = np.unique(t['call'][t['fullsort']])
    z = np.zeros(0, dtype=np.int64)
    ht = np.concatenate(ht) if ht else z
    fs = sizes[prim[fs_calls]].ravel() if len(fs_calls) else z
    ap = sizes[o['call_kind'] == 3].ravel()
    return dict(head_tail=ht[ht > 0], fullsort=fs[fs > 0], afterpulse=ap[ap > 0], segment=np.concatenate(seg) if seg else z)


def _classes(prefix, x, exact=(12, 13, 64, 65)):
    out = set()
    if np.any((x >= 2) & (x <= ORDER_INLINE)): out.add(f'{prefix}_2_12')
    if np.any((x > ORDER_INLINE) & (x <= ORDER_WAVE)): out.add(f'{prefix}_13_64')
    if np.any((x > ORDER_WAVE) & (x <= ORDER_MAX)): out.add(f'{prefix}_65_4096')
    if np.any(x > ORDER_MAX): out.add(f'{prefix}_above_4096')
    for v in exact:
        if np.any(x == v): out.add(f'{prefix}_exactly_{v}')
    return out


# the rows of the seam table
ROWS = [
    # block grid
    'batch_below_one_block', 'photons_multiple_of_2048', 'fewer_than_8_blocks', 'blocks_not_multiple_of_8', 'single_photon',
    # fast blocks
    'r0_and_3_is_0', 'r0_and_3_is_1', 'r0_and_3_is_2', 'r0_and_3_is_3', 'window_lost_electrons', 'window_poisson_zeros', 'window_zero_run_8',
    'nwin_512', 'nwin_513',
    # generic blocks
    'block_two_instructions', 'block_100_instructions', 'block_photonless_amp0_between', 'block_photonless_all_lost_between',
    'wide_block_inside', 'wide_block_at_first_photon', 'wide_block_at_last_photon',
    # tile layout of a single-instruction set
    'layout_head_ranges_tail', 'layout_ranges_only', 'layout_head_only', 'layout_ranges_tail_no_head', 'layout_head_tail_no_ranges',
    # sizes of what gets ordered (a head or a tail lies in one block: at most 2048 photons, no row above 4096)
    'head_tail_2_12', 'head_tail_13_64', 'head_tail_65_4096', 'head_tail_exactly_12', 'head_tail_exactly_13', 'head_tail_exactly_64', 'head_tail_exactly_65',
    'fullsort_2_12', 'fullsort_13_64', 'fullsort_65_4096', 'fullsort_above_4096', 'fullsort_exactly_12', 'fullsort_exactly_13', 'fullsort_exactly_64',
    'fullsort_exactly_65',
    'afterpulse_2_12', 'afterpulse_13_64', 'afterpulse_65_4096', 'afterpulse_above_4096', 'afterpulse_exactly_12', 'afterpulse_exactly_13',
    'afterpulse_exactly_64', 'afterpulse_exactly_65',
    # (block, channel) segments
    'segment_0', 'segment_1', 'segment_2_64', 'segment_exactly_64', 'segment_exactly_65', 'segment_far_above_64',
    # run sets
    'run_set_3_s1', 'run_set_3_s2', 'run_set_photonless_middle', 'run_set_large_and_small',
    # emitter front end
    's2_ends_on_256_emitters', 's2_ends_on_512_more_emitters', 'at_least_300_s2_of_amp_1', 'amp0_first', 'amp0_middle', 'amp0_last', 's1_behind_last_s2',
    's1_amplitudes_1_3_4_5_255_256_257_1023',
]


def seams(case, s, orc, o, t):
    """the rows of ROWS this case reaches"""
    s_ins, ip = s['s_ins'], s['ip']
    n = len(s_ins)
    out = set()
    P, nb = t['n_photons'], t['n_blocks']
    if 0 < P < GEN_BLOCK: out.add('batch_below_one_block')
    if P > 0 and P % GEN_BLOCK == 0: out.add('photons_multiple_of_2048')
    if 0 < nb < 8: out.add('fewer_than_8_blocks')
    if nb % 8: out.add('blocks_not_multiple_of_8')
    if P == 1: out.add('single_photon')
    is_s2 = s_ins['type'] != 1
    for b in np.flatnonzero(t['fast']):
        i = t['ins_lo'][b]
        out.add(f'r0_and_3_is_{int(t["r0"][b]) & 3}')
        if is_s2[i] and t['zeros'][b]:
            out.add('window_lost_electrons' if ip['p_hit'][i] < 1.0 else 'window_poisson_zeros')
            if t['zero_run'][b] >= 8: out.add('window_zero_run_8')
        if t['nwin'][b] == GEN_WIN: out.add('nwin_512')
    for b in np.flatnonzero(~t['fast']):
        i0, i1 = t['ins_lo'][b], t['ins_hi'][b]
        with_photons = [i for i in range(i0, i1 + 1) if min(t['p1'][b], t['ins_ph0'][i + 1]) > max(t['p0'][b], t['ins_ph0'][i])]
        if len(with_photons) == 2: out.add('block_two_instructions')
        if len(with_photons) >= 100: out.add('block_100_instructions')
        for i in range(i0 + 1, i1):
            if t['ins_nph'][i] == 0 and s_ins['amp'][i] == 0: out.add('block_photonless_amp0_between')
            if t['ins_nph'][i] == 0 and s_ins['amp'][i] > 0: out.add('block_photonless_all_lost_between')
        if i0 == i1:                                             # generic for its width alone
            if t['nwin'][b] == GEN_WIN + 1: out.add('nwin_513')
            if t['ins_ph0'][i0] < t['p0'][b] and t['ins_ph0'][i0 + 1] > t['p1'][b]: out.add('wide_block_inside')
            elif t['ins_ph0'][i0] == t['p0'][b] and not t['fullsort'][i0]: out.add('wide_block_at_first_photon')
            elif t['ins_ph0'][i0 + 1] == t['p1'][b] and t['ins_ph0'][i0] < t['p0'][b] and not t['fullsort'][i0]: out.add('wide_block_at_last_photon')
    for i in np.flatnonzero(~t['fullsort'] & (t['ins_nph'] > 0)):
        lay = (bool(t['head'][i]), bool(t['n_fast'][i]), bool(t['tail'][i]))
        name = {(True, True, True): 'layout_head_ranges_tail', (False, True, False): 'layout_ranges_only', (True, False, False): 'layout_head_only',
                (False, True, True): 'layout_ranges_tail_no_head', (True, False, True): 'layout_head_tail_no_ranges'}.get(lay)
        assert name or lay == (True, True, False), (i, lay)      # (a tail without ranges and without a head does not exist)
        if name: out.add(name)
    z = ordered_sizes(orc, o, s, t)
    out |= _classes('head_tail', z['head_tail']) | _classes('fullsort', z['fullsort']) | _classes('afterpulse', z['afterpulse'])
    sg = z['segment']
    if len(sg):
        if np.any(sg == 0): out.add('segment_0')
        if np.any(sg == 1): out.add('segment_1')
        if np.any((sg >= 2) & (sg <= 64)): out.add('segment_2_64')
        if np.any(sg == 64): out.add('segment_exactly_64')
        if np.any(sg == 65): out.add('segment_exactly_65')
        if np.any(sg > 500): out.add('segment_far_above_64')
    # run sets
    call = t['call']
    for q in np.flatnonzero(np.bincount(call) >= 3):
        m = np.flatnonzero(call == q)
        kind = 's1' if s_ins['type'][m[0]] == 1 else 's2'
        if (t['ins_nph'][m] > 0).all(): out.add(f'run_set_3_{kind}')
        if t['ins_nph'][m[0]] > 0 and t['ins_nph'][m[-1]] > 0 and (t['ins_nph'][m[1:-1]] == 0).any(): out.add('run_set_photonless_middle')
    for q in np.flatnonzero(np.bincount(call) >= 2):
        k = t['ins_nph'][call == q]
        if k.max() > 20000 and 0 < k.min() < 200: out.add('run_set_large_and_small')
    # emitter front end
    ends = t['em_off'][1:][is_s2 & (s_ins['amp'] > 0)]
    if np.any(ends % 256 == 0): out.add('s2_ends_on_256_emitters')
    if np.any((ends % 256 == 0) & (ends >= 512)): out.add('s2_ends_on_512_more_emitters')
    if int(np.sum(is_s2 & (s_ins['amp'] == 1))) >= 300: out.add('at_least_300_s2_of_amp_1')
    if n > 2:
        if s_ins['amp'][0] == 0: out.add('amp0_first')
        if np.any(s_ins['amp'][1:-1] == 0): out.add('amp0_middle')
        if s_ins['amp'][-1] == 0: out.add('amp0_last')
    if is_s2.any() and np.flatnonzero(~is_s2).max(initial=-1) > np.flatnonzero(is_s2).max():
        out.add('s1_behind_last_s2')
        if {1, 3, 4, 5, 255, 256, 257, 1023} <= set(s_ins['amp'][~is_s2].tolist()): out.add('s1_amplitudes_1_3_4_5_255_256_257_1023')
    return out, z
