"""Designed instruction spacings for the digitise-window rule: the case table behind tests/golden/window_edges.npz and
window_edges_tpc.npz (make_golden.py window_edges runs the reference's RawDataOptical on them), and what the tests read back from the
fixtures.  Shared by make_golden.py, tests/test_window_edges_reference.py and tests/test_gpu_window_edges.py.  No test lives here.

The rule (rawdata.py:96-98): before a cluster of instructions is simulated the pulse cache is digitised when
    min(instruction time of the cluster) - last_pulse_end_time > right_raw_extension
and a pulse exists; last_pulse_end_time is the running maximum of (pulse right x sample_duration) over everything simulated so far
(rawdata.py:188-190), -inf before the first pulse.  A DECISION is one evaluation of that rule, one per cluster; its `diff` is
tmin - last_pulse_end_time - right_raw_extension: the cache is digitised ("flush") when diff > 0.

With pmt_transit_time_spread = 0 the transit-time draw (pulse.py:53-56) adds the constant int(pmt_transit_time_mean) to every photon,
so the pulse of a photon that enters Pulse.__call__ at T ns has (pulse.py:118-127)
    left = (T + ttm) // dt - samples_to_store_before - samples_before_pulse_center
    right = (T + ttm) // dt + samples_to_store_after + samples_after_pulse_center
and every diff can be designed to the ns.  All of dt, the stored and template samples, trigger_window, right_raw_extension, ttm, the
accepted photon window and the dead PMTs are read from the config; nothing of them is mirrored here.

Every cluster carries `expect`: whether the reference digitises the cache before it.  The Stream checks each against the formulas above
when the case is built; the generator checks each against what the reference did.
"""
import numpy as np

from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype

SECTIONS = ['A', 'B', 'C', 'D', 'E', 'F', '-']          # '-': clusters that only separate cases (each far behind everything before it)
A_VARIANTS = ['previous', 'three_back', 'two_equal']
FIXTURES = dict(nveto='window_edges.npz', tpc='window_edges_tpc.npz')


class Stream:
    """collects clusters of optical instructions in time order and follows the reference's state (last_pulse_end_time) with the formulas
    of the module docstring"""

    def __init__(self, cfg, t0=1_000_003):
        self.dt = int(cfg.get('sample_duration', 10))
        self.before = int(cfg['samples_to_store_before']) + int(cfg.get('samples_before_pulse_center', 2))
        self.after = int(cfg['samples_to_store_after']) + int(cfg.get('samples_after_pulse_center', 20))
        self.tw = int(cfg['trigger_window'])
        self.rext = int(cfg['right_raw_extension'])
        self.ttm = int(np.float64(cfg['pmt_transit_time_mean']))             # (np.random.normal(mean, 0, n).astype(np.int64))
        assert float(cfg['pmt_transit_time_spread']) == 0.0
        self.cutoff = int(cfg.get('nveto_time_max_cutoff', int(1e6)))
        self.dead = set(np.flatnonzero(np.asarray(cfg['gains']) == 0).tolist())
        self.n_channels = len(cfg['gains'])
        self.t0 = t0
        self.E = None                   # last_pulse_end_time; None: -inf
        self.last_time = None           # time of the last instruction
        self.ins = []                   # (time, [(channel, timing), ...])
        self.clusters = []              # dict(first, n, tmin, section, variant, delta, diff, expect, end, parity, tag)
        self.pulses = []                # per instruction [(channel, left, right)], channel ascending: the prediction

    # ---- the formulas
    def pulse_bounds(self, T):
        b = (T + self.ttm) // self.dt
        return b - self.before, b + self.after

    def end_of(self, T):
        return self.pulse_bounds(T)[1] * self.dt

    def kept(self, ch, timing):
        return 0 <= timing < self.cutoff and ch not in self.dead

    # ---- placing clusters
    def at(self, delta):
        """the cluster time that puts the decision `delta` ns behind the threshold"""
        return self.E + self.rext + delta

    def fresh(self, parity=None):
        """a time far behind everything so far; parity: of (pulse left - trigger_window) of a photon with timing 0 at that time"""
        t = self.t0 if self.last_time is None else max(self.last_time, self.E or 0) + 3 * self.rext + 7 * self.dt + 3
        if parity is not None:
            while (self.pulse_bounds(t)[0] - self.tw) % 2 != parity:
                t += self.dt
        return t

    def add(self, tmin, instrs, section, expect, variant='', delta=None, parity=None, tag=''):
        """one cluster.  instrs: [(offset from tmin, [(channel, timing), ...]), ...], offsets ascending from 0 with gaps of at most
        right_raw_extension; delta: the designed diff; parity: the designed parity of min(pulse left) - trigger_window of the window
        this cluster opens"""
        assert instrs[0][0] == 0 and all(0 <= b[0] - a[0] <= self.rext for a, b in zip(instrs[:-1], instrs[1:]))
        assert self.last_time is None or tmin - self.last_time > self.rext, 'a new cluster: more than right_raw_extension behind the last instruction'
        diff = None if self.E is None else tmin - self.E - self.rext
        assert expect == (diff is not None and diff > 0), (section, variant, delta, diff, expect)
        assert delta is None or diff == delta, (section, variant, delta, diff)
        c = dict(first=len(self.ins), n=len(instrs), tmin=tmin, section=section, variant=variant, delta=delta, diff=diff, expect=bool(expect),
                 end=None, parity=parity, tag=tag)
        self.clusters.append(c)
        for off, photons in instrs:
            t = tmin + off
            per_ch = {}
            for ch, timing in photons:
                assert 0 <= ch < self.n_channels
                if self.kept(ch, timing):
                    l, r = self.pulse_bounds(t + timing)
                    a = per_ch.get(ch, (l, r))
                    per_ch[ch] = (min(a[0], l), max(a[1], r))
            self.ins.append((t, list(photons)))
            self.pulses.append([(ch,) + per_ch[ch] for ch in sorted(per_ch)])
            for l, r in per_ch.values():
                c['end'] = r * self.dt if c['end'] is None else max(c['end'], r * self.dt)
            self.last_time = t
        if c['end'] is not None:            # the cluster's pulses join the running maximum (rawdata.py:188-190)
            self.E = c['end'] if self.E is None else max(self.E, c['end'])
        return c

    def separator(self, ch=1):
        """a single-photon cluster far behind everything: closes the case before it"""
        return self.add(self.fresh(), [(0, [(ch, 0)])], '-', expect=self.E is not None)

    # ---- what the generator and the tests read
    def inputs(self):
        """(instructions with _first / _last, flat channels, flat timings)"""
        n = len(self.ins)
        ins = np.zeros(n, dtype=instruction_dtype + optical_extra_dtype)
        nph = np.array([len(p) for _, p in self.ins], dtype=np.int64)
        ins['type'], ins['event_number'], ins['amp'], ins['recoil'] = 1, np.arange(n), nph, 7
        ins['time'] = [t for t, _ in self.ins]
        ins['_last'] = np.cumsum(nph)
        ins['_first'] = ins['_last'] - nph
        assert np.all(np.diff(ins['time']) >= 0)
        channels = np.array([ch for _, p in self.ins for ch, _ in p], dtype=np.int64)
        timings = np.array([tm for _, p in self.ins for _, tm in p], dtype=np.int64)
        return ins, channels, timings

    def table(self):
        """the decisions as flat arrays (stored in the fixture as dec_*)"""
        c = self.clusters
        big = np.iinfo(np.int64).min
        return dict(dec_first=np.array([x['first'] for x in c], dtype=np.int64), dec_n=np.array([x['n'] for x in c], dtype=np.int64),
                    dec_tmin=np.array([x['tmin'] for x in c], dtype=np.int64),
                    dec_section=np.array([SECTIONS.index(x['section']) for x in c], dtype=np.int8),
                    dec_variant=np.array([x['variant'] for x in c]), dec_tag=np.array([x['tag'] for x in c]),
                    dec_has_delta=np.array([x['delta'] is not None for x in c]),
                    dec_delta=np.array([0 if x['delta'] is None else x['delta'] for x in c], dtype=np.int64),
                    dec_has_diff=np.array([x['diff'] is not None for x in c]),
                    dec_diff=np.array([big if x['diff'] is None else x['diff'] for x in c], dtype=np.int64),
                    dec_expect=np.array([x['expect'] for x in c]),
                    dec_parity=np.array([-1 if x['parity'] is None else x['parity'] for x in c], dtype=np.int8))

    def predicted_pulses(self):
        """(pulse offsets per instruction, channel, left, right) in the order Pulse.__call__ makes them"""
        off = np.concatenate([[0], np.cumsum([len(p) for p in self.pulses])]).astype(np.int64)
        flat = [x for p in self.pulses for x in p]
        return off, *(np.array([x[k] for x in flat], dtype=np.int64) for k in range(3))

    def predicted_windows(self):
        """(left, right) of the digitise windows (rawdata.py:215-222): the clusters between two flushes, empty caches left out"""
        out, lo, hi = [], None, None
        for c in self.clusters:
            if c['expect'] and lo is not None:
                out.append((lo, hi))
                lo = hi = None
            for p in self.pulses[c['first']:c['first'] + c['n']]:
                for _, l, r in p:
                    lo, hi = (l, r) if lo is None else (min(lo, l), max(hi, r))
        if lo is not None:
            out.append((lo, hi))
        left = np.array([l - self.tw for l, _ in out], dtype=np.int64)
        return left - left % 2, np.array([r + self.tw for _, r in out], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- the sections
def section_a(s, chs):
    """threshold: the next cluster's minimum instruction time is E + rext + delta, delta -1, 0, +1; a flush only at +1.  E set by the
    previous cluster / by a cluster three back through one late photon (the clusters between end earlier: the running maximum, not the
    last end) / by two clusters with the same end"""
    a, b, c, d = chs
    for delta in (-1, 0, 1):
        s.add(s.fresh(), [(0, [(a, 3)])], 'A', expect=s.E is not None, variant='previous', tag='sets_E')
        s.add(s.at(delta), [(0, [(b, 0)])], 'A', expect=delta > 0, variant='previous', delta=delta)
    for delta in (-1, 0, 1):
        t1 = s.fresh()
        late = 3 * s.rext + 1234
        s.add(t1, [(0, [(a, 0), (d, late)])], 'A', expect=True, variant='three_back', tag='sets_E')
        e_run = s.E
        assert e_run == s.end_of(t1 + late)
        t2 = t1 + s.rext + 10
        for k, ch in enumerate((b, c)):         # they end earlier, and no cache is digitised in front of them
            cl = s.add(t2 + k * (s.rext + 10), [(0, [(ch, 5)])], 'A', expect=False, variant='three_back', tag='ends_earlier')
            assert cl['end'] < e_run and s.E == e_run
        s.add(s.at(delta), [(0, [(a, 0)])], 'A', expect=delta > 0, variant='three_back', delta=delta)
    for delta in (-1, 0, 1):
        t1 = s.fresh()
        late = s.rext + 500
        s.add(t1, [(0, [(a, late)])], 'A', expect=True, variant='two_equal', tag='sets_E')
        e1 = s.E
        t2 = t1 + s.rext + 1
        cl = s.add(t2, [(0, [(b, t1 + late - t2)])], 'A', expect=False, variant='two_equal', tag='same_end')
        assert cl['end'] == e1 == s.E
        s.add(s.at(delta), [(0, [(c, 0)])], 'A', expect=delta > 0, variant='two_equal', delta=delta)


def section_b(s):
    """whose time counts: the cluster minimum belongs to an instruction that makes no pulse (_first == _last, or every photon cut:
    negative, at / behind the cutoff, on the dead PMT) while another instruction of the cluster makes one; whole clusters without pulses"""
    dead = sorted(s.dead)[0]
    cut = [(5, -1), (6, s.cutoff), (dead, 0), (9, -300), (8, 2 * s.cutoff)]
    for variant, first in (('first_equals_last', []), ('all_cut', cut)):
        for delta in (-1, 1):
            s.add(s.fresh(), [(0, [(20, 0)])], 'B', expect=True, variant=variant, tag='sets_E')
            # the pulse comes from an instruction 30 ns later: at delta -1 it is behind the threshold itself, and does not count
            s.add(s.at(delta), [(0, first), (30, [(21, 0)])], 'B', expect=delta > 0, variant=variant, delta=delta)
    # a whole cluster without pulses more than rext behind E: the cache is digitised, E stays (the next decision finds an empty cache)
    for variant, photons in (('pulseless_beyond', []), ('pulseless_beyond_cut', cut)):
        s.add(s.fresh(), [(0, [(22, 0)])], 'B', expect=True, variant=variant, tag='sets_E')
        e = s.E
        s.add(s.at(1), [(0, photons), (40, [])], 'B', expect=True, variant=variant, delta=1, tag='pulseless')
        assert s.E == e
        s.add(s.last_time + s.rext + 1, [(0, [(23, 0)])], 'B', expect=True, variant=variant, tag='empty_cache')
    # a whole cluster without pulses within rext of E changes nothing: the decision behind it is made against the same E
    for delta in (-1, 1):
        t1 = s.fresh()
        s.add(t1, [(0, [(24, 0), (25, 3 * s.rext + 77)])], 'B', expect=True, variant='pulseless_within', tag='sets_E')
        e = s.E
        s.add(t1 + s.rext + 10, [(0, cut if delta > 0 else [])], 'B', expect=False, variant='pulseless_within', tag='pulseless')
        assert s.E == e
        s.add(s.at(delta), [(0, [(26, 0)])], 'B', expect=delta > 0, variant='pulseless_within', delta=delta)


def section_c(s):
    """before any pulse: three clusters without pulses more than rext apart open the stream -- no window, no flush; then the first
    pulse, then a decision at +1"""
    assert s.E is None and not s.ins
    dead = sorted(s.dead)[0]
    t = s.fresh()
    for k, photons in enumerate(([], [(3, -5), (4, s.cutoff)], [(dead, 0), (dead, 10)])):
        s.add(t + k * (2 * s.rext + 11), [(0, photons)], 'C', expect=False, variant='no_pulse_yet', tag='pulseless')
    assert s.E is None
    s.add(s.last_time + 5 * s.rext, [(0, [(30, 0)])], 'C', expect=False, variant='no_pulse_yet', tag='first_pulse')
    s.add(s.at(1), [(0, [(31, 0)])], 'C', expect=True, variant='no_pulse_yet', delta=1)


def section_d(s):
    """even landing (rawdata.py:221-222): windows whose min(pulse left) - trigger_window is odd and even, of one cluster and merged"""
    for parity in (1, 0):
        s.add(s.fresh(parity), [(0, [(40, 0), (41, 2 * s.dt)])], 'D', expect=True, variant='single', parity=parity)
        s.add(s.fresh(parity), [(0, [(42, 0)])], 'D', expect=True, variant='merged', parity=parity)
        s.add(s.at(-5), [(0, [(43, 0)])], 'D', expect=False, variant='merged', delta=-5, tag='merges')


def section_e(s, chs):
    """rows inside one merged window of four clusters.  x: hit by instructions of three clusters with idle stretches between (the row
    spans the union, several ZLE intervals); y: hit only by the last cluster; p, q: their pulses start and end the window; x2: next to x"""
    x, x2, y, p, q = chs
    s.add(s.fresh(), [(0, [(p, 0)]), (2 * s.dt, [(x, 4)] * 3)], 'E', expect=True, variant='rows', tag='first')
    s.add(s.at(-10), [(0, [(x, 1)] * 3 + [(x2, 0)] * 2)], 'E', expect=False, variant='rows', delta=-10)
    s.add(s.at(-10), [(0, [(x2, 7)] * 2)], 'E', expect=False, variant='rows', delta=-10)
    s.add(s.at(-10), [(0, [(x, 0)] * 3 + [(y, 2)] * 3), (3 * s.dt, [(q, 40 * s.dt)] * 2)], 'E', expect=False, variant='rows', delta=-10, tag='last')


def section_f(s):
    """host clustering (np.diff > rext, rawdata.py:63): instruction gaps of exactly rext and rext + 1, and equal instruction times.  The
    first instruction of each probe makes no pulse and sits exactly at the threshold (delta 0); the second makes one.  Gap rext: one
    cluster, its minimum is the first instruction's, no flush.  Gap rext + 1: a cluster of its own, rext + 1 behind the threshold"""
    s.add(s.fresh(), [(0, [(50, 0)])], 'F', expect=True, variant='gap_rext', tag='sets_E')
    s.add(s.at(0), [(0, []), (s.rext, [(51, 0)])], 'F', expect=False, variant='gap_rext', delta=0)
    s.add(s.fresh(), [(0, [(50, 0)])], 'F', expect=True, variant='gap_rext_plus_1', tag='sets_E')
    s.add(s.at(0), [(0, [])], 'F', expect=False, variant='gap_rext_plus_1', delta=0, tag='pulseless')
    s.add(s.last_time + s.rext + 1, [(0, [(51, 0)])], 'F', expect=True, variant='gap_rext_plus_1', delta=s.rext + 1)
    # the same with pulses in both instructions: exactly rext apart, they are one cluster, and the instruction rext + 1 behind is not
    s.add(s.fresh(), [(0, [(52, 0)]), (s.rext, [(53, 0)])], 'F', expect=True, variant='gap_rext_pulses')
    c = s.add(s.last_time + s.rext + 1, [(0, [(54, 0)])], 'F', expect=False, variant='gap_rext_pulses', tag='merges')
    assert c['diff'] < 0
    # equal instruction times: two pulse-making instructions; an empty one and a pulse-making one (the empty one first in the input)
    s.add(s.fresh(), [(0, [(55, 0)]), (0, [(56, 6)])], 'F', expect=True, variant='equal_times', tag='sets_E')
    s.add(s.at(1), [(0, []), (0, [(57, 0)])], 'F', expect=True, variant='equal_times', delta=1)
    s.add(s.at(0), [(0, [(58, 0)]), (0, []), (0, [(59, 1)])], 'F', expect=False, variant='equal_times', delta=0)


def nveto_cases(cfg):
    """window_edges.npz: the 120-channel neutron-veto configuration of the optical chains (one dead PMT, right_raw_extension 2000)"""
    s = Stream(cfg)
    section_c(s)
    s.separator()
    section_a(s, (10, 11, 12, 13))
    s.separator()
    section_b(s)
    s.separator()
    section_d(s)
    s.separator()
    section_e(s, (63, 64, s.n_channels - 1, 0, 100))
    s.separator()
    section_f(s)
    s.separator()
    return s


def tpc_cases(cfg):
    """window_edges_tpc.npz: the bundled TPC configuration (494 channels, right_raw_extension 100000): sections A and E.  E: a top channel
    (it has a high-energy row) starts the window, a bottom channel ends it, 63 / 64 and the last channel in between"""
    s = Stream(cfg)
    section_a(s, (10, 300, 252, 253))
    s.separator()
    n_top = int(cfg['n_top_pmts'])
    section_e(s, (63, 64, s.n_channels - 1, 17, n_top + 47))
    s.separator()
    return s


CASES = dict(nveto=nveto_cases, tpc=tpc_cases)


# ---------------------------------------------------------------------------------------------------------------- reading a fixture
def fixture_decisions(d, rext, dt):
    """every decision the reference made, from the fixture's own arrays: per cluster of the instructions (np.diff(time) > rext) its first
    call, its minimum time, the running maximum of pl_right x dt over the calls before it (None before the first pulse), diff, and whether
    the reference digitised in front of it (flush_at_call: the number of Pulse calls made when digitize_pulse_cache was entered), and the
    end (max pulse right x dt) of its own pulses (None: it made none)"""
    t = np.asarray(d['instructions']['time'], dtype=np.int64)
    assert np.all(np.diff(t) >= 0)                  # (so call k is instruction k)
    first = np.concatenate([[0], np.flatnonzero(np.diff(t) > rext) + 1])
    call_end = np.full(len(t), np.iinfo(np.int64).min)
    for k in range(len(t)):
        a, b = int(d['call_pulse_off'][k]), int(d['call_pulse_off'][k + 1])
        if b > a:
            call_end[k] = int(d['pl_right'][a:b].max()) * dt
    flushed = set(np.asarray(d['flush_at_call']).tolist())
    out, run = [], None
    for c, k0 in enumerate(first):
        k1 = int(first[c + 1]) if c + 1 < len(first) else len(t)
        tmin = int(t[k0:k1].min())
        e = int(call_end[k0:k1].max())
        e = None if e == np.iinfo(np.int64).min else e
        out.append(dict(first=int(k0), n=k1 - int(k0), tmin=tmin, E=run, diff=None if run is None else tmin - run - rext, flush=int(k0) in flushed,
                        end=e))
        if e is not None:
            run = e if run is None else max(run, e)
    return out


def tile_stream(d, shifts, fillers, cfg, share_photons=False):
    """the recorded stream of a fixture tiled: copy j shifted by shifts[j] ns; fillers: [(time, ...)] of single instructions without photons
    (_first == _last), anywhere.  Returns a dict with what replay_chain_on_engine / replay_chain_on_oracle, RawDataOptical and
    simulate_optical read (instructions, channels, timings, call_*, ph_*, dg_first_pulse, dg_n_pulses, set_cluster, set_tmin) plus
    copy_of_call (-1: filler) -- instructions in time order, one call per instruction.  Every copy has its own stretch of the flat
    channels / timings arrays; share_photons: all copies name the fixture's one stretch instead (overlapping _first:_last ranges, which
    rawdata.py:477 takes as they come)"""
    from wfsim_amd.scheduler import schedule
    ins0 = d['instructions']
    n0, nf = len(ins0), len(fillers)
    ins = np.zeros(n0 * len(shifts) + nf, dtype=ins0.dtype)
    src = np.full(len(ins), -1, dtype=np.int64)          # call of the fixture behind every instruction
    copy = np.full(len(ins), -1, dtype=np.int64)
    for j, sh in enumerate(shifts):
        blk = ins0.copy()
        blk['time'] += sh
        if not share_photons:
            blk['_first'] += j * len(d['channels'])
            blk['_last'] += j * len(d['channels'])
        ins[j * n0:(j + 1) * n0] = blk
        src[j * n0:(j + 1) * n0] = np.arange(n0)
        copy[j * n0:(j + 1) * n0] = j
    fill = np.zeros(nf, dtype=ins0.dtype)
    fill['type'], fill['recoil'], fill['time'] = 1, 7, np.asarray(fillers, dtype=np.int64)
    ins[n0 * len(shifts):] = fill
    o = np.argsort(ins['time'], kind='stable')
    ins, src, copy = ins[o], src[o], copy[o]
    ins['event_number'] = np.arange(len(ins))
    shift_of = np.where(copy >= 0, np.asarray(shifts, dtype=np.int64)[np.maximum(copy, 0)], 0)
    reps = 1 if share_photons else len(shifts)
    out = dict(instructions=ins, channels=np.tile(d['channels'], reps), timings=np.tile(d['timings'], reps), copy_of_call=copy, call_of_call=src)
    live = src >= 0
    nph = np.where(live, np.diff(d['call_ph_off'])[np.maximum(src, 0)], 0)
    npl = np.where(live, np.diff(d['call_pulse_off'])[np.maximum(src, 0)], 0)
    out['call_ph_off'] = np.concatenate([[0], np.cumsum(nph)]).astype(np.int64)
    out['call_pulse_off'] = np.concatenate([[0], np.cumsum(npl)]).astype(np.int64)
    idx = np.concatenate([np.arange(d['call_ph_off'][k], d['call_ph_off'][k + 1]) for k in src[live]] + [np.zeros(0, np.int64)]).astype(np.int64)
    out['ph_t'] = d['ph_t'][idx] + np.repeat(shift_of[live], nph[live])
    for k in ('ph_ch', 'ph_dpe', 'ph_gain'):
        out[k] = d[k][idx]
    out['call_kind'] = np.where(live, d['call_kind'][np.maximum(src, 0)], 0).astype(np.int8)
    out['call_has_gains'] = np.zeros(len(ins), dtype=bool)
    # the reference's windows, copy by copy: pulses of copy j are consecutive (the copies do not interleave)
    assert np.all(np.diff(copy[live]) >= 0)
    P0 = int(d['call_pulse_off'][-1])
    out['dg_first_pulse'] = np.concatenate([d['dg_first_pulse'] + j * P0 for j in range(len(shifts))]).astype(np.int64)
    out['dg_n_pulses'] = np.tile(d['dg_n_pulses'], len(shifts)).astype(np.int64)
    order, key, cluster = schedule(ins, cfg)
    assert np.array_equal(order, np.arange(len(ins)))
    out['set_cluster'] = cluster.astype(np.int32)
    out['set_tmin'] = key.astype(np.int64)             # (per pulse set: the key of its instruction, as tests/helpers.py chain_sets)
    return out
