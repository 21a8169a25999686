"""PMT afterpulses behind supplied photons (RawDataOptical with enable_pmt_afterpulses): the expectation the device is held to.

The oracle's optical scheduler (orc_simulate_optical) makes no afterpulse call, so the expectation is put together from two pieces,
both pinned on the CPU (tests/test_optical_afterpulse_cpu.py):

* ``afterpulses_of``: the oracle's pmt_afterpulse_call (oracle/wfsim_oracle.c, afterpulse.py:172-249) restated in numpy on the
  oracle's Philox -- pinned against the oracle's own kind-3 call behind a tile-generated S2;
* ``drive_optical``: orc_simulate_optical restated call by call (RawData.sim_data, rawdata.py:166-190: the afterpulse Pulse call
  behind every primary call that made a photon) -- pinned, afterpulses off, against orc_simulate_optical byte for byte.

No test lives here.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
from wfsim_amd.config import kernel_params

SITE_AP, SITE_AP_SCREEN, SITE_AP_X = 32, 40, 48


class _Philox:
    """the oracle's Philox4x32-10 with the session key (seed low word, seed high word), one call per counter"""

    def __init__(self, seed):
        self.f = O.lib().orc_philox
        self.key = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint32)
        self.ctr, self.out = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
        self.p = [C.c_void_p(a.ctypes.data) for a in (self.ctr, self.key, self.out)]

    def __call__(self, emitter, gid, item, site):
        self.ctr[:] = (emitter, gid, item, site)
        self.f(*self.p)
        return [int(x) for x in self.out]


def u53(a, b):
    return (float(a >> 5) * 67108864.0 + float(b >> 6)) / 9007199254740992.0


def afterpulses_of(seed, tables, gains, modifier, t_modifier, parents):
    """The photons of the afterpulse Pulse call behind the parents (t, ch, dpe, emitter, gid, item), each an array in the order of
    the primary call: (t int64, ch int16, gain float64), element by element in table order, parent by parent, then stably sorted
    by channel -- what the oracle hands to its kind-3 pulse call."""
    t, ch, dpe, em, gid, item = (np.asarray(x) for x in parents)
    draw = _Philox(int(seed))
    modifier, t_modifier = float(modifier), float(t_modifier)
    out_t, out_ch, out_g = [], [], []
    for e, (name, d) in enumerate(tables.items()):
        dc, ac = np.asarray(d['delaytime_cdf'], dtype=np.float64), np.asarray(d['amplitude_cdf'], dtype=np.float64)
        dbin, abin = float(d['delaytime_bin_size']), float(d['amplitude_bin_size'])
        for i in range(len(t)):
            c = int(ch[i])
            sw = draw(int(em[i]), int(gid[i]), int(item[i]), SITE_AP_SCREEN + (e >> 2))
            w = draw(int(em[i]), int(gid[i]), int(item[i]), SITE_AP + e)
            rU0, rU1 = 1.0 - u53(sw[e & 3], w[1]), 1.0 - u53(w[2], w[3])
            row = dc[c]
            rU0 = rU0 / modifier if modifier != 0.0 else np.inf
            if dpe[i]:
                rU0 /= 2
            if not rU0 <= row[-1]:
                continue
            if 'Uniform' in name:
                x = draw(int(em[i]), int(gid[i]), int(item[i]), SITE_AP_X + e)
                delay, amp = (row[0] + (row[1] - row[0]) * u53(x[0], x[1])) * dbin, 1.0
            else:
                delay = int(np.argmin(np.abs(row - rU0))) * dbin - t_modifier
                arow = ac[c] if ac.ndim == 2 else ac
                amp = int(np.argmin(np.abs(arow - rU1))) * abin
            out_t.append(int(float(int(t[i])) + delay))
            out_ch.append(c)
            out_g.append(float(gains[c]) * amp)
    out_t, out_ch, out_g = np.asarray(out_t, dtype=np.int64), np.asarray(out_ch, dtype=np.int16), np.asarray(out_g, dtype=np.float64)
    o = np.argsort(out_ch, kind='stable')
    return out_t[o], out_ch[o], out_g[o]


def primary_items(ins_row, channels, timings, cutoff):
    """index inside the instruction's _first:_last range of every photon of its primary call, in the call's order: the photons that
    survive the cutoff (rawdata.py:485-486), stably sorted by channel"""
    f, l = int(ins_row['_first']), int(ins_row['_last'])
    tr = np.asarray(timings[f:l])
    k = np.flatnonzero((tr >= 0) & (tr < cutoff))
    return k[np.argsort(np.asarray(channels[f:l])[k], kind='stable')]


def optical_primaries(cfg, ins, channels, timings, cutoff, make_oracle):
    """(oracle run of simulate_optical without afterpulses, processing order of the instructions, per call its items)"""
    orc = make_oracle(cfg)
    orc.simulate_optical(ins, np.arange(len(ins), dtype=np.uint32), channels, timings, cutoff)
    o = orc.results()
    order = np.lexsort((np.arange(len(ins)), ins['time']))
    items = []
    for k, i in enumerate(order):
        it = primary_items(ins[i], channels, timings, cutoff)
        a, b = o['call_ph_off'][k], o['call_ph_off'][k + 1]
        assert np.array_equal(np.asarray(channels[ins['_first'][i]:ins['_last'][i]])[it], o['ph_ch'][a:b]), k
        items.append(it)
    return orc, o, order, items


def afterpulses_of_call(cfg, ap_tables, o, k, gid, items):
    """afterpulses_of for primary call k of an optical run (counter (0, gid, item, site))"""
    a, b = o['call_ph_off'][k], o['call_ph_off'][k + 1]
    p = kernel_params(cfg)
    n = b - a
    return afterpulses_of(p['seed'], ap_tables, np.asarray(cfg['gains'], dtype=np.float64), p['pmt_ap_modifier'], p['pmt_ap_t_modifier'],
                          (o['ph_t'][a:b], o['ph_ch'][a:b], o['ph_dpe'][a:b], np.zeros(n, np.int64), np.full(n, gid), items))


class WindowRule:
    """when the scheduler digitises (rawdata.py:64-66, 96-98): in front of an instruction that opens a new cluster (more than
    right_raw_extension behind the previous instruction), if a pulse exists and the instruction is more than right_raw_extension
    behind the end of the latest pulse of the whole session so far (max(pulse right) * dt)"""

    def __init__(self, orc, rext, dt):
        self.orc, self.rext, self.dt, self.prev_t = orc, float(rext), int(dt), None

    def before_instruction(self, t_ins):
        if self.prev_t is None or float(t_ins - self.prev_t) > self.rext:
            right = self.orc.get('pl_right')
            if len(right) and float(t_ins - int(right.max()) * self.dt) > self.rext:
                self.orc.digitize_and_zle(0)
        self.prev_t = t_ins


def drive_optical(cfg, ins, channels, timings, cutoff, ap_tables=None, make_oracle=None):
    """orc_simulate_optical restated call by call on a second oracle session, with the afterpulse Pulse call (kind 3, explicit gains)
    behind every primary call that holds a photon when ``ap_tables`` are given.  Returns (the driven oracle, per primary call the
    afterpulse photons (t, ch, gain) or None, processing order).  Noise must be off: the noise stream id of a window is internal
    to the oracle's scheduler."""
    if make_oracle is None:
        from tests.helpers import make_oracle
    assert not kernel_params(cfg)['enable_noise']
    _, o, order, items = optical_primaries(cfg, ins, channels, timings, cutoff, make_oracle)
    orc = make_oracle(cfg)
    rext, dt = float(cfg['right_raw_extension']), int(cfg['sample_duration'])
    aps = []
    rule = WindowRule(orc, rext, dt)
    for k, i in enumerate(order):
        rule.before_instruction(int(ins['time'][i]))
        a, b = o['call_ph_off'][k], o['call_ph_off'][k + 1]
        orc.pulse_call(0, k, o['ph_t'][a:b], o['ph_ch'][a:b], o['ph_dpe'][a:b], o['ph_gain'][a:b], False)
        ap = None
        if ap_tables and b > a:                                     # afterpulse.py:162-164: no photons, no call
            ap = afterpulses_of_call(cfg, ap_tables, o, k, int(i), items[k])
            orc.pulse_call(3, k, ap[0], ap[1], np.zeros(len(ap[0]), np.uint8), ap[2], True)
        aps.append(ap)
    orc.digitize_and_zle(0)
    return orc, aps, order


def edge_input(n, n_channels, seed, max_photons=8, dead_channel=None, cutoff=int(1e6)):
    """n optical instructions sorted by time, 1 us apart with 30 % gaps of 2.5 .. 9 us, 0 .. max_photons photons each on n_channels
    channels, with the edges the afterpulse path can trip over: an instruction with _first == _last (3), one whose photons are all
    cut (5), photons on a turned-off PMT (7, and 2 % of all), two instructions at the same time (10, 11) and a few photons
    1.5 .. 12 us late.  Returns (instructions, channels, timings)."""
    from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype
    rng = np.random.default_rng(seed)
    ins = np.zeros(n, dtype=instruction_dtype + optical_extra_dtype)
    gaps = np.where(rng.random(n) < 0.3, rng.integers(2500, 9000, n), 1000)
    gaps[11] = 0
    ins['type'], ins['time'], ins['event_number'] = 1, 1_000_000 + np.cumsum(gaps), np.arange(n)
    nph = rng.integers(0, max_photons + 1, n)
    nph[3], nph[5], nph[7], nph[10], nph[11], nph[-1] = 0, max(nph[5], 2), max(nph[7], 3), max(nph[10], 1), max(nph[11], 1), max(nph[-1], 2)
    ins['_last'] = np.cumsum(nph)
    ins['_first'] = ins['_last'] - nph
    ins['amp'] = nph
    tot = int(nph.sum())
    channels = rng.integers(0, n_channels, tot)
    timings = rng.exponential(60, tot).astype(np.int64)
    late = rng.random(tot) < 0.03
    timings[late] += rng.integers(1500, 12000, int(late.sum()))
    timings[rng.random(tot) < 0.01] = -5
    timings[rng.random(tot) < 0.01] = cutoff
    a, b = ins['_first'][5], ins['_last'][5]
    timings[a:b] = np.where(np.arange(b - a) % 2 == 0, -1, cutoff)
    if dead_channel is not None:
        channels[rng.random(tot) < 0.02] = dead_channel
        channels[ins['_first'][7]] = dead_channel
        timings[ins['_first'][7]] = 20
    return ins, channels, timings
