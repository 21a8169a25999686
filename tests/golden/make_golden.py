#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by RUNNING the reference (WFSim v1.2.2).

Run once in the build container (needs /root/reference; the GPU box never runs this):

    python tests/golden/make_golden.py
    python tests/golden/make_golden.py optical_chain pmt_ap_draws     # these two write their own files only
    python tests/golden/make_golden.py pulse_edges                    # so does this one: the reference on designed photon lists
    python tests/golden/make_golden.py window_edges                   # and this one: the reference on designed instruction spacings
    python tests/golden/make_golden.py zle_edges                      # and this one: the reference on rows designed through the noise table
    python tests/golden/make_golden.py spe_channels                   # and this one: the reference on per-channel SPE columns

The reference's hot-path modules are imported under the stubs of ``_ref_stubs.py`` (identity njit, so
every draw comes from numpy's seeded global generator).  What is written is DATA only: inputs and
outputs at the stage boundaries of SURVEY.md section 8c (G1..G7), the cleaned bundled fax config and
the bundled single-channel SPE distribution.  No reference source text is stored.

Stage boundaries captured per chain case (everything downstream of them is deterministic):
  * per Pulse.__call__   : post-TTS photon times, channels, DPE flags, per-photon gains  -> pulses
                           (optical chains: also the photon list on entry, before the transit-time draw)
  * per digitize call    : pulse list -> (left, right, channel mask, raw rows in their active range)
  * per ZLE              : yielded (channel, left, right, data) tuples
  * truth rows
"""
import gzip
import json
import os
import re
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _ref_stubs import import_reference, import_reference_interface, REFERENCE_ROOT   # noqa: E402
from wfsim_amd.dtypes import instruction_dtype, truth_extra_dtype, optical_extra_dtype   # noqa: E402

TMP = '/tmp/wfsim_golden_tmp'
os.makedirs(TMP, exist_ok=True)
N_TPC, N_TOP = 494, 253


# ---------------------------------------------------------------------------------------------
# config / resources
# ---------------------------------------------------------------------------------------------
def load_bundled_config():
    """files/XENONnT_wfsim_config.json with // and # comments and trailing commas removed."""
    out = []
    for line in open(REFERENCE_ROOT + '/files/XENONnT_wfsim_config.json'):
        if line.lstrip().startswith('//'):
            continue
        if '"url_base"' in line:
            continue
        line = re.sub(r'#.*$', '', line)
        line = re.sub(r'\s//.*$', '', line)
        out.append(line)
    txt = ''.join(out)
    txt = re.sub(r',\s*([\]}])', r'\1', txt)
    return json.loads(txt)


def spe_distribution():
    df = pd.read_csv(REFERENCE_ROOT + '/files/XENONnT_spe_distributions_single_channel.csv')
    charge = df['charge'].values.astype(np.float64)
    pdf = df['0'].values.astype(np.float64)
    mean = (charge * pdf).sum() / pdf.sum()
    return charge / mean, pdf, mean       # normalised so the mean SPE scaling factor is 1


def write_spe_csv(path):
    charge, pdf, _ = spe_distribution()
    cols = {'charge': charge}
    for ch in range(N_TPC):
        cols[str(ch)] = pdf
    pd.DataFrame(cols).to_csv(path, index=False)


def synthetic_pmt_positions():
    """A made-up PMT layout (rings) used only to get a non-uniform, position dependent pattern."""
    def rings(n):
        k = np.arange(n)
        r = 48.0 * np.sqrt((k + 0.5) / n)
        phi = k * 2.399963229728653
        return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)
    return np.concatenate([rings(N_TOP), rings(N_TPC - N_TOP)])


PMT_XY = synthetic_pmt_positions()


class SyntheticPatternMap:
    """Host callable standing in for straxen.InterpolatingMap: positions[n, >=2] -> weights[n, 494]."""
    def __init__(self, scale, width_top, width_bottom, floor):
        self.scale, self.wt, self.wb, self.floor = scale, width_top, width_bottom, floor
        self.shape = (N_TPC,)

    def __call__(self, positions, **kw):
        positions = np.asarray(positions, dtype=np.float64)
        d2 = ((positions[:, None, :2] - PMT_XY[None, :, :]) ** 2).sum(axis=2)
        w = np.where(np.arange(N_TPC)[None, :] < N_TOP, self.wt, self.wb)
        return self.scale * (self.floor + np.exp(-d2 / (2 * w ** 2)))


def base_config(**overrides):
    c = load_bundled_config()
    spe_csv = TMP + '/spe_494.csv'
    if not os.path.exists(spe_csv):
        write_spe_csv(spe_csv)
    c.update(dict(
        detector='XENONnT', n_tpc_pmts=N_TPC, n_top_pmts=N_TOP,
        channel_map=dict(tpc=(0, 493), he=(500, 752), aqmon=(790, 807), sum_signal=800),
        gains=np.full(N_TPC, 2e6), channels_bottom=np.arange(N_TOP, N_TPC),
        right_raw_extension=100000, field_distortion_model='none',
        s1_lce_correction_map=['constant dummy', 1, []], se_gain_map=['constant dummy', 1, []],
        diffusion_constant_transverse=0, url_base='/nonexistent', photon_area_distribution=spe_csv,
        seed=1, per_pmt_truth=False, chunk_size=1,
    ))
    c.update(overrides)
    return c


def make_instructions(rows):
    ins = np.zeros(len(rows), dtype=instruction_dtype)
    for i, r in enumerate(rows):
        for k, v in r.items():
            ins[i][k] = v
        ins[i]['event_number'] = r.get('event_number', i)
        ins[i]['recoil'] = r.get('recoil', 7)
    return ins


# ---------------------------------------------------------------------------------------------
# instrumented run of the reference
# ---------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self, ref):
        self.ref = ref
        self.calls = []        # Pulse.__call__ records
        self.digits = []       # digitize records
        self.zle = []          # (digitize index, ch, left, right, data)
        self._gain_parts = None
        self._randint = []
        self.designed_ix = None  # per digitise window the noise start index to hand out instead of the draw (zle_edges)

    def install(self):
        P = self.ref.pulse.Pulse
        rec = self
        orig_call = P.__call__
        orig_add = P.add_current

        def add_current(t, g, pulse_left, dt, templates, cur):
            rec._gain_parts.append(np.array(g, dtype=np.float64))
            return orig_add(t, g, pulse_left, dt, templates, cur)

        def call(self_, *a):
            rec._gain_parts = []
            # the photon list as the caller left it (S1 / S2 fill theirs inside their own __call__ before this one: those
            # entries are the generator's; for RawDataOptical.sim_primary this is what sim_primary itself decided)
            in_t = np.array(self_.__dict__.get('_photon_timings', []), dtype=np.int64)
            in_ch = np.array(self_.__dict__.get('_photon_channels', []), dtype=np.int64)
            orig_call(self_, *a)
            gains = np.concatenate(rec._gain_parts) if rec._gain_parts else np.zeros(0)
            if len(gains) != len(self_._photon_timings):
                # photons on turned-off PMTs are skipped before a gain is drawn (pulse.py:89): stored with gain 0
                live = ~np.isin(self_._photon_channels, self_.config['turned_off_pmts'])
                full = np.zeros(len(self_._photon_timings))
                full[live] = gains
                gains = full
            rec.calls.append(dict(
                kind=type(self_).__name__, in_t=in_t, in_ch=in_ch,
                t=np.array(self_._photon_timings, dtype=np.int64),
                ch=np.array(self_._photon_channels, dtype=np.int64),
                dpe=np.array(self_._photon_is_dpe, dtype=bool),
                gain=gains,
                has_gains='_photon_gains' in self_.__dict__,
                e_t=np.array(getattr(self_, '_electron_timings', []), dtype=np.int64),
                pulses=[dict(p) for p in self_._pulses],
                truth=dict((k, np.array(v)) for k, v in self_._truth_buffer.items()),
            ))
        P.add_current = staticmethod(add_current)
        P.__call__ = call
        self._restore = (orig_call, orig_add)

        R = self.ref.rawdata.RawData
        orig_dig = R.digitize_pulse_cache

        def digitize(self_):
            n_cached = len(self_._pulses_cache)
            first_pulse_id = rec.n_pulses_seen() - n_cached
            old = np.random.randint
            rec._randint = []

            def randint(*a, **k):
                v = old(*a, **k)
                if rec.designed_ix is not None:
                    # a designed start index: one the reference could have drawn (rawdata.py:417: low=0, high=high)
                    v = int(rec.designed_ix[len(rec.digits)])
                    assert k.get('low', 0) == 0 and 0 <= v < k['high'], (len(rec.digits), v, k)
                rec._randint.append(int(v))
                return v
            np.random.randint = randint
            try:
                orig_dig(self_)
            finally:
                np.random.randint = old
            if n_cached == 0:
                return
            m = self_._channel_mask
            chs = np.where(m['mask'])[0]
            rows = [np.array(self_._raw_data[c, m['left'][c]:m['right'][c] + 1]) for c in chs]
            rec.digits.append(dict(
                left=int(self_.left), right=int(self_.right), first_pulse=first_pulse_id, n_pulses=n_cached,
                ch=chs.astype(np.int64), ch_left=m['left'][chs].astype(np.int64),
                ch_right=m['right'][chs].astype(np.int64), rows=rows,
                sum_row=np.array(self_._raw_data[800]), ix_rand=list(rec._randint)))
        R.digitize_pulse_cache = digitize
        self._restore_dig = orig_dig

    def uninstall(self):
        P = self.ref.pulse.Pulse
        P.__call__, add = self._restore
        P.add_current = staticmethod(add)
        self.ref.rawdata.RawData.digitize_pulse_cache = self._restore_dig

    def n_pulses_seen(self):
        return sum(len(c['pulses']) for c in self.calls)


def run_chain(ref, config, instructions, seed, pattern_maps=None, noise=None, ap=None, store_currents=False, ele_ap=None):
    """Run reference RawData over instructions; return flat dict of arrays for np.savez."""
    config = dict(config)
    # the reference caches Resources keyed on file names only; clear so per-case patches do not leak
    ref.load_resource._cached_configs.clear()
    ref.pulse._cached_pmt_current_templates.clear()
    ref.pulse._cached_uniform_to_pe_arr.clear()
    if ap is not None:
        path = TMP + '/pmt_ap.json.gz'
        with gzip.open(path, 'wt') as f:
            json.dump({k: {q: (v.tolist() if isinstance(v, np.ndarray) else v) for q, v in d.items()}
                       for k, d in ap.items()}, f)
        config['photon_ap_cdfs'] = path
        config['enable_pmt_afterpulses'] = True
    if noise is not None:
        path = TMP + '/noise.npz'
        np.savez(path, arr_0=noise)
        config['noise_file'] = path
        config['enable_noise'] = True
    if ele_ap is not None:
        config['enable_electron_afterpulses'] = True
        config['ele_ap_pdfs'] = ''
        orig_get = ref.load_resource.straxen.get_resource
        ref.load_resource.straxen.get_resource = lambda path, fmt='text': (ele_ap if fmt in ('dill', 'pkl.gz') else orig_get(path, fmt=fmt))
    try:
        rd = ref.rawdata.RawData(config)
    finally:
        if ele_ap is not None:
            ref.load_resource.straxen.get_resource = orig_get
    secondaries = []
    if ele_ap is not None:
        rd.resource.uniform_to_ele_ap = ele_ap
        gen = rd.pulses['pi_el'].generate_instruction

        def generate_instruction(signal_pulse, signal_pulse_instruction):
            out = gen(signal_pulse, signal_pulse_instruction)
            if len(out):
                secondaries.append(np.array(out))
            return out
        rd.pulses['pi_el'].generate_instruction = generate_instruction
    if pattern_maps is not None:
        rd.resource.s1_pattern_map = pattern_maps['s1']
        rd.resource.s2_pattern_map = pattern_maps['s2']
    return record_chain(ref, rd, instructions, seed, instruction_dtype + truth_extra_dtype + [('fill', bool)],
                        store_currents=store_currents, secondaries=secondaries if ele_ap is not None else None)


def record_chain(ref, rd, instructions, seed, truth_dtype, store_currents=False, secondaries=None, store_entry=False):
    """Run a constructed reference RawData / RawDataOptical over instructions under the Recorder; flat dict of arrays."""
    truth = np.zeros(max(len(instructions) * 2, 10), dtype=truth_dtype)
    rec = Recorder(ref)
    rec.install()
    np.random.seed(seed)
    try:
        for ch, left, right, data in rd(instructions, truth_buffer=truth, progress_bar=False):
            rec.zle.append((len(rec.digits) - 1, int(ch), int(left), int(right), np.array(data, dtype=np.int64)))
    finally:
        rec.uninstall()

    out = dict(instructions=instructions, seed=np.int64(seed))
    if secondaries is not None:
        out['secondaries'] = np.concatenate(secondaries) if secondaries else np.zeros(0, dtype=instructions.dtype)
    flatten_recorder(rec, out, store_currents=store_currents, store_entry=store_entry)
    out['truth'] = truth[truth['fill']]
    return out


def flatten_recorder(rec, out, store_currents=False, store_entry=False):
    """what the Recorder saw as flat arrays, added to out: call_*, ph_*, e_t, call_truth_*, pl_*, dg_*, row_*, zle_*"""
    calls = rec.calls
    if store_entry:
        out['call_in_off'] = np.concatenate([[0], np.cumsum([len(c['in_t']) for c in calls])]).astype(np.int64)
        out['in_t'] = np.concatenate([c['in_t'] for c in calls] + [np.zeros(0, np.int64)])
        out['in_ch'] = np.concatenate([c['in_ch'] for c in calls] + [np.zeros(0, np.int64)]).astype(np.int16)
    kinds = ['Pulse', 'S1', 'S2', 'PMT_Afterpulse', 'PhotoIonization_Electron', 'PhotoElectric_Electron']
    out['call_kind'] = np.array([kinds.index(c['kind']) for c in calls], dtype=np.int8)
    out['call_has_gains'] = np.array([c['has_gains'] for c in calls], dtype=bool)
    out['call_ph_off'] = np.concatenate([[0], np.cumsum([len(c['t']) for c in calls])]).astype(np.int64)
    out['ph_t'] = np.concatenate([c['t'] for c in calls] + [np.zeros(0, np.int64)])
    out['ph_ch'] = np.concatenate([c['ch'] for c in calls] + [np.zeros(0, np.int64)]).astype(np.int16)
    out['ph_dpe'] = np.concatenate([c['dpe'] for c in calls] + [np.zeros(0, bool)])
    out['ph_gain'] = np.concatenate([c['gain'] for c in calls] + [np.zeros(0)])
    assert len(out['ph_gain']) == len(out['ph_t'])
    out['call_e_off'] = np.concatenate([[0], np.cumsum([len(c['e_t']) for c in calls])]).astype(np.int64)
    out['e_t'] = np.concatenate([c['e_t'] for c in calls] + [np.zeros(0, np.int64)])
    tkeys = sorted(calls[0]['truth'].keys()) if calls else []
    for k in tkeys:
        out['call_truth_' + k] = np.array([c['truth'][k] for c in calls])
    pulses = [p for c in calls for p in c['pulses']]
    out['call_pulse_off'] = np.concatenate([[0], np.cumsum([len(c['pulses']) for c in calls])]).astype(np.int64)
    out['pl_ch'] = np.array([p['channel'] for p in pulses], dtype=np.int16)
    out['pl_left'] = np.array([p['left'] for p in pulses], dtype=np.int64)
    out['pl_right'] = np.array([p['right'] for p in pulses], dtype=np.int64)
    out['pl_photons'] = np.array([p['photons'] for p in pulses], dtype=np.int64)
    if store_currents:
        out['pl_cur_off'] = np.concatenate([[0], np.cumsum([len(p['current']) for p in pulses])]).astype(np.int64)
        out['pl_current'] = np.concatenate([p['current'] for p in pulses])
    d = rec.digits
    out['dg_left'] = np.array([x['left'] for x in d], dtype=np.int64)
    out['dg_right'] = np.array([x['right'] for x in d], dtype=np.int64)
    out['dg_first_pulse'] = np.array([x['first_pulse'] for x in d], dtype=np.int64)
    out['dg_n_pulses'] = np.array([x['n_pulses'] for x in d], dtype=np.int64)
    out['dg_ix_rand'] = np.array([x['ix_rand'][0] if x['ix_rand'] else -1 for x in d], dtype=np.int64)
    out['dg_row_off'] = np.concatenate([[0], np.cumsum([len(x['ch']) for x in d])]).astype(np.int64)
    out['row_ch'] = np.concatenate([x['ch'] for x in d] + [np.zeros(0, np.int64)]).astype(np.int16)
    out['row_left'] = np.concatenate([x['ch_left'] for x in d] + [np.zeros(0, np.int64)])
    out['row_right'] = np.concatenate([x['ch_right'] for x in d] + [np.zeros(0, np.int64)])
    rows = [r for x in d for r in x['rows']]
    out['row_data_off'] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    out['row_data'] = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
    out['dg_sum_min'] = np.array([x['sum_row'].min() for x in d], dtype=np.int64)
    out['dg_sum_total'] = np.array([x['sum_row'].sum() for x in d], dtype=np.int64)
    z = rec.zle
    out['zle_digit'] = np.array([x[0] for x in z], dtype=np.int64)
    out['zle_ch'] = np.array([x[1] for x in z], dtype=np.int16)
    out['zle_left'] = np.array([x[2] for x in z], dtype=np.int64)
    out['zle_right'] = np.array([x[3] for x in z], dtype=np.int64)
    out['zle_data_off'] = np.concatenate([[0], np.cumsum([len(x[4]) for x in z])]).astype(np.int64)
    out['zle_data'] = np.concatenate([x[4] for x in z] + [np.zeros(0, np.int64)]).astype(np.int32)
    assert np.all(out['zle_data'] == np.concatenate([x[4] for x in z] + [np.zeros(0, np.int64)]))
    return out


# ---------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------
def fixture_tables(ref):
    cfg = base_config()
    p = ref.pulse.Pulse(cfg)
    _, pdf, mean = spe_distribution()
    # the charge axis exactly as the reference parsed it back from the CSV (pandas' default float parser is
    # not round-trip exact, so this can differ from charge/mean in the last bit)
    charge = p.resource.photon_area_distribution['charge'].values.astype(np.float64)
    np.savez_compressed(
        HERE + '/tables.npz',
        templates=p._pmt_current_templates, spe_row=p.uniform_to_pe_arr(np.arange(2000) / 2000.0 + 1e-9, 0),
        spe_table_row_full=p._Pulse__uniform_to_pe_arr[7], current_max=p.current_max,
        current_2_adc=np.float64(p.current_2_adc), spe_charge=charge, spe_pdf=pdf, spe_mean=np.float64(mean))
    jcfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in cfg.items()
            if k not in ('photon_area_distribution', 'url_base', 'turned_off_pmts')}
    with open(HERE + '/config_nt.json', 'w') as f:
        json.dump(jcfg, f, indent=0, sort_keys=True)
    return p


def fixture_add_current(ref, p):
    """G1: direct calls of the reference's Pulse.add_current."""
    rng = np.random.default_rng(11)
    T = p._pmt_current_templates
    cases = []

    def case(t, g, extra_left=52, extra_right=70):
        t = np.asarray(t, dtype=np.int64)
        g = np.asarray(g, dtype=np.float64)
        left = int(t.min() // 10) - extra_left
        right = int(t.max() // 10) + extra_right
        cur = np.zeros(right - left + 1)
        ref.pulse.Pulse.add_current(t, g, left, 10, T, cur)
        cases.append((t, g, left, cur))
    case([1234], [1.0])                                   # single photon
    case([1234, 1234, 1234], [0.5, 1.5, 2.25])            # duplicate-ns photons are merged
    case([-37, -31, -5, 0, 3, 9, 10], rng.uniform(1e6, 3e6, 7))     # negative times: floor // and %
    case(rng.integers(10**9, 10**9 + 300, 40), rng.uniform(1e6, 3e6, 40))         # S1-like
    case(rng.normal(5 * 10**8, 600, 2000).astype(np.int64), rng.uniform(0, 6e6, 2000))   # S2-like, collisions
    case(rng.integers(0, 50000, 300), rng.uniform(1e6, 3e6, 300))    # long sparse tile
    out = dict(n=np.int64(len(cases)))
    for i, (t, g, left, cur) in enumerate(cases):
        out[f't{i}'], out[f'g{i}'], out[f'left{i}'], out[f'cur{i}'] = t, g, np.int64(left), cur
    np.savez_compressed(HERE + '/add_current.npz', **out)


def synthetic_afterpulse_tables(rng):
    """Shape per afterpulse.py:181-186: element -> delaytime_cdf[n_ch, n_bins] (NOT normalised: last value
    is the AP probability), amplitude_cdf[n_ch, n_bins] or [n_bins], bin sizes."""
    nb = 200
    out = {}
    for name, p_ap, mean_delay, amp2d in [('He', 0.02, 60, True), ('Xe', 0.012, 140, False)]:
        x = np.arange(nb)
        shape = np.cumsum(np.exp(-0.5 * ((x - mean_delay) / 15.0) ** 2))
        shape /= shape[-1]
        prob = p_ap * rng.uniform(0.5, 1.5, N_TPC)
        dcdf = shape[None, :] * prob[:, None]
        a = np.cumsum(np.exp(-0.5 * ((np.arange(100) - 25) / 8.0) ** 2))
        a /= a[-1]
        acdf = np.repeat(a[None, :], N_TPC, axis=0) if amp2d else a
        out[name] = dict(delaytime_cdf=dcdf, amplitude_cdf=acdf, delaytime_bin_size=10.0, amplitude_bin_size=0.04)
    # 'Uniform' element: delaytime_cdf is [n_ch, 2]; delay ~ U(col0, col1) * bin and the AP probability is col -1
    out['Uniform'] = dict(delaytime_cdf=np.stack([np.full(N_TPC, 0.004), np.full(N_TPC, 0.008)], axis=1),
                          amplitude_cdf=np.ones(3), delaytime_bin_size=1000.0, amplitude_bin_size=1.0)
    return out


def fixture_chains(ref):
    pat = dict(s1=SyntheticPatternMap(14e-5, 30.0, 18.0, 0.15), s2=SyntheticPatternMap(30e-5, 9.0, 25.0, 0.02))
    np.savez_compressed(HERE + '/pattern.npz', pmt_xy=PMT_XY,
                        s1_params=np.array([14e-5, 30.0, 18.0, 0.15]), s2_params=np.array([30e-5, 9.0, 25.0, 0.02]))
    MS = 1_000_000

    # A: S1s -- isolated, plus two overlapping in one cluster (per-pulse rounding, several pulses per row)
    rows = [dict(type=1, time=MS * (i + 1), x=5.0 * i - 20, y=3.0 * i - 10, z=-10.0 - 8 * i, amp=amp)
            for i, amp in enumerate([417, 1667, 60, 5000, 1, 900, 25000])]
    rows += [dict(type=1, time=MS * 9, x=1, y=2, z=-50, amp=1667), dict(type=1, time=MS * 9 + 370, x=-7, y=12, z=-20, amp=1200),
             dict(type=1, time=MS * 9 + 60_000, x=-7, y=12, z=-20, amp=800)]
    np.savez_compressed(HERE + '/chain_s1.npz',
                        **run_chain(ref, base_config(), make_instructions(rows), 101, pat, store_currents=True))

    # B: S2s, S1+S2 pair in one cluster, deep S2
    rows = [dict(type=2, time=MS * 1, x=3, y=-4, z=-10, amp=120),
            dict(type=1, time=MS * 2, x=10, y=10, z=-5, amp=3000), dict(type=2, time=MS * 2, x=10, y=10, z=-5, amp=400),
            dict(type=2, time=MS * 4, x=-30, y=20, z=-95, amp=250),
            dict(type=2, time=MS * 5, x=0, y=0, z=-1, amp=3)]
    np.savez_compressed(HERE + '/chain_s2.npz',
                        **run_chain(ref, base_config(), make_instructions(rows), 202, pat, store_currents=False))

    # C: high-energy channels active (int(factor) = 20), uniform dummy maps
    rows = [dict(type=1, time=MS, x=0, y=0, z=-40, amp=2500), dict(type=2, time=MS, x=0, y=0, z=-40, amp=150),
            dict(type=1, time=3 * MS, x=20, y=0, z=-5, amp=700)]
    np.savez_compressed(HERE + '/chain_he.npz',
                        **run_chain(ref, base_config(high_energy_deamplification_factor=20),
                                    make_instructions(rows), 303, None))

    # D: noise on (synthetic noise array, 494 columns -> HE rows get no noise), short noise array wraps
    rng = np.random.default_rng(5)
    noise = np.round(rng.normal(0, 2.2, (3000, N_TPC))).astype(np.int16)
    np.savez_compressed(HERE + '/noise.npz', noise=noise)
    rows = [dict(type=1, time=MS, x=0, y=0, z=-40, amp=1500), dict(type=2, time=MS, x=0, y=0, z=-40, amp=200),
            dict(type=1, time=3 * MS, x=20, y=0, z=-5, amp=300), dict(type=2, time=5 * MS, x=20, y=0, z=-60, amp=80)]
    np.savez_compressed(HERE + '/chain_noise.npz',
                        **run_chain(ref, base_config(), make_instructions(rows), 404, pat, noise=noise))

    # E: PMT afterpulses on (synthetic CDF tables)
    ap = synthetic_afterpulse_tables(np.random.default_rng(6))
    np.savez_compressed(HERE + '/pmt_ap_tables.npz',
                        **{f'{k}_{q}': np.asarray(v) for k, d in ap.items() for q, v in d.items()})
    rows = [dict(type=1, time=MS, x=0, y=0, z=-40, amp=6000), dict(type=2, time=MS, x=5, y=5, z=-40, amp=300),
            dict(type=1, time=4 * MS, x=20, y=0, z=-5, amp=50)]
    np.savez_compressed(HERE + '/chain_pmt_ap.npz',
                        **run_chain(ref, base_config(), make_instructions(rows), 505, pat, ap=ap))


def params_overrides():
    """chain F: everything the digitiser / ZLE / pulse window code reads from the config at non-default values,
    non-uniform gains and three turned-off PMTs (shared with the tests through chain_params_config.json)"""
    rng = np.random.default_rng(77)
    gains = np.round(rng.uniform(1.0e6, 3.0e6, N_TPC))
    off = [5, 200, 300]
    gains[off] = 0
    return dict(gains=gains, turned_off_pmts=np.array(off), trigger_window=30, samples_to_store_before=20,
                samples_to_store_after=70, zle_threshold=25, special_thresholds={'7': 40, '310': 5},
                digitizer_reference_baseline=15000, right_raw_extension=30000)


def fixture_chain_params(ref):
    pat = dict(s1=SyntheticPatternMap(14e-5, 30.0, 18.0, 0.15), s2=SyntheticPatternMap(30e-5, 9.0, 25.0, 0.02))
    MS = 1_000_000
    ov = params_overrides()
    rows = [dict(type=1, time=MS, x=0, y=0, z=-40, amp=4000), dict(type=2, time=MS, x=4, y=-3, z=-40, amp=250),
            dict(type=1, time=MS + 50_000, x=-20, y=5, z=-70, amp=900),           # same cluster only with the default rext
            dict(type=1, time=3 * MS, x=20, y=0, z=-5, amp=12000), dict(type=2, time=4 * MS, x=-12, y=30, z=-80, amp=60)]
    np.savez_compressed(HERE + '/chain_params.npz', **run_chain(ref, base_config(**ov), make_instructions(rows), 606, pat))
    with open(HERE + '/chain_params_config.json', 'w') as f:
        json.dump({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in ov.items()}, f)


def geometry_overrides():
    """chain I: a digitiser with another sample duration and pulse template length (pulse.py:146-187 builds the templates for
    whatever the config says): 5 ns samples, 3 + 37 template samples, other stored / trigger windows"""
    return dict(sample_duration=5, samples_before_pulse_center=3, samples_after_pulse_center=37,
                samples_to_store_before=30, samples_to_store_after=40, trigger_window=40)


def fixture_chain_geometry(ref):
    pat = dict(s1=SyntheticPatternMap(14e-5, 30.0, 18.0, 0.15), s2=SyntheticPatternMap(30e-5, 9.0, 25.0, 0.02))
    MS = 1_000_000
    ov = geometry_overrides()
    rows = [dict(type=1, time=MS, x=0, y=0, z=-40, amp=3000), dict(type=2, time=MS, x=4, y=-3, z=-40, amp=200),
            dict(type=1, time=3 * MS, x=20, y=0, z=-5, amp=9000), dict(type=1, time=3 * MS + 300, x=-5, y=5, z=-15, amp=700),
            dict(type=2, time=4 * MS, x=-12, y=30, z=-80, amp=50)]
    ref.load_resource._cached_configs.clear()
    np.savez_compressed(HERE + '/chain_geometry.npz', **run_chain(ref, base_config(**ov), make_instructions(rows), 707, pat, store_currents=True))
    with open(HERE + '/chain_geometry_config.json', 'w') as f:
        json.dump(ov, f)


def fixture_chain_runsets(ref):
    """chain G: save_full_truth=False -- S1s within 100 ns and S2s within int(0.2 / v) ns of each other share one
    Pulse call and one truth row (rawdata.py:106-127, 364-372)"""
    pat = dict(s1=SyntheticPatternMap(14e-5, 30.0, 18.0, 0.15), s2=SyntheticPatternMap(30e-5, 9.0, 25.0, 0.02))
    MS = 1_000_000
    rows = [dict(type=1, time=MS, x=1, y=2, z=-10, amp=900), dict(type=1, time=MS + 50, x=3, y=-2, z=-12, amp=700),
            dict(type=1, time=MS + 120, x=-5, y=0, z=-11, amp=500), dict(type=1, time=MS + 400, x=9, y=9, z=-10, amp=1100),
            dict(type=2, time=MS, x=1, y=2, z=-10.0, amp=60), dict(type=2, time=MS + 50, x=3, y=-2, z=-10.1, amp=40),
            dict(type=2, time=MS + 120, x=-5, y=0, z=-10.5, amp=30),
            dict(type=1, time=3 * MS, x=0, y=0, z=-30, amp=2000), dict(type=2, time=3 * MS, x=0, y=0, z=-30, amp=100)]
    np.savez_compressed(HERE + '/chain_runsets.npz',
                        **run_chain(ref, base_config(save_full_truth=False), make_instructions(rows), 707, pat))


N_NVETO = 120


def optical_chain_overrides(case):
    """chains J: the 120-channel nVeto configuration of RawDataOptical (one dead PMT); shared with the tests through
    chain_optical_config.json.  'main' leaves nveto_time_max_cutoff out (rawdata.py:481: default int(1e6))"""
    gains = np.full(N_NVETO, 2e6)
    gains[7] = 0.0
    ov = dict(detector='XENONnT_neutron_veto', n_tpc_pmts=N_NVETO, n_top_pmts=0, gains=gains, channels_bottom=[],
              channel_map=dict(nveto=(2000, 2119), sum_signal=800, he=(500, 752)), right_raw_extension=2000)
    if case == 'cutoff':
        ov['nveto_time_max_cutoff'] = 5000
    return ov


def optical_chain_inputs(case):
    """instructions (_first / _last), flat channels and timings of the two optical chains"""
    rng = np.random.default_rng(dict(main=1201, cutoff=1202)[case])
    cutoff = optical_chain_overrides(case).get('nveto_time_max_cutoff', int(1e6))
    n = dict(main=200, cutoff=40)[case]
    # 1 us apart, with gaps above right_raw_extension: many clusters, some of several instructions
    gap = np.where(rng.random(n) < 0.3, rng.integers(2500, 9000, n), 1000)
    time = 1_000_000 + np.cumsum(gap)
    nph = rng.integers(0, 9, n)
    if case == 'main':
        time[61] = time[60]                                 # two instructions with the same time
        first_in_cluster = np.flatnonzero(gap > 2000)
        nph[[0, first_in_cluster[5], 100, n - 1]] = 0       # _first == _last: first of the stream / of a cluster, inside, last of the stream
        nph[[30, 150, n - 3]] = [4, 6, 8]
    else:
        nph[[3, n - 1]] = 0
        nph[[10, 20]] = [5, 7]
    ins = np.zeros(n, dtype=instruction_dtype + optical_extra_dtype)
    ins['type'], ins['time'], ins['event_number'], ins['amp'], ins['recoil'] = 1, time, np.arange(n), nph, 7
    ins['_last'] = np.cumsum(nph)
    ins['_first'] = ins['_last'] - nph
    tot = int(nph.sum())
    channels = rng.integers(0, N_NVETO, tot).astype(np.int64)
    channels[rng.random(tot) < 0.04] = 7                    # photons on the dead PMT
    if case == 'main':
        timings = rng.exponential(60, tot).astype(np.int64)
        timings[rng.random(tot) < 0.03] = -rng.integers(1, 400)
        timings[rng.random(tot) < 0.03] = cutoff + rng.integers(0, 5000)
        late = rng.random(tot) < 0.02                       # a few late photons: pulses that reach into later clusters
        timings[late] = rng.integers(1500, 12000, late.sum())
        a = int(ins['_first'][30]); timings[a:a + 4] = [-1, cutoff, 2 * cutoff, -300]          # every photon of this one is cut
        a = int(ins['_first'][150]); timings[a:a + 3] = [0, -1, 1]; channels[a:a + 3] = [11, 11, 7]
        # the far end of the accepted window, near the end of the stream (a pulse 1 ms late keeps the cache open behind it)
        a = int(ins['_first'][n - 3]); timings[a:a + 3] = [cutoff - 1, cutoff, cutoff + 1]; channels[a:a + 3] = [33, 33, 34]
    else:
        timings = rng.integers(-500, 2 * cutoff, tot).astype(np.int64)
        a = int(ins['_first'][10]); timings[a:a + 5] = [cutoff - 1, cutoff, cutoff + 1, 0, -1]
        a = int(ins['_first'][20]); timings[a:a + 3] = [4999, 5000, 4998]; channels[a:a + 3] = [50, 50, 50]
    return ins, channels, timings, cutoff


def fixture_chain_optical(ref):
    """chains J: RawDataOptical (rawdata.py:461-495) over optical instructions -- sim_primary's slicing, window mask, channel sort and
    event-time offset (the photon list on entry to Pulse.__call__: in_t / in_ch), then everything the other chains record"""
    cfgs = {}
    for case in ('main', 'cutoff'):
        ov = optical_chain_overrides(case)
        ins, channels, timings, cutoff = optical_chain_inputs(case)
        cfg = base_config(**ov)
        ref.load_resource._cached_configs.clear()
        ref.pulse._cached_pmt_current_templates.clear()
        ref.pulse._cached_uniform_to_pe_arr.clear()
        orig_get = ref.load_resource.straxen.get_resource
        # the nVeto Resource loads nv_pmt_qe, which only the Geant4 front end reads (strax_interface.py:253)
        ref.load_resource.straxen.get_resource = lambda path, fmt='text': ({} if fmt == 'json' else orig_get(path, fmt=fmt))
        try:
            rd = ref.rawdata.RawDataOptical(cfg, channels=channels, timings=timings)
        finally:
            ref.load_resource.straxen.get_resource = orig_get
        out = record_chain(ref, rd, ins, dict(main=1211, cutoff=1212)[case],
                           instruction_dtype + optical_extra_dtype + truth_extra_dtype + [('fill', bool)], store_entry=True)
        out.update(channels=channels, timings=timings, cutoff=np.int64(cutoff))
        name = 'chain_optical.npz' if case == 'main' else 'chain_optical_cutoff.npz'
        np.savez_compressed(HERE + '/' + name, **out)
        cfgs[case] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in ov.items()}
        print(case, len(out['call_kind']), 'calls', len(out['dg_left']), 'windows', len(out['in_t']), 'photons of', len(timings))
    with open(HERE + '/chain_optical_config.json', 'w') as f:
        json.dump(cfgs, f)


def window_edges_overrides(name):
    """the two configs of the designed-spacing fixtures (tests/window_edges.py), shared with the tests through window_edges_config.json:
    the optical chains' nVeto configuration and the bundled TPC one, both with pmt_transit_time_spread 0 -- the transit-time draw
    (pulse.py:53-56) is then the constant pmt_transit_time_mean"""
    return dict(optical_chain_overrides('main') if name == 'nveto' else {}, pmt_transit_time_spread=0)


def fixture_window_edges(ref):
    """window_edges.npz / window_edges_tpc.npz: RawDataOptical (rawdata.py:24-157, 461-495) over instruction streams whose every
    digitise decision is designed to the ns (tests/window_edges.py holds the case table).  Recorded like the optical chains, plus
    flush_at_call: the number of Pulse calls made whenever RawData.__call__ entered digitize_pulse_cache -- the reference's verdict on
    every decision, empty caches included.  Asserted here: the recorded photon times are timings + instruction time +
    pmt_transit_time_mean, every recorded pulse has the bounds the case table predicts, every decision got the verdict in `expect`,
    and the windows are the predicted ones."""
    from tests import window_edges as WE
    cfgs = {}
    for name in ('nveto', 'tpc'):
        ov = window_edges_overrides(name)
        cfg = base_config(**ov)
        s = WE.CASES[name](cfg)
        ins, channels, timings = s.inputs()
        ref.load_resource._cached_configs.clear()
        ref.pulse._cached_pmt_current_templates.clear()
        ref.pulse._cached_uniform_to_pe_arr.clear()
        orig_get = ref.load_resource.straxen.get_resource
        if name == 'nveto':         # (nv_pmt_qe, as in fixture_chain_optical)
            ref.load_resource.straxen.get_resource = lambda path, fmt='text': ({} if fmt == 'json' else orig_get(path, fmt=fmt))
        try:
            rd = ref.rawdata.RawDataOptical(cfg, channels=channels, timings=timings)
        finally:
            ref.load_resource.straxen.get_resource = orig_get
        n_calls, flush_at = [0], []
        sim_primary = rd.sim_primary

        def counted_sim_primary(*a, **k):
            n_calls[0] += 1
            return sim_primary(*a, **k)

        def counted_digitize():
            flush_at.append(n_calls[0])
            return type(rd).digitize_pulse_cache(rd)         # (the Recorder's, looked up when called)
        rd.sim_primary, rd.digitize_pulse_cache = counted_sim_primary, counted_digitize
        out = record_chain(ref, rd, ins, dict(nveto=1221, tpc=1222)[name],
                           instruction_dtype + optical_extra_dtype + truth_extra_dtype + [('fill', bool)], store_entry=True)
        for k in ('dg_sum_min', 'dg_sum_total'):
            out.pop(k, None)
        cutoff = cfg.get('nveto_time_max_cutoff', int(1e6))
        out.update(channels=channels, timings=timings, cutoff=np.int64(cutoff), flush_at_call=np.array(flush_at, dtype=np.int64))
        out.update(s.table())
        # ---- the three assertions of the generator
        n = len(ins)
        assert len(out['call_kind']) == n == n_calls[0] and flush_at[-1] == n         # one call per instruction, in input order; the last digitise
        ttm = int(cfg['pmt_transit_time_mean'])
        for k in range(n):
            a, b = int(ins['_first'][k]), int(ins['_last'][k])
            keep = (timings[a:b] >= 0) & (timings[a:b] < cutoff)
            want = sorted(zip(channels[a:b][keep].tolist(), (timings[a:b][keep] + ins['time'][k] + ttm).tolist()))
            c, e = int(out['call_ph_off'][k]), int(out['call_ph_off'][k + 1])
            assert sorted(zip(out['ph_ch'][c:e].tolist(), out['ph_t'][c:e].tolist())) == want, ('photon times of call', k)
        off, pch, pl, pr = s.predicted_pulses()
        assert np.array_equal(out['call_pulse_off'], off) and np.array_equal(out['pl_ch'], pch), 'pulses per call'
        assert np.array_equal(out['pl_left'], pl) and np.array_equal(out['pl_right'], pr), 'pulse bounds'
        verdict = np.isin(out['dec_first'], out['flush_at_call'][:-1])
        wrong = np.flatnonzero(verdict != out['dec_expect'])
        assert len(wrong) == 0, ('the reference disagrees with expect at clusters', wrong.tolist(), [s.clusters[i] for i in wrong])
        assert set(out['flush_at_call'][:-1].tolist()) <= set(out['dec_first'].tolist())
        wl, wr = s.predicted_windows()
        assert np.array_equal(out['dg_left'], wl) and np.array_equal(out['dg_right'], wr), 'windows'
        fname = WE.FIXTURES[name]
        np.savez_compressed(HERE + '/' + fname, **out)
        cfgs[name] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in ov.items()}
        designed = out['dec_has_delta']
        print(fname, n, 'instructions', len(out['dec_first']), 'decisions', int(designed.sum()), 'designed', len(out['dg_left']), 'windows',
              len(out['zle_ch']), 'ZLE tuples', os.path.getsize(HERE + '/' + fname), 'bytes')
    with open(HERE + '/window_edges_config.json', 'w') as f:
        json.dump(cfgs, f)


# the probability columns of pmt_ap_tables.npz scaled up for the draw fixture (and, through the fixture, for the tests that
# compare with it): ~10 % afterpulses per parent and element instead of ~1 %, so that 10^5s of afterpulses need 10^6 parents,
# not 10^7.  For 'Uniform' the column is also the upper end of the delay (afterpulse.py:213-216): delays U(48, 96) ns.
# 'Uniform_hi': P = 0.3, with pmt_ap_modifier 1.8 a double-PE parent always makes one (P * modifier * 2 > 1)
PMT_AP_SCALE = dict(He=5.0, Xe=8.0, Uniform=12.0, Uniform_hi=37.5)
PMT_AP_T_MODIFIER = 3


def fixture_pmt_ap_draws(ref):
    """Draws of the reference's PMT_Afterpulse.photon_afterpulse (afterpulse.py:172-249), a static method, on plain objects: per
    element alone (a one-element table) and pmt_ap_modifier, parents on all 494 channels at time 0 (the returned time is the
    delay), double-PE fraction p_double_pe_emision, non-uniform gains, pmt_ap_t_modifier 3.  Stored as COUNTS: parents per
    channel (single / double PE), afterpulses per channel, histograms over the delay bin index (Uniform: over the delay in whole
    ns) and the amplitude bin index, for He the joint delay x amplitude table coarsened to 20 x 20; one call with all elements."""
    import types
    tab = np.load(HERE + '/pmt_ap_tables.npz')
    cfg0 = base_config()
    p_dpe = float(cfg0['p_double_pe_emision'])
    gains = np.round(np.random.default_rng(31).uniform(1.0e6, 3.0e6, N_TPC))

    def tables(name, scale):
        el = name.split('_')[0]
        return {el: dict(delaytime_cdf=tab[f'{el}_delaytime_cdf'] * scale, amplitude_cdf=tab[f'{el}_amplitude_cdf'],
                         delaytime_bin_size=float(tab[f'{el}_delaytime_bin_size']), amplitude_bin_size=float(tab[f'{el}_amplitude_bin_size']))}

    def draw(uniform_to_pmt_ap, modifier, n_min, rng, chunk=2_000_000, max_chunks=200):
        config = dict(pmt_ap_modifier=modifier, pmt_ap_t_modifier=PMT_AP_T_MODIFIER, gains=gains)
        resource = types.SimpleNamespace(uniform_to_pmt_ap=uniform_to_pmt_ap)
        single, double = np.zeros(N_TPC, np.int64), np.zeros(N_TPC, np.int64)
        out, n, ordered = [], 0, True
        for _ in range(max_chunks):
            ch = rng.integers(0, N_TPC, chunk)
            dpe = rng.random(chunk) < p_dpe
            single += np.bincount(ch[~dpe], minlength=N_TPC); double += np.bincount(ch[dpe], minlength=N_TPC)
            parent = types.SimpleNamespace(_photon_timings=np.zeros(chunk, np.int64), _photon_channels=ch, _photon_is_dpe=dpe)
            t, c, g = ref.afterpulse.PMT_Afterpulse.photon_afterpulse(parent, resource, config)
            ordered &= bool(np.all(np.diff(c) >= 0))
            out.append((np.asarray(t, np.float64), np.asarray(c, np.int64), np.asarray(g, np.float64)))
            n += len(t)
            if n >= n_min:
                break
        assert n >= n_min
        t, c, g = (np.concatenate([o[k] for o in out]) for k in range(3))
        return single, double, t, c, g, ordered

    out = dict(p_dpe=np.float64(p_dpe), gains=gains, t_modifier=np.int64(PMT_AP_T_MODIFIER),
               **{f'scale_{k}': np.float64(v) for k, v in PMT_AP_SCALE.items()})
    cases = [(el, m) for el in ('He', 'Xe', 'Uniform') for m in (0.6, 1.0, 1.8)] + [('Uniform_hi', 1.8)]
    names = []
    np.random.seed(1301)                                  # photon_afterpulse draws from numpy's global generator
    rng = np.random.default_rng(1302)                     # the parents
    for name, m in cases:
        el = name.split('_')[0]
        case = f'{name}_m{int(round(m * 10)):02d}'
        names.append(case)
        T = tables(name, PMT_AP_SCALE[name])
        single, double, t, c, g, ordered = draw(T, m, 400_000, rng)
        assert ordered
        out[f'{case}_par_single'], out[f'{case}_par_double'] = single, double
        out[f'{case}_ap_ch'] = np.bincount(c, minlength=N_TPC).astype(np.int64)
        if el == 'Uniform':
            dbin = np.floor(t).astype(np.int64)          # Pulse.add_current receives the times .astype(int64) (pulse.py:130)
            abin = np.rint(g / gains[c]).astype(np.int64)
            out[f'{case}_delay'] = np.bincount(dbin, minlength=512).astype(np.int64)
            out[f'{case}_amp'] = np.bincount(abin, minlength=4).astype(np.int64)
        else:
            dbin = np.rint((t + PMT_AP_T_MODIFIER) / T[el]['delaytime_bin_size']).astype(np.int64)
            abin = np.rint(g / gains[c] / T[el]['amplitude_bin_size']).astype(np.int64)
            assert np.allclose(dbin * T[el]['delaytime_bin_size'] - PMT_AP_T_MODIFIER, t) and dbin.min() >= 0 and dbin.max() < 200
            assert np.allclose(abin * T[el]['amplitude_bin_size'] * gains[c], g, rtol=1e-9) and abin.max() < 100
            out[f'{case}_delay'] = np.bincount(dbin, minlength=200).astype(np.int64)
            out[f'{case}_amp'] = np.bincount(abin, minlength=100).astype(np.int64)
            if el == 'He':
                joint = np.zeros((20, 20), np.int64)
                np.add.at(joint, (dbin // 10, abin // 5), 1)
                out[f'{case}_joint'] = joint
        print(case, 'parents', int(single.sum() + double.sum()), 'afterpulses', len(t))
    # all elements in one call: the output is sorted by channel and the elements add
    T = {}
    for el in ('He', 'Xe', 'Uniform'):
        T.update(tables(el, PMT_AP_SCALE[el]))
    single, double, t, c, g, ordered = draw(T, 1.0, 400_000, rng)
    names.append('all_m10')
    out['all_m10_par_single'], out['all_m10_par_double'] = single, double
    out['all_m10_ap_ch'] = np.bincount(c, minlength=N_TPC).astype(np.int64)
    out['all_m10_channel_sorted'] = np.bool_(ordered)
    print('all_m10', 'parents', int(single.sum() + double.sum()), 'afterpulses', len(t))
    out['cases'] = np.array(names)
    np.savez_compressed(HERE + '/pmt_ap_draws.npz', **out)


def pulse_edges_geometry_overrides():
    """the geometry of chain I; the stored samples and the trigger window stay those of the bundled configuration"""
    return dict(sample_duration=5, samples_before_pulse_center=3, samples_after_pulse_center=37)


def run_pulse_edges(ref, config, builder, seed):
    """The reference below the photon generators: per case one Pulse.__call__ with preassigned gains (pulse.py:53 skips the transit-time
    draw, pulse.py:105-107 takes the gains as given), its _pulses handed to a RawData's _pulses_cache, and per group one
    digitize_pulse_cache() + ZLE() (rawdata.py:204-311), all under the Recorder.  Returns the flat arrays of record_chain plus the
    explicit pulse sets (set_cluster, set_tmin), the case / group names and the call -> case / group indices."""
    ref.load_resource._cached_configs.clear()
    ref.pulse._cached_pmt_current_templates.clear()
    ref.pulse._cached_uniform_to_pe_arr.clear()
    config = dict(config, enable_noise=False)
    pulse = ref.pulse.Pulse(config)
    rd = ref.rawdata.RawData(config)
    rd._pulses_cache = []
    rng = np.random.default_rng(seed)
    rec = Recorder(ref)
    rec.install()
    np.random.seed(seed)          # (Pulse.__call__ still draws the double-PE flags, which a call with preassigned gains never reads)
    try:
        for gi in range(len(builder.groups)):
            for case in builder.cases:
                if case['group'] != gi:
                    continue
                t, ch, g = [], [], []
                for times, gains, channel in case['tiles']:
                    if gains is None:
                        gains = rng.uniform(1e6, 3e6, len(times))
                    elif callable(gains):
                        gains = gains(rng, times)
                    t.append(times); ch.append(np.full(len(times), channel, dtype=np.int64)); g.append(np.asarray(gains, dtype=np.float64))
                pulse._photon_timings = np.concatenate(t).astype(np.int64)
                pulse._photon_channels = np.concatenate(ch)
                pulse._photon_gains = np.concatenate(g)
                assert np.all(np.diff(pulse._photon_channels) >= 0)
                pulse()
                rd._pulses_cache += pulse._pulses
            rd.digitize_pulse_cache()
            for c, left, right, data in rd.ZLE():
                rec.zle.append((len(rec.digits) - 1, int(c), int(left), int(right), np.array(data, dtype=np.int64)))
    finally:
        rec.uninstall()
    assert len(rec.digits) == len(builder.groups)
    out = dict(seed=np.int64(seed))
    flatten_recorder(rec, out, store_currents=True)
    out['set_cluster'] = np.array([c['group'] for c in builder.cases], dtype=np.int32)
    out['set_tmin'] = np.array([c['set_tmin'] for c in builder.cases], dtype=np.int64)
    out['case_names'] = np.array([c['name'] for c in builder.cases])
    out['call_case'] = np.arange(len(builder.cases), dtype=np.int32)
    out['group_names'] = np.array(builder.groups)
    out['call_group'] = out['set_cluster'].copy()
    return out, pulse


def fixture_pulse_edges(ref):
    """pulse_edges.npz / pulse_edges_geometry.npz: the reference on photon lists designed to sit on every boundary of the HIP pulse
    kernels (tests/pulse_edges.py holds the case table).  No sample of any pulse may lie near a rounding tie (exact rational
    arithmetic, tests/pulse_edges.py: fixture_exact): the random gains are redrawn with the next seed until none is within 4 B."""
    from fractions import Fraction
    from tests import pulse_edges as PE
    for name, overrides, make_cases, seed0 in [('pulse_edges.npz', {}, PE.main_cases, 5101),
                                               ('pulse_edges_geometry.npz', pulse_edges_geometry_overrides(), PE.geometry_cases, 5201)]:
        cfg = base_config(**overrides)
        ref.load_resource._cached_configs.clear()
        ref.pulse._cached_pmt_current_templates.clear()
        p = ref.pulse.Pulse(dict(cfg))
        dt = int(cfg['sample_duration'])
        templates, c2a = np.array(p._pmt_current_templates), float(p.current_2_adc)
        ties = PE.find_ties(templates, c2a)
        assert set(ties) == {'even', 'odd'}, ties
        thr_gain = PE.truth_threshold_gain(p.current_max, c2a, cfg['zle_threshold'])
        for seed in range(seed0, seed0 + 20):
            builder = make_cases(thr_gain, ties)
            out, pulse = run_pulse_edges(ref, cfg, builder, seed)
            exact = PE.fixture_exact(out, templates, c2a, dt)
            # the designed ties: the peak sample of the two single-photon pulses
            names = [str(out['case_names'][k]) for k in out['call_case']]
            skip, tie_pulse, tie_sample, tie_k = set(), [], [], []
            for kind in ('even', 'odd'):
                j = int(out['call_pulse_off'][names.index('e_tie_' + kind)])
                cur = out['pl_current'][out['pl_cur_off'][j]:out['pl_cur_off'][j + 1]]
                s = int(np.argmax(cur))
                assert cur[s] * np.float64(c2a) == ties[kind][0] + 0.5 and exact[j]['dist'][s] < Fraction(1, 10 ** 9)
                skip.add((j, s)); tie_pulse.append(j); tie_sample.append(s); tie_k.append(ties[kind][0])
            bad, ratio, dist = PE.near_ties(exact, skip)
            print(name, 'seed', seed, 'near ties', len(bad), 'smallest distance', float(dist), '= %.3g B' % float(ratio))
            if not bad:
                break
        else:
            raise RuntimeError('no seed without a near tie')
        out['min_tie_distance'] = np.float64(float(dist))
        out['min_tie_distance_over_B'] = np.float64(float(ratio))
        out['tie_pulse'], out['tie_sample'], out['tie_k'] = (np.array(x, dtype=np.int64) for x in (tie_pulse, tie_sample, tie_k))
        out['templates'], out['current_2_adc'] = templates, np.float64(c2a)
        np.savez_compressed(HERE + '/' + name, **out)
        print(name, len(out['call_kind']), 'calls', len(out['pl_ch']), 'pulses', len(out['ph_t']), 'photons', len(out['dg_left']), 'windows')
    with open(HERE + '/pulse_edges_geometry_config.json', 'w') as f:
        json.dump(pulse_edges_geometry_overrides(), f)


def run_zle_edges(ref, config, fam, seed):
    """run_pulse_edges' route with the noise on: per case one Pulse.__call__ with preassigned gains, per window one
    digitize_pulse_cache() + ZLE() under the Recorder, which hands the window's designed ix_rand to add_noise in place of the draw (and
    asserts it is below the `high` the reference passed).  The designed table is installed as run_chain installs noise=."""
    ref.load_resource._cached_configs.clear()
    ref.pulse._cached_pmt_current_templates.clear()
    ref.pulse._cached_uniform_to_pe_arr.clear()
    path = TMP + '/noise_zle_edges.npz'
    np.savez(path, arr_0=fam.table())
    config = dict(config, noise_file=path, enable_noise=True)
    pulse = ref.pulse.Pulse(config)
    rd = ref.rawdata.RawData(config)
    assert rd.resource.noise_data.shape == (fam.N, fam.columns) and np.array_equal(rd.resource.noise_data, fam.table())
    rd._pulses_cache = []
    rec = Recorder(ref)
    rec.designed_ix = fam.ix_rands()
    rec.install()
    np.random.seed(seed)
    c2a = None
    try:
        for w in fam.windows:
            for ci in w['cases']:
                case = fam.cases[ci]
                pulse._photon_timings = case['times'].copy()
                pulse._photon_channels = np.full(len(case['times']), case['channel'], dtype=np.int64)
                pulse._photon_gains = case['gains'].copy()
                pulse()
                assert len(pulse._pulses) == 1
                # no sample of a designed pulse near a rounding tie: either arithmetic form rounds it like the reference
                x = np.abs(pulse._pulses[0]['current'] * pulse.current_2_adc)
                assert np.all(np.abs(x - np.floor(x) - 0.5) > 1e-6 * np.maximum(x, 1.0)), case['name']
                rd._pulses_cache += pulse._pulses
            rd.digitize_pulse_cache()
            for c, left, right, data in rd.ZLE():
                rec.zle.append((len(rec.digits) - 1, int(c), int(left), int(right), np.array(data, dtype=np.int64)))
    finally:
        rec.uninstall()
    assert len(rec.digits) == len(fam.windows)
    out = {}
    flatten_recorder(rec, out)
    assert np.array_equal(out['dg_ix_rand'], fam.ix_rands()), (out['dg_ix_rand'], fam.ix_rands())
    order = [ci for w in fam.windows for ci in w['cases']]
    out['set_cluster'] = np.array([fam.cases[ci]['window'] for ci in order], dtype=np.int32)
    out['set_tmin'] = np.array([int(fam.cases[ci]['times'].min()) for ci in order], dtype=np.int64)
    out['call_case'] = np.array(order, dtype=np.int32)
    out['case_names'] = np.array([c['name'] for c in fam.cases])
    out['noise_shape'] = np.array([fam.N, fam.columns], dtype=np.int64)
    for k in [k for k in out if k.startswith('call_truth_')] + ['e_t', 'call_e_off', 'dg_sum_min', 'dg_sum_total']:
        del out[k]              # (the truth of the designed photons and the sum row are not what this fixture is about)
    return out


def fixture_zle_edges(ref):
    """zle_edges.npz: the reference on rows designed sample by sample through the noise table (tests/zle_edges.py holds the case
    table): per family (a configuration and a table) the flatten_recorder layout under '<family>/<name>'"""
    from tests import zle_edges as ZE
    tab = np.load(HERE + '/tables.npz')
    templates, c2a = tab['templates'], float(tab['current_2_adc'])
    out, cfgs = dict(families=np.array(ZE.FAMILIES)), {}
    for i, name in enumerate(ZE.FAMILIES):
        cfgs[name] = ZE.overrides(name)
        cfg = base_config(**cfgs[name])
        fam = ZE.family(name, cfg, templates, c2a)
        r = run_zle_edges(ref, cfg, fam, 6100 + i)
        for k, v in r.items():
            out[f'{name}/{k}'] = v
        print(name, 'windows', len(fam.windows), 'rows', len(r['row_ch']), 'samples', len(r['row_data']), 'intervals', len(r['zle_ch']),
              'table', (fam.N, fam.columns))
    np.savez_compressed(HERE + '/zle_edges.npz', **out)
    with open(HERE + '/zle_edges_config.json', 'w') as f:
        json.dump(cfgs, f, indent=0, sort_keys=True)


def run_spe_channels(ref, family, seed):
    """run_pulse_edges' route with the gains left to the reference: per case one Pulse.__call__ on a designed photon list WITHOUT
    _photon_gains (pulse.py:53-56 draws the transit times, :97-103 the gains through uniform_to_pe_arr(p, channel)), per group one
    digitize_pulse_cache() + ZLE(), all under the Recorder.  The columns go in as a CSV, as a real SPE file does.  Returns the flat
    arrays, the reference's table and the charge axis as the reference parsed it."""
    from tests import spe_channels as SC
    csv = SC.write_csv(family, TMP + f'/spe_channels_{family}.csv', SC.N_WIDE)
    csv494 = SC.write_csv(family, TMP + f'/spe_channels_{family}_494.csv', SC.N_TPC)
    tables, pulses = {}, {}
    for key, path, p_dpe in [('wide', csv, None), ('tpc', csv494, None), ('dpe', csv494, SC.P_DPE_HIGH)]:
        ref.load_resource._cached_configs.clear()
        ref.pulse._cached_pmt_current_templates.clear()
        ref.pulse._cached_uniform_to_pe_arr.clear()
        config = base_config(photon_area_distribution=path, gains=SC.gains(N_TPC), enable_noise=False)
        if p_dpe is not None:
            config['p_double_pe_emision'] = p_dpe
        pulses[key] = ref.pulse.Pulse(config)
        tables[key] = np.array(pulses[key]._Pulse__uniform_to_pe_arr)
        shapes = pulses[key].resource.photon_area_distribution
        charge = shapes['charge'].values.astype(np.float64)
        parsed = np.stack([shapes[k].values.astype(np.float64) for k in shapes.columns[1:]])
        # the rule rebuilds the columns the reference read; the charge axis comes back from the CSV an ulp off on a few bins and is stored as parsed
        assert np.array_equal(parsed, SC.pdfs(family, len(parsed))) and np.allclose(charge, SC.charge_axis()[0], rtol=1e-15, atol=0)
    assert tables['wide'].shape == (SC.N_WIDE, SC.N_GRID) and np.array_equal(tables['wide'][:N_TPC], tables['tpc'])
    assert np.array_equal(tables['dpe'], tables['tpc'])
    SC.assert_design(family, SC.pdfs(family, SC.N_WIDE), tables['wide'], charge)
    rd = ref.rawdata.RawData(dict(pulses['tpc'].config))
    rd._pulses_cache = []
    rec = Recorder(ref)
    rec.install()
    np.random.seed(seed)
    cases = SC.reference_cases(N_TPC, int(pulses['tpc'].config.get('sample_duration', 10)))
    try:
        for gi in range(len(SC.GROUPS)):
            for case in cases:
                if case['group'] != gi:
                    continue
                pulse = pulses['tpc' if case['p_dpe'] is None else 'dpe']
                pulse.__dict__.pop('_photon_gains', None)
                pulse._photon_timings = np.concatenate([t for t, _, _ in case['tiles']]).astype(np.int64)
                pulse._photon_channels = np.concatenate([np.full(len(t), c, dtype=np.int64) for t, _, c in case['tiles']])
                assert np.all(np.diff(pulse._photon_channels) >= 0)
                pulse()
                assert not rec.calls[-1]['has_gains']
                rd._pulses_cache += pulse._pulses
            rd.digitize_pulse_cache()
            for c, left, right, data in rd.ZLE():
                rec.zle.append((len(rec.digits) - 1, int(c), int(left), int(right), np.array(data, dtype=np.int64)))
    finally:
        rec.uninstall()
    assert len(rec.digits) == len(SC.GROUPS)
    out = dict(seed=np.int64(seed))
    flatten_recorder(rec, out)
    out['set_cluster'] = np.array([c['group'] for c in cases], dtype=np.int32)
    out['set_tmin'] = np.array([int(out['ph_t'][a:b].min()) for a, b in zip(out['call_ph_off'][:-1], out['call_ph_off'][1:])], dtype=np.int64)
    out['case_names'] = np.array([c['name'] for c in cases])
    out['call_case'] = np.arange(len(cases), dtype=np.int32)
    out['group_names'] = np.array(SC.GROUPS)
    out['call_group'] = out['set_cluster'].copy()
    out['call_p_dpe'] = np.array([float(pulses['tpc' if c['p_dpe'] is None else 'dpe'].config['p_double_pe_emision']) for c in cases])
    for k in ['e_t', 'call_e_off', 'dg_sum_min', 'dg_sum_total']:
        del out[k]
    # the design, on what the reference did: every channel hit, the marked ones at least 50 times, double PEs plentiful
    hit = np.bincount(out['ph_ch'], minlength=N_TPC)
    assert hit.min() >= 1 and all(hit[c] >= 50 for c in SC.SPECIAL + SC.EDGE_CHANNELS)
    a, b = out['call_ph_off'][-2:]
    assert out['ph_dpe'][a:b].mean() > 0.5 and out['ph_dpe'][:a].any()
    out['table'] = tables['wide']
    out['charge'] = charge
    return out


def fixture_spe_channels(ref):
    """spe_channels.npz: per family of per-channel SPE columns (tests/spe_channels.py) the reference's table for 500 columns and its
    Pulse calls on designed photon lists with the gains drawn by the reference, under '<family>/<name>'"""
    from tests import spe_channels as SC
    out = dict(families=np.array(SC.FAMILIES))
    for i, family in enumerate(SC.FAMILIES):
        r = run_spe_channels(ref, family, 7100 + i)
        for k, v in r.items():
            out[f'{family}/{k}'] = v
        print(family, 'calls', len(r['call_kind']), 'photons', len(r['ph_t']), 'double PE', int(r['ph_dpe'].sum()), 'channels hit',
              len(np.unique(r['ph_ch'])), 'pulses', len(r['pl_ch']), 'rows', len(r['row_ch']), 'intervals', len(r['zle_ch']))
    np.savez_compressed(HERE + '/spe_channels.npz', **out)
    with open(HERE + '/spe_channels_config.json', 'w') as f:
        json.dump(dict(gains=SC.gains(N_TPC).tolist(), p_double_pe_emision_high=SC.P_DPE_HIGH, n_columns=SC.N_WIDE,
                       special_columns=dict(zero=SC.ZERO_CH, first_positive_bin=SC.FIRST_CH, last_bin=SC.LAST_CH, gain_zero=SC.DEAD_CH)),
                  f, indent=0, sort_keys=True)


class StubDelayHist:
    """stand-in for the multihist.Hist1d the reference loads as uniform_to_ele_ap (private resource): the members
    afterpulse.py touches -- n, bin_centers, get_random (bin by content, uniform inside the bin)"""

    def __init__(self, histogram, bin_edges):
        self.histogram, self.bin_edges = np.asarray(histogram, float), np.asarray(bin_edges, float)
        self.bin_centers = 0.5 * (self.bin_edges[1:] + self.bin_edges[:-1])
        self.n = self.histogram.sum()

    def get_random(self, size):
        i = np.random.choice(len(self.bin_centers), size=size, p=self.histogram / self.n)
        return self.bin_centers[i] + np.random.uniform(-0.5, 0.5, size) * np.diff(self.bin_edges)[i]


def fixture_chain_electron_ap(ref):
    """chain H: enable_electron_afterpulses -- every S2 queues photo-ionisation electron instructions (type 4,
    afterpulse.py:14-91) that the scheduler feeds back (rawdata.py:133-145); all type-4 instructions of a cluster
    share one Pulse call.  The generated secondaries are stored with the chain."""
    pat = dict(s1=SyntheticPatternMap(14e-5, 30.0, 18.0, 0.15), s2=SyntheticPatternMap(30e-5, 9.0, 25.0, 0.02))
    MS = 1_000_000
    edges = np.linspace(0, 700e3, 141)
    h = np.exp(-np.arange(140) / 30.0); h *= 4e-3 / h.sum()
    np.savez_compressed(HERE + '/ele_ap_hist.npz', histogram=h, bin_edges=edges)
    rows = [dict(type=1, time=MS, x=0, y=0, z=-20, amp=2000), dict(type=2, time=MS, x=0, y=0, z=-20, amp=300),
            dict(type=2, time=MS + 450_000, x=5, y=-3, z=-60, amp=400),      # inside the first S2's afterpulse range
            dict(type=1, time=4 * MS, x=5, y=-3, z=-61, amp=900), dict(type=2, time=6 * MS, x=-9, y=4, z=-5, amp=150)]
    np.savez_compressed(HERE + '/chain_ele_ap.npz',
                        **run_chain(ref, base_config(), make_instructions(rows), 808, pat, ele_ap=StubDelayHist(h, edges)))


def run_chunker(ref, config, instructions, seed, pattern_maps=None, record_buffer_length=None, ele_ap=None):
    """The reference's ChunkRawRecords (strax_interface.py:354-504) around the reference's RawData: records the stream the
    generator hands to the chunker -- every yielded (channel, left, right, data) with rawdata.left / .right at that moment,
    every truth row with the position in the stream where it was written -- and every chunk the chunker yields (bounds,
    the records of each data type by FIELD, the truth rows)."""
    config = dict(config)
    ref.load_resource._cached_configs.clear()
    ref.pulse._cached_pmt_current_templates.clear()
    ref.pulse._cached_uniform_to_pe_arr.clear()
    si = ref.strax_interface
    log = dict(pulses=[], truth_at=[], truth_rows=[])

    class RecordingRawData(ref.rawdata.RawData):
        def __call__(self, instructions, truth_buffer=None, **kwargs):
            for tup in super().__call__(instructions, truth_buffer=truth_buffer, progress_bar=False):
                ch, left, right, data = tup
                log['pulses'].append((int(ch), int(left), int(right), np.array(data, dtype=np.int64), int(self.left), int(self.right)))
                yield tup

        def get_truth(self, instruction, truth_buffer):
            before = truth_buffer['fill'].copy()
            super().get_truth(instruction, truth_buffer)
            new = np.flatnonzero(truth_buffer['fill'] & ~before)
            for ix in new:
                log['truth_at'].append(len(log['pulses']))          # written before this pulse of the stream is yielded
                log['truth_rows'].append(truth_buffer[ix].copy())

    if ele_ap is not None:
        config['enable_electron_afterpulses'] = True
        config['ele_ap_pdfs'] = ''
        orig_get = ref.load_resource.straxen.get_resource
        ref.load_resource.straxen.get_resource = lambda path, fmt='text': (ele_ap if fmt in ('dill', 'pkl.gz') else orig_get(path, fmt=fmt))
    try:
        sim = si.ChunkRawRecords(config, rawdata_generator=RecordingRawData)
    finally:
        if ele_ap is not None:
            ref.load_resource.straxen.get_resource = orig_get
    if ele_ap is not None:
        sim.rawdata.resource.uniform_to_ele_ap = ele_ap
    if pattern_maps is not None:
        sim.rawdata.resource.s1_pattern_map = pattern_maps['s1']
        sim.rawdata.resource.s2_pattern_map = pattern_maps['s2']
    if record_buffer_length is not None:
        sim.record_buffer = np.zeros(record_buffer_length, dtype=sim.record_buffer.dtype)
    np.random.seed(seed)
    chunks = []
    for res in sim(instructions):
        chunks.append(dict(pre=int(sim.chunk_time_pre), end=int(sim.chunk_time),
                           **{k: np.array(v) for k, v in res.items()}))
    out = dict(instructions=instructions, seed=np.int64(seed), record_buffer_length=np.int64(len(sim.record_buffer)),
               source_finished=np.bool_(sim.source_finished()))
    P = log['pulses']
    out['p_ch'] = np.array([q[0] for q in P], dtype=np.int16); out['p_left'] = np.array([q[1] for q in P], dtype=np.int64)
    out['p_right'] = np.array([q[2] for q in P], dtype=np.int64)
    out['p_data_off'] = np.concatenate([[0], np.cumsum([len(q[3]) for q in P])]).astype(np.int64)
    out['p_data'] = np.concatenate([q[3] for q in P] + [np.zeros(0, np.int64)]).astype(np.int32)
    out['p_gen_left'] = np.array([q[4] for q in P], dtype=np.int64); out['p_gen_right'] = np.array([q[5] for q in P], dtype=np.int64)
    out['t_at'] = np.array(log['truth_at'], dtype=np.int64)
    trows = np.array(log['truth_rows']) if log['truth_rows'] else np.zeros(0, dtype=sim.truth_buffer.dtype)
    for name in trows.dtype.names:
        if name != 'fill':
            out['t_' + name] = trows[name]
    out['c_pre'] = np.array([c['pre'] for c in chunks], dtype=np.int64); out['c_end'] = np.array([c['end'] for c in chunks], dtype=np.int64)
    for kind in ('raw_records', 'raw_records_he', 'raw_records_aqmon'):
        recs = [c[kind] for c in chunks if kind in c]
        if not recs:
            continue
        out[f'c_{kind}_off'] = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
        allr = np.concatenate(recs)
        for f in ('time', 'length', 'dt', 'channel', 'pulse_length', 'record_i', 'baseline'):
            out[f'c_{kind}_{f}'] = allr[f]
        out[f'c_{kind}_data_sum'] = allr['data'].astype(np.int64).sum(axis=1) if len(allr) else np.zeros(0, np.int64)
        out[f'c_{kind}_data_head'] = allr['data'][:, :8].astype(np.int32) if len(allr) else np.zeros((0, 8), np.int32)
    tr = [c['truth'] for c in chunks]
    out['c_truth_off'] = np.concatenate([[0], np.cumsum([len(t) for t in tr])]).astype(np.int64)
    allt = np.concatenate(tr)
    for name in allt.dtype.names:
        out['c_truth_' + name] = allt[name]
    return out


def fixture_chunker(ref):
    """golden chains for the chunker (reference ChunkRawRecords): several chunks; a chunk closing inside an event
    (strax_interface.py:400-404); a record buffer smaller than the run (flush :409-418 and skipped pulses :420-422);
    electron afterpulses (secondaries fed back while chunks close)."""
    pat = dict(s1=SyntheticPatternMap(14e-5, 30.0, 18.0, 0.15), s2=SyntheticPatternMap(30e-5, 9.0, 25.0, 0.02))
    MS = 1_000_000
    rng = np.random.default_rng(77)
    # A: 14 S1 + S2 pairs over 21 ms, 4 ms chunks
    rows = []
    for i in range(14):
        t = int(MS * (1 + 1.5 * i) + rng.integers(0, 200_000))
        x, y, z = rng.uniform(-25, 25), rng.uniform(-25, 25), -rng.uniform(2, 90)
        rows += [dict(type=1, time=t, x=x, y=y, z=z, amp=int(rng.choice([300, 1200, 4000]))),
                 dict(type=2, time=t, x=x, y=y, z=z, amp=int(rng.choice([20, 90, 300])))]
    np.savez_compressed(HERE + '/chunker_multi.npz', **run_chunker(ref, base_config(chunk_size=0.004), make_instructions(rows), 901, pat))
    # B: chunk boundaries inside events: S2s 0.45 ms apart chain the clusters' windows over several 1 ms chunks
    rows = [dict(type=2, time=MS + 450_000 * i, x=3 * i - 10, y=5 - i, z=-70 - i, amp=150) for i in range(9)]
    rows += [dict(type=1, time=9 * MS, x=0, y=0, z=-30, amp=2000), dict(type=2, time=9 * MS, x=0, y=0, z=-30, amp=60),
             dict(type=1, time=12 * MS, x=4, y=4, z=-3, amp=700)]
    np.savez_compressed(HERE + '/chunker_midevent.npz',
                        **run_chunker(ref, base_config(chunk_size=0.001, right_raw_extension=500_000), make_instructions(rows), 902, pat))
    # C: record buffer of 700 records: the S2s of ~500 records each force flushes, the big one is partly skipped
    rows = [dict(type=2, time=MS * (1 + 2 * i), x=2 * i, y=-i, z=-20 - 5 * i, amp=int(a)) for i, a in enumerate([120, 200, 80, 2500, 150, 60])]
    rows += [dict(type=1, time=MS * (2 + 2 * i), x=1, y=1, z=-10, amp=900) for i in range(5)]
    np.savez_compressed(HERE + '/chunker_tinybuffer.npz',
                        **run_chunker(ref, base_config(chunk_size=0.005), make_instructions(rows), 903, pat, record_buffer_length=700))
    # D: electron afterpulses (delays up to 0.7 ms), 2 ms chunks
    edges = np.linspace(0, 700e3, 141)
    h = np.exp(-np.arange(140) / 30.0); h *= 4e-3 / h.sum()
    rows = [dict(type=1, time=MS, x=0, y=0, z=-20, amp=2000), dict(type=2, time=MS, x=0, y=0, z=-20, amp=300),
            dict(type=2, time=MS + 450_000, x=5, y=-3, z=-60, amp=400),
            dict(type=1, time=4 * MS, x=5, y=-3, z=-61, amp=900), dict(type=2, time=4 * MS, x=5, y=-3, z=-61, amp=250),
            dict(type=2, time=6 * MS, x=-9, y=4, z=-5, amp=150), dict(type=1, time=9 * MS, x=-9, y=4, z=-5, amp=400)]
    np.savez_compressed(HERE + '/chunker_ele_ap.npz',
                        **run_chunker(ref, base_config(chunk_size=0.002), make_instructions(rows), 904, pat, ele_ap=StubDelayHist(h, edges)))



def fixture_ele_ap_generators(ref):
    """Draws of the reference's electron-afterpulse generators (afterpulse.py:29-92 photo-ionisation, :107-131 gate): for a
    parent S2 with 4000 detected photons, 600 calls each -- instructions per call, electrons per call, and pooled over the
    calls: drift-time grid (from z), electrons per instruction, radius^2, which photon was picked as time zero."""
    cfg = base_config(enable_electron_afterpulses=True, enable_gate_afterpulses=True, photoelectric_p=0.002)
    edges = np.linspace(0, 700e3, 141)
    h = np.exp(-np.arange(140) / 30.0); h *= 4e-3 / h.sum()
    hist = StubDelayHist(h, edges)
    ref.load_resource._cached_configs.clear()
    orig_get = ref.load_resource.straxen.get_resource
    ref.load_resource.straxen.get_resource = lambda path, fmt='text': (hist if fmt in ('dill', 'pkl.gz') else orig_get(path, fmt=fmt))
    cfg['ele_ap_pdfs'] = ''
    try:
        pi = ref.afterpulse.PhotoIonization_Electron(cfg)
        pe = ref.afterpulse.PhotoElectric_Electron(cfg)
    finally:
        ref.load_resource.straxen.get_resource = orig_get
    pi.resource.uniform_to_ele_ap = hist

    class Parent:
        _photon_timings = 5_000_000 + np.arange(4000, dtype=np.int64) * 3
    parent_ins = make_instructions([dict(type=2, time=5_000_000, x=1, y=2, z=-30, amp=200)])
    np.random.seed(606)
    out = {}
    for tag, gen, t_off in (('pi', pi, -cfg['drift_time_gate']), ('pe', pe, +cfg['drift_time_gate'])):
        n_ins, n_el, z, amp, r2, pick = [], [], [], [], [], []
        for _ in range(600):
            ins = gen.generate_instruction(Parent, parent_ins)
            n_ins.append(len(ins)); n_el.append(int(np.sum(ins['amp'])) if len(ins) else 0)
            if len(ins):
                z.append(ins['z']); amp.append(ins['amp']); r2.append(ins['x'].astype(np.float64) ** 2 + ins['y'].astype(np.float64) ** 2)
                pick.append((ins['time'] - t_off - 5_000_000) // 3)
        out[f'{tag}_n_ins'] = np.array(n_ins); out[f'{tag}_n_el'] = np.array(n_el)
        out[f'{tag}_delay'] = -np.concatenate(z).astype(np.float64) / cfg['drift_velocity_liquid']
        out[f'{tag}_amp'] = np.concatenate(amp); out[f'{tag}_r2'] = np.concatenate(r2); out[f'{tag}_pick'] = np.concatenate(pick)
    out['n_photons'] = np.int64(4000); out['histogram'] = h; out['bin_edges'] = edges; out['photoelectric_p'] = np.float64(0.002)
    np.savez_compressed(HERE + '/ele_ap_draws.npz', **out)


def gas_gap_resources():
    """synthetic stand-ins for the private garfield gas gap files (load_resource.py:96-98): excitation-time inverse CDFs for 10
    gas gaps 0.1 mm apart (a smooth S-shaped quantile function whose scale grows with the gap, plus a long last tail as in
    the real tables) and a gas gap map linear in x"""
    gas_gap = 0.20 + 0.01 * np.arange(10)
    q = (np.arange(1000) + 0.5) / 1000
    shape = 120.0 * q + 35.0 * np.log(q / (1 - q)) + 900.0 * q ** 12
    inv = np.array([(0.6 + 2.2 * (g - 0.2) / 0.09) * shape + 40 * g for g in gas_gap])
    return dict(gas_gap=gas_gap, timing_inv_cdf=inv)


def fixture_gas_gap(ref):
    """draws of the reference's 'garfield_gas_gap' luminescence (s2.py:413-483) for three instructions at different gas gaps"""
    gg = gas_gap_resources()

    class Res:
        s2_luminescence_gg = gg

        @staticmethod
        def garfield_gas_gap_map(xy):
            return 0.2 + 0.0009 * (np.asarray(xy)[:, 0] + 50.0)
    xy = np.array([[-48.0, 3.0], [1.7, -20.0], [37.3, 11.0]])
    n = np.array([250_000, 250_000, 250_000])
    np.random.seed(717)
    t = ref.s2.S2.luminescence_timings_garfield_gasgap(xy, n, Res).astype(np.int64)
    out = dict(gas_gap=gg['gas_gap'], timing_inv_cdf=gg['timing_inv_cdf'], xy=xy, cont_gap=Res.garfield_gas_gap_map(xy))
    for k in range(3):
        v, c = np.unique(t[n[:k].sum():n[:k + 1].sum()], return_counts=True)
        out[f'lum{k}_v'], out[f'lum{k}_c'] = v, c
    np.savez_compressed(HERE + '/gas_gap.npz', **out)


def fixture_aft_sigma(ref):
    """S2.photon_channels with s2_aft_sigma / s2_aft_skewness (s2.py:660-665): photons on the top array per instruction, for
    3000 instructions of 2000 photons at one position of a fixed pattern (top fraction 0.72: the clip at 1 is reached)"""
    rng = np.random.default_rng(5)
    p0 = rng.uniform(0.5, 1.5, N_TPC)
    p0[:N_TOP] *= 0.72 / p0[:N_TOP].sum()
    p0[N_TOP:] *= 0.28 / p0[N_TOP:].sum()

    class Res:
        @staticmethod
        def s2_pattern_map(pos):
            return np.tile(p0, (len(pos), 1))
    n_ins, n_ph = 3000, 2000
    cfg = base_config(s2_aft_sigma=0.15, s2_aft_skewness=2.0, turned_off_pmts=np.zeros(0, dtype=np.int64))
    np.random.seed(99)
    ch = ref.s2.S2.photon_channels(np.full(n_ins, 10), np.zeros(n_ins), np.zeros((n_ins, 2)), np.repeat(np.arange(n_ins), n_ph), cfg, Res)
    top = (np.asarray(ch).reshape(n_ins, n_ph) < N_TOP).sum(axis=1)
    # within the top array the relative pattern is untouched: pooled top-channel histogram
    hist = np.bincount(np.asarray(ch)[np.asarray(ch) < N_TOP], minlength=N_TOP)
    np.savez_compressed(HERE + '/aft_sigma.npz', pattern=p0, n_photons=n_ph, sigma=0.15, skewness=2.0, top_counts=top, top_hist=hist)


def fixture_noise_float(ref):
    """RawData.add_noise (rawdata.py:398-437, numba) with a FLOAT noise array on int64 rows: what `data[ch, ix] += noise[ix, ch]`
    stores.  Rows as long as the noise array (high = 0 -> ix_rand = 0, no random draw)."""
    rng = np.random.default_rng(12)
    n_ch, n = 3, 64
    data = rng.integers(-40, 5, size=(n_ch, n)).astype(np.int64)
    noise = rng.uniform(-3.0, 3.0, size=(n, n_ch))
    noise[::7] = np.round(noise[::7])               # some exact integers, some exact halves
    noise[3::11] = np.round(noise[3::11]) + 0.5
    mask = np.zeros(n_ch, dtype=[('mask', '?'), ('left', 'i8'), ('right', 'i8')])
    mask['mask'], mask['left'], mask['right'] = True, 0, n - 1
    out = data.copy()
    ref.rawdata.RawData.add_noise(out, mask, noise, n, n_ch)
    np.savez_compressed(HERE + '/noise_float.npz', data=data, noise=noise, out=out)


def diffusion_case():
    """inputs of the transverse-diffusion fixture: a smooth synthetic S2 pattern map on a regular grid (the one of
    tests/test_gpu_pattern_maps.map_config(0)), constant radial / azimuthal diffusion maps, four S2 positions (one at the edge)"""
    rng = np.random.default_rng(0)
    gx = np.linspace(-66, 66, 31)
    pmt = rng.uniform(-60, 60, (N_TPC, 2))
    d2 = (gx[:, None, None] - pmt[None, None, :, 0]) ** 2 + (gx[None, :, None] - pmt[None, None, :, 1]) ** 2
    s2 = (1.0 / (1.0 + d2 / 40.0)).astype(np.float32)
    pattern = dict(coordinate_system=[['x', [-66, 66, 31]], ['y', [-66, 66, 31]]], map=s2)
    xy = np.array([[3.0, -7.0], [-30.0, 22.0], [40.0, 45.0], [0.5, 62.5]])
    z = np.array([-20.0, -60.0, -110.0, -140.0])
    return pattern, xy, z, dict(d_r=900.0, d_a=300.0, tpc_radius=64.0, v=6.77e-5)      # cm^2/s, cm, cm/ns


def fixture_diffusion(ref):
    """S2.s2_pattern_map_diffuse (s2.py:560-613) with diffusion_transverse_map: averaged patterns of four instructions of
    20000 electrons each"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('_itp_map', os.path.join(os.path.dirname(os.path.dirname(HERE)), 'wfsim_amd', 'itp_map.py'))
    itp = importlib.util.module_from_spec(spec); spec.loader.exec_module(itp)
    pattern, xy, z, par = diffusion_case()

    class Res:
        s2_pattern_map = itp.InterpolatingMap(pattern)

        @staticmethod
        def field_dependencies_map(z, xy, map_name='map'):
            return np.full(len(z), dict(diffusion_radial_map=par['d_r'], diffusion_azimuthal_map=par['d_a'])[map_name], dtype=np.float64)
    cfg = base_config(tpc_radius=par['tpc_radius'], drift_velocity_liquid=par['v'], diffusion_constant_transverse=1.0,
                      enable_field_dependencies=dict(diffusion_transverse_map=True, drift_speed_map=False))
    ne = np.full(len(z), 20000)
    np.random.seed(404)
    pat = ref.s2.S2.s2_pattern_map_diffuse(ne, z, xy, cfg, Res)
    np.savez_compressed(HERE + '/diffusion.npz', patterns=pat, n_electron=ne)


def fixture_optical_adjustment(ref):
    """utils.optical_adjustment (host preparation of optical input): random photon lists, a third of the entries longer
    than PULSE_MAX_DURATION, some empty"""
    rng = np.random.default_rng(11)
    n = 60
    ins = np.zeros(n, dtype=instruction_dtype + optical_extra_dtype)
    nph = rng.integers(0, 25, n); nph[::7] = 0
    ins['_first'] = np.cumsum(nph) - nph
    ins['_last'] = np.cumsum(nph)
    ins['time'] = 1_000_000 * np.arange(n)
    ins['type'], ins['event_number'] = 1, np.arange(n)
    tot = int(nph.sum())
    timings = rng.integers(0, 400, tot).astype(np.int64)
    tail = rng.random(tot) < 0.08
    timings[tail] += rng.integers(900, 5000, tail.sum())
    channels = rng.integers(0, 120, tot).astype(np.int64)
    t_in, c_in = timings.copy(), channels.copy()
    out = ref.utils.optical_adjustment(ins.copy(), timings, channels)
    np.savez_compressed(HERE + '/optical_adjustment.npz', ins_in=ins, timings_in=t_in, channels_in=c_in,
                        ins_out=out, timings_out=timings, channels_out=channels)


class _FakeBranch:
    """what uproot hands the reference for one branch of the Geant4 tree: .array(library='np') -> (object) array per event"""

    def __init__(self, values):
        self.values = values

    def array(self, library='np'):
        return self.values


def synthetic_g4_events(rng, n_events, ch_lo, ch_hi, with_energy):
    """array-backed stand-in for the Geant4 optical tree (strax_interface.py:292-322 reads these branches)"""
    nhit = rng.integers(0, 40, n_events); nhit[::9] = 0

    def ragged(make):
        out = np.empty(n_events, dtype=object)
        for i in range(n_events):
            out[i] = make(int(nhit[i]))
        return out
    ev = dict(eventid=np.arange(100, 100 + n_events, dtype=np.int64),
              pmthitID=ragged(lambda k: rng.integers(ch_lo - 3, ch_hi + 4, k).astype(np.int64)),          # a few ids outside the array
              pmthitTime=ragged(lambda k: np.where(rng.random(k) < 0.1, rng.uniform(1.5e-6, 6e-6, k), rng.uniform(0, 4e-7, k))),   # s; some > 1 us: split pulses
              xp_pri=rng.uniform(-600, 600, n_events), yp_pri=rng.uniform(-600, 600, n_events), zp_pri=rng.uniform(-1400, 0, n_events))
    if with_energy:
        ev['pmthitEnergy'] = ragged(lambda k: np.where(rng.random(k) < 0.05, 0.9, rng.uniform(2.0, 4.5, k)))       # eV; 0.9 eV -> 1378 nm: outside the table
    return ev


def fixture_optical_frontend(ref):
    """the host front end of the optical / nVeto path run on the REFERENCE -- _read_optical_nveto + read_optical
    (strax_interface.py:234-333) on an array-backed stand-in for the Geant4 tree (uproot is not installed: `uproot.open` is
    pointed at it), and RawRecordsFromMcChain.set_timing (:824-863) on a bare object.  The random draws come from numpy's
    legacy global generator, seeded: a RandomState with the same seed reproduces them in the test."""
    import types
    si = ref.strax_interface
    out = {}
    rng = np.random.default_rng(2024)
    ch_lo, ch_hi = 2000, 2119
    wl = np.arange(250.0, 701.0, 10.0)
    qe = {str(c): (35.0 * np.exp(-0.5 * ((wl - 400.0 - (c % 7) * 3) / 80.0) ** 2)).tolist() for c in range(ch_lo, ch_hi + 1)}
    qe_data = dict(nv_pmt_qe_wavelength=wl.tolist(), nv_pmt_qe=qe)
    out['qe_wavelength'] = wl
    out['qe_table'] = np.array([qe[str(c)] for c in range(ch_lo, ch_hi + 1)])
    cases = [('nveto', 'XENONnT_neutron_veto', True, dict(nv_pmt_ce_factor=0.8), 501),
             ('nveto_noqe', 'XENONnT_neutron_veto', False, dict(entry_start=105, entry_stop=140), 502),
             ('tpc', 'XENONnT', None, dict(entry_start=110), 503)]
    for tag, detector, use_qe, extra, seed in cases:
        lo, hi = (ch_lo, ch_hi) if detector != 'XENONnT' else (0, 493)
        ev = synthetic_g4_events(rng, 64, lo, hi, with_energy=detector != 'XENONnT')
        if detector == 'XENONnT':
            ev['pmthitID'] = np.array([np.clip(h, 0, 493) for h in ev['pmthitID']] + [None], dtype=object)[:-1]
        config = dict(detector=detector, channel_map=dict(nveto=(ch_lo, ch_hi), tpc=(0, 493)), fax_file='stand-in', tag=tag, **extra)
        fake = {k: _FakeBranch(v) for k, v in ev.items()}
        sys.modules['uproot'].open = lambda path, _f=fake: types.SimpleNamespace(get=lambda name: _f)
        si.uproot = sys.modules['uproot']
        si.wfsim.load_config = lambda cfg, _q=(qe_data if use_qe else None): types.SimpleNamespace(nv_pmt_qe=_q)
        si._cached_wavelength_to_qe_arr.clear()
        np.random.seed(seed)
        ins, channels, timings = si.read_optical(config)
        for k, v in ev.items():
            if v.dtype == object:
                out[f'{tag}_{k}_flat'] = np.concatenate([np.asarray(x) for x in v]) if len(v) else np.zeros(0)
                out[f'{tag}_{k}_len'] = np.array([len(x) for x in v], dtype=np.int64)
            else:
                out[f'{tag}_{k}'] = v
        out[f'{tag}_seed'] = np.int64(seed)
        out[f'{tag}_entry'] = np.array([config.get('entry_start', 0), config['entry_stop']], dtype=np.int64)
        out[f'{tag}_ce'] = np.float64(extra.get('nv_pmt_ce_factor', 1.0))
        out[f'{tag}_ins'], out[f'{tag}_channels'], out[f'{tag}_timings'] = ins, channels, timings
        print(tag, len(ins), 'instructions', len(channels), 'photons kept of', int(out[f'{tag}_pmthitID_len'].sum()))
    # ---- RawRecordsFromMcChain.set_timing on a bare object
    for tag, targets, entry, seed in [('both', ('tpc', 'nveto'), (None, None), 601), ('nv_only', ('nveto',), (3, 40), 602), ('tpc_only', ('tpc',), (None, None), 603)]:
        obj = object.__new__(si.RawRecordsFromMcChain)
        obj.config = dict(targets=targets, event_rate=1000.0, entry_start=entry[0] if entry[0] is not None else 0, entry_stop=entry[1])
        g4 = []
        if 'tpc' in targets:
            n = 90
            epix = np.zeros(n, dtype=instruction_dtype)
            epix['g4id'] = np.sort(rng.integers(2, 45, n))
            epix['time'] = rng.integers(0, 2_000_000, n)          # physical delays inside the event
            epix['time'][::17] += 3_000_000_000                   # far too late: removed
            epix['type'] = rng.integers(1, 3, n)
            epix['amp'] = rng.integers(1, 500, n)
            obj.instructions_epix = epix
            g4.append(epix['g4id'])
            out[f'timing_{tag}_epix_in'] = epix.copy()
        if 'nveto' in targets:
            n = 40
            nv = np.zeros(n, dtype=instruction_dtype + optical_extra_dtype)
            nv['g4id'] = np.sort(rng.choice(np.arange(3, 40), n))
            nv['time'] = rng.integers(0, 500, n)
            nv['type'] = 1
            obj.instructions_nveto = nv
            g4.append(nv['g4id'])
            out[f'timing_{tag}_nveto_in'] = nv.copy()
        obj.g4id = np.unique(np.concatenate(g4))
        np.random.seed(seed)
        si.RawRecordsFromMcChain.set_timing(obj)
        out[f'timing_{tag}_seed'] = np.int64(seed)
        out[f'timing_{tag}_entry_in'] = np.array([-1 if e is None else e for e in entry], dtype=np.int64)
        out[f'timing_{tag}_entry_out'] = np.array([obj.config['entry_start'], obj.config['entry_stop']], dtype=np.int64)
        if 'tpc' in targets:
            out[f'timing_{tag}_epix_out'] = obj.instructions_epix
        if 'nveto' in targets:
            out[f'timing_{tag}_nveto_out'] = obj.instructions_nveto
    np.savez_compressed(HERE + '/optical_frontend.npz', **out)


def hist(x):
    v, c = np.unique(np.asarray(x, dtype=np.int64), return_counts=True)
    return v.astype(np.int64), c.astype(np.int64)


def fixture_distributions(ref):
    """G7: integer-valued samples of every random stage, as (value, count) histograms."""
    cfg = base_config()
    ref.load_resource._cached_configs.clear()
    s1, s2 = ref.s1.S1(cfg), ref.s2.S2(cfg)
    P = ref.pulse.Pulse
    out = {}
    n = 2_000_000
    np.random.seed(9001)
    t = s1.photon_timings(t=np.array([0]), n_photon_hits=np.array([n]), recoil_type=np.array([7]),
                          config=cfg, phase='liquid')
    out['s1_simple_v'], out['s1_simple_c'] = hist(t)
    tts = np.random.normal(cfg['pmt_transit_time_mean'], cfg['pmt_transit_time_spread'] / 2.35482, n).astype(np.int64)
    out['tts_v'], out['tts_c'] = hist(tts)
    out['st_gas_v'], out['st_gas_c'] = hist(P.singlet_triplet_delays(n, cfg['singlet_fraction_gas'], cfg, 'gas'))
    out['lum_v'], out['lum_c'] = hist(s2.luminescence_timings_simple(np.zeros((1, 2)), np.array([n]), cfg, s2.resource))
    # electron arrival + photons/electron for two depths
    for tag, z in [('z10', -10.0), ('z90', -90.0)]:
        zi, xy = np.array([z]), np.zeros((1, 2))
        ne = np.array([400_000])
        sc = s2.get_s2_light_yield(xy, cfg, s2.resource)
        nxy, npe, et = s2.get_n_photons(np.array([0]), ne, zi, xy, sc, cfg, s2.resource)
        out[f'etime_{tag}_v'], out[f'etime_{tag}_c'] = hist(et)
        out[f'nph_e_{tag}_v'], out[f'nph_e_{tag}_c'] = hist(npe)
        out[f'sc_gain_{tag}'] = sc
        dm, ds = s2.get_s2_drift_time_params(zi, xy, cfg, s2.resource)
        out[f'drift_{tag}'] = np.array([dm[0], ds[0]])
        n_el = s2.get_electron_yield(np.full(200_000, 1000), np.zeros((200_000, 2)), np.full(200_000, z),
                                     np.zeros((200_000, 2)), cfg, s2.resource)
        out[f'nel_{tag}_v'], out[f'nel_{tag}_c'] = hist(n_el)
    nh = s1.get_n_photons(np.full(400_000, 1667), np.zeros((400_000, 3)), s1.resource.s1_lce_correction_map, cfg)
    out['s1_nhits_v'], out['s1_nhits_c'] = hist(nh)
    # full S2 photon time relative to instruction time (all terms), z=-10
    np.random.seed(9002)
    ins = make_instructions([dict(type=2, time=0, x=0, y=0, z=-10, amp=20000)])
    s2(ins)
    out['s2_full_v'], out['s2_full_c'] = hist(s2._photon_timings)
    out['s2_full_ch_counts'] = np.bincount(s2._photon_channels, minlength=N_TPC).astype(np.int64)
    # SPE gain factors
    np.random.seed(9003)
    p = P(cfg)
    idx = (np.random.random(n) * 2000).astype(np.int64) + 1
    out['spe_idx_counts'] = np.bincount(idx, minlength=2001).astype(np.int64)
    dpe = np.random.binomial(1, cfg['p_double_pe_emision'], n)
    out['dpe_frac'] = np.array([dpe.mean(), n])
    np.savez_compressed(HERE + '/dists.npz', **out)


def model_fixture_inputs():
    """synthetic resources of the model variants (the real splines / garfield tables are private files)"""
    rng = np.random.default_rng(4242)
    zg, ug = np.linspace(-100.0, 0.0, 11), np.linspace(0.0, 1.0, 21)
    shape_u = -np.log(1 - 0.97 * ug)                                 # a propagation-time quantile function
    s1_top = (4.0 + 0.05 * (zg[:, None] + 100.0)) * shape_u[None, :] + 1.5
    s1_bot = (9.0 - 0.04 * (zg[:, None] + 100.0)) * shape_u[None, :] + 0.5
    u2 = np.linspace(0.0, 1.0, 33)
    s2_top = 12.0 * -np.log(1 - 0.95 * u2)
    s2_bot = 3.0 + 25.0 * u2 ** 2
    gx = np.linspace(-0.25, 0.25, 11)
    gt = np.stack([rng.gamma(3.0 + 8 * abs(x), 60.0, 4000) + 900 for x in gx])          # ns, [rows, samples]
    return dict(s1_z=zg, s1_u=ug, s1_top=s1_top, s1_bottom=s1_bot, s2_u=u2, s2_top=s2_top, s2_bottom=s2_bot,
                garfield_x=gx, garfield_t=gt)


def fixture_model_distributions(ref):
    """Delay of a photon (all terms + transit time, pulse.py:53-56) under the model variants of S1.photon_timings
    (s1.py:162-238) and S2.photon_timings (s2.py:504-557), as histograms of the reference's own draws."""
    from wfsim_amd.itp_map import InterpolatingMap          # stands in for straxen.InterpolatingMap (the resource object)
    m = model_fixture_inputs()
    out = {k: v for k, v in m.items()}
    n = 2_000_000
    s1_spline = InterpolatingMap(dict(coordinate_system=[['z', [-100.0, 0.0, 11]], ['u', [0.0, 1.0, 21]]],
                                      top=m['s1_top'].tolist(), bottom=m['s1_bottom'].tolist()), method='RegularGridInterpolator')
    s2_spline = InterpolatingMap(dict(coordinate_system=[['u', [0.0, 1.0, 33]]], top=m['s2_top'].tolist(), bottom=m['s2_bottom'].tolist()))

    def tts(cfg, k):
        return np.random.normal(cfg['pmt_transit_time_mean'], cfg['pmt_transit_time_spread'] / 2.35482, k).astype(np.int64)

    # S1: custom recoil models, with and without the 'simple' terms.  S1.er reads `units`, which s1.py never imports (as
    # shipped the ER branch ends in a NameError): the module is handed the reference's own units module to pin what the
    # code computes once that import exists
    if not hasattr(ref.s1, 'units'):
        ref.s1.units = ref.units
    for tag, model, recoil in [('er', 'custom', 7), ('nr', 'custom', 0), ('alpha', 'custom', 6), ('led', 'custom', 20), ('er_simple', 'simple+custom', 7)]:
        cfg = base_config(s1_model_type=model, led_pulse_length=33.3)
        ref.load_resource._cached_configs.clear()
        s1 = ref.s1.S1(cfg)
        np.random.seed(9100 + recoil)
        t = s1.photon_timings(t=np.array([0]), n_photon_hits=np.array([n]), recoil_type=np.array([recoil]), config=cfg, phase='liquid')
        out[f's1_{tag}_v'], out[f's1_{tag}_c'] = hist(t + tts(cfg, n))
    # S1: optical propagation at a z between two grid nodes, top and bottom array channels
    cfg = base_config(s1_model_type='simple+optical_propagation')
    ref.load_resource._cached_configs.clear()
    s1 = ref.s1.S1(cfg)
    s1.resource.s1_optical_propagation_spline = s1_spline
    for tag, ch in [('top', 5), ('bottom', 300)]:
        np.random.seed(9200 + ch)
        t = s1.photon_timings(t=np.array([0]), n_photon_hits=np.array([n]), recoil_type=np.array([7]), config=cfg, phase='liquid',
                              channels=np.full(n, ch), positions=np.array([[0.0, 0.0, -33.3]]), resource=s1.resource)
        out[f's1_prop_{tag}_v'], out[f's1_prop_{tag}_c'] = hist(t + tts(cfg, n))
    # S2: optical propagation (simple luminescence), garfield luminescence (zero_delay), both
    gar = dict(t=m['garfield_t'], x=m['garfield_x'])
    for tag, lum, tm in [('prop', 'simple', 'optical_propagation'), ('garfield', 'garfield', 'zero_delay'), ('garfield_prop', 'garfield', 'optical_propagation')]:
        cfg = base_config(s2_luminescence_model=lum, s2_time_model=tm)
        ref.load_resource._cached_configs.clear()
        s2 = ref.s2.S2(base_config())          # the garfield table is attached below instead of being read from a private file
        s2.resource.s2_optical_propagation_spline = s2_spline
        s2.resource.s2_luminescence = gar
        xy = np.array([[0.21, 0.0]])
        for side, ch in [('top', 5), ('bottom', 300)]:
            np.random.seed(9300 + ch)
            t = s2.photon_timings(xy, np.array([n]), np.zeros(1, dtype=np.int64), np.array([n]), np.full(n, ch), 'gas', cfg, s2.resource)
            out[f's2_{tag}_{side}_v'], out[f's2_{tag}_{side}_c'] = hist(t + tts(cfg, n))
    # S2 'simple' luminescence with gas gap warping (s2.py:360-378): the gas gap comes from a map of the position
    cfg = base_config(enable_gas_gap_warping=True, s2_time_model='zero_delay')
    ref.load_resource._cached_configs.clear()
    s2 = ref.s2.S2(base_config())
    s2.resource.gas_gap_length = lambda xy: 0.25 + 0.0004 * xy[:, 0]
    for tag, x in [('narrow', -20.0), ('wide', 30.0)]:
        np.random.seed(9400 + int(x))
        t = s2.photon_timings(np.array([[x, 0.0]]), np.array([n]), np.zeros(1, dtype=np.int64), np.array([n]), np.full(n, 5), 'gas', cfg, s2.resource)
        out[f's2_warp_{tag}_v'], out[f's2_warp_{tag}_c'] = hist(t + tts(cfg, n))
    np.savez_compressed(HERE + '/dists_models.npz', **out)


def fixture_chain_stats(ref):
    """Per-instruction summary statistics of full reference runs (statistical end-to-end pins)."""
    MS = 1_000_000
    out = {}
    for tag, rows, seed in [
        ('s1', [dict(type=1, time=MS * (i + 1), x=0, y=0, z=-50, amp=1667) for i in range(300)], 71),
        ('s2', [dict(type=2, time=MS * (i + 1), x=0, y=0, z=-10, amp=300) for i in range(60)], 72),
    ]:
        r = run_chain(ref, base_config(), make_instructions(rows), seed, None)
        tr = r['truth']
        for f in ['n_photon', 'n_pe', 'n_photon_trigger', 'n_pe_trigger', 'raw_area', 'raw_area_trigger',
                  'n_photon_bottom', 't_mean_photon', 't_sigma_photon', 't_first_photon', 't_last_photon',
                  'n_electron', 't_mean_electron', 't_sigma_electron', 'endtime', 'time']:
            out[f'{tag}_{f}'] = tr[f]
        nz = np.bincount(r['zle_digit'], minlength=len(r['dg_left']))
        out[f'{tag}_n_zle'] = nz
        ln = (r['zle_right'] - r['zle_left'] + 1)
        out[f'{tag}_zle_samples'] = np.bincount(r['zle_digit'], weights=ln, minlength=len(r['dg_left']))
        area = np.array([(16000 - r['zle_data'][a:b]).sum() for a, b in zip(r['zle_data_off'][:-1], r['zle_data_off'][1:])])
        out[f'{tag}_zle_area'] = np.bincount(r['zle_digit'], weights=area, minlength=len(r['dg_left']))
        out[f'{tag}_width'] = r['dg_right'] - r['dg_left']
    np.savez_compressed(HERE + '/chain_stats.npz', **out)


if __name__ == '__main__':
    which = sys.argv[1:] or ['tables', 'add_current', 'chains', 'dists', 'models', 'stats', 'chunker', 'ele_ap_draws', 'gas_gap', 'aft_sigma', 'noise_float', 'diffusion', 'frontend']
    ref = import_reference_interface() if ('chunker' in which or 'frontend' in which) else import_reference()
    own = {'optical_chain', 'pmt_ap_draws', 'pulse_edges', 'window_edges', 'zle_edges', 'spe_channels'}           # these write their own files only
    p = fixture_tables(ref) if set(which) - own else None
    if 'optical_chain' in which:
        fixture_chain_optical(ref)
    if 'pmt_ap_draws' in which:
        fixture_pmt_ap_draws(ref)
    if 'pulse_edges' in which:
        fixture_pulse_edges(ref)
    if 'window_edges' in which:
        fixture_window_edges(ref)
    if 'zle_edges' in which:
        fixture_zle_edges(ref)
    if 'spe_channels' in which:
        fixture_spe_channels(ref)
    if 'add_current' in which:
        fixture_add_current(ref, p)
    if 'chains' in which:
        fixture_chains(ref)
    if 'chains' in which or 'params' in which:
        fixture_chain_params(ref)
    if 'chains' in which or 'geometry' in which:
        fixture_chain_geometry(ref)
    if 'chains' in which or 'runsets' in which:
        fixture_chain_runsets(ref)
    if 'chains' in which or 'ele_ap' in which:
        fixture_chain_electron_ap(ref)
    if 'optical' in which or 'tables' in which:
        fixture_optical_adjustment(ref)
    if 'frontend' in which:
        fixture_optical_frontend(ref)
    if 'dists' in which:
        fixture_distributions(ref)
    if 'models' in which:
        fixture_model_distributions(ref)
    if 'stats' in which:
        fixture_chain_stats(ref)
    if 'chunker' in which:
        fixture_chunker(ref)
    if 'ele_ap_draws' in which or 'ele_ap' in which:
        fixture_ele_ap_generators(ref)
    if 'gas_gap' in which or 'models' in which:
        fixture_gas_gap(ref)
    if 'aft_sigma' in which:
        fixture_aft_sigma(ref)
    if 'noise_float' in which:
        fixture_noise_float(ref)
    if 'diffusion' in which:
        fixture_diffusion(ref)
    for f in sorted(os.listdir(HERE)):
        if f.endswith(('.npz', '.json')):
            print(f'{f:28s} {os.path.getsize(os.path.join(HERE, f)) / 1024:9.1f} KiB')
