#!/usr/bin/env python3
"""Generate tests/golden/chain_optical_ap.npz (+ chain_optical_ap_config.json) by RUNNING the reference's RawDataOptical with PMT
afterpulses on: RawData.sim_data (rawdata.py:166-190) runs the afterpulse Pulse call behind every primary call, the optical ones
included.  Run once in the build container, next to make_golden.py (whose helpers it imports; that file is not edited):

    python tests/golden/make_golden_optical_ap.py

Detector XENONnT (494 channels; the reference loads no afterpulse tables for the neutron veto), the tables of pmt_ap_tables.npz with
every probability column times 4 (about a quarter of the parents fire), pmt_ap_modifier 1.3, pmt_ap_t_modifier 3, three turned-off
PMTs, right_raw_extension 2 us so that the stream breaks into windows.  What is written is DATA only, as for the other chains.
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G   # noqa: E402
from _ref_stubs import import_reference   # noqa: E402
from tests.optical_afterpulse import edge_input   # noqa: E402
from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype, truth_extra_dtype   # noqa: E402

AP_SCALE, SEED = 4.0, 1311
TURNED_OFF = [7, 130, 400]


def overrides():
    gains = np.full(G.N_TPC, 2e6)
    gains[TURNED_OFF] = 0.0
    return dict(gains=gains, turned_off_pmts=TURNED_OFF, right_raw_extension=2000, pmt_ap_modifier=1.3, pmt_ap_t_modifier=3)


def scaled_tables():
    d = np.load(HERE + '/pmt_ap_tables.npz')
    out = {}
    for name in ['He', 'Xe', 'Uniform']:
        out[name] = dict(delaytime_cdf=d[f'{name}_delaytime_cdf'] * AP_SCALE, amplitude_cdf=d[f'{name}_amplitude_cdf'],
                         delaytime_bin_size=float(d[f'{name}_delaytime_bin_size']), amplitude_bin_size=float(d[f'{name}_amplitude_bin_size']))
    return out


def main():
    ref = import_reference()
    ov = overrides()
    ins, channels, timings = edge_input(80, G.N_TPC, seed=1301, max_photons=40, dead_channel=TURNED_OFF[0])
    cfg = G.base_config(**ov)
    path = G.TMP + '/pmt_ap_optical.json.gz'           # the gz-json photon_ap_cdfs mechanism of run_chain
    with gzip.open(path, 'wt') as f:
        json.dump({k: {q: (v.tolist() if isinstance(v, np.ndarray) else v) for q, v in d.items()} for k, d in scaled_tables().items()}, f)
    cfg['photon_ap_cdfs'] = path
    cfg['enable_pmt_afterpulses'] = True
    ref.load_resource._cached_configs.clear()
    ref.pulse._cached_pmt_current_templates.clear()
    ref.pulse._cached_uniform_to_pe_arr.clear()
    rd = ref.rawdata.RawDataOptical(cfg, channels=channels, timings=timings)
    out = G.record_chain(ref, rd, ins, SEED, instruction_dtype + optical_extra_dtype + truth_extra_dtype + [('fill', bool)], store_entry=True)
    out.update(channels=channels, timings=timings, cutoff=np.int64(1e6))
    for k in ('dg_sum_min', 'dg_sum_total'):
        out.pop(k, None)
    np.savez_compressed(HERE + '/chain_optical_ap.npz', **out)
    with open(HERE + '/chain_optical_ap_config.json', 'w') as f:
        json.dump(dict({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in ov.items()}, ap_scale=AP_SCALE), f)
    kinds = out['call_kind']
    print(len(kinds), 'calls', int((kinds == 3).sum()), 'afterpulse calls', len(out['dg_left']), 'windows', len(out['ph_t']), 'photons',
          os.path.getsize(HERE + '/chain_optical_ap.npz'), 'bytes')


if __name__ == '__main__':
    main()
