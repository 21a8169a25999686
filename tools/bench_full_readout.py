"""Side benchmark: what full readout costs (config 'full_readout').

* ``mixed_off``   the mixed batch of workloads.mixed_config (S1 + S2 pairs, PMT afterpulses, the 3000-sample noise table) with the
                  switch off: the "changes nothing when off" check.  ``--parent-json`` names the result of this tool's ``mixed_off`` leg
                  on the parent commit (same box); the verdict ``inside_parent_spread`` compares the medians of the repetitions with
                  the parent's minimum and maximum, both lists are recorded.
* ``mixed_on``    the same batch with the switch on;
* ``s1_on`` / ``s1_off``   10^4 S1 instructions (workloads.s1_batch) with the noise model (sigma 2.2), one window each: the batch
                  whose rows are almost all rows without a pulse.

Per leg: ms per step (several repetitions), records, bytes of records, rows, and from one profiled step the times of the row kernels
-- k_row_empty is the new one.  ``record_bytes_at_hbm_ms`` is what writing the records alone costs at the HBM rate (--hbm-tbs,
8 TB/s peak of the MI355X), and ``fraction_of_hbm`` that over the step; ``ns_per_sample`` compares the rows without a pulse
(k_row_empty over their samples) with the resident rows (k_row_pulse over theirs) in the same run.

usage: python tools/bench_full_readout.py [--instructions 10000] [--steps 10] [--warmup 3] [--legs mixed_off,mixed_on] [--parent-json f] [--out profiles/full_readout.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wfsim_amd import workloads as W                          # noqa: E402
from wfsim_amd.engine import Engine                           # noqa: E402
from wfsim_amd.physics import instruction_params              # noqa: E402
from wfsim_amd.resource import Resource                       # noqa: E402
from wfsim_amd.scheduler import schedule                      # noqa: E402

ROW_KERNELS = ('k_rows_widen', 'k_row_empty', 'k_row_pulse', 'k_zle', 'k_pack', 'k_pack_res', 'k_tile_add')
RECORD_BYTES = 244


def make(ins, **overrides):
    cfg = W.mixed_config(seed=3, **overrides)
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    eng = Engine(cfg, res)
    ip = instruction_params(ins[order], cfg, res, device_maps=eng.device_maps)
    eng.load_instructions(ins[order], order.astype(np.uint32), cluster, key, ip)
    return eng


def timed(eng, steps, warmup, repeats=5):
    out = []
    for _ in range(repeats):
        for _ in range(warmup):
            eng.run()
        t0 = time.perf_counter()
        for _ in range(steps):
            c = eng.run()                 # (ends with a read-back of the batch's counters: the stream is idle when it returns)
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return out, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instructions', type=int, default=10000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--legs', default='mixed_off,mixed_on,s1_off,s1_on')
    ap.add_argument('--hbm-tbs', type=float, default=8.0)
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (torch.cuda before the library, engine.load_library)
    res = dict(instructions=args.instructions, steps=args.steps, warmup=args.warmup, hbm_tbs=args.hbm_tbs)
    for leg in args.legs.split(','):
        on = leg.endswith('_on')
        ov = dict(full_readout=True) if on else {}       # (off: the key is absent, as on the parent commit)
        if leg.startswith('s1'):
            ins, ov = W.s1_batch(args.instructions), dict(ov, noise_model={'sigma': 2.2})
        else:
            ins = W.mixed_batch(args.instructions)
        eng = make(ins, **ov)
        ms, c = timed(eng, args.steps, args.warmup)
        eng.set_profiling(True)
        eng.run()
        kt = eng.kernel_times()
        eng.set_profiling(False)
        med = float(np.median(ms))
        rec_bytes = int(c['n_records']) * RECORD_BYTES
        hbm_ms = 1e3 * rec_bytes / (args.hbm_tbs * 1e12)
        r = dict(ms_per_step=[round(x, 3) for x in ms], median_ms=round(med, 3), records=int(c['n_records']), record_bytes=rec_bytes,
                 rows=int(c['n_rows']), intervals=int(c['n_intervals']), raw_samples=int(c['n_raw_samples']),
                 record_bytes_at_hbm_ms=round(hbm_ms, 4), fraction_of_hbm=round(hbm_ms / med, 4),
                 kernels_ms={k: round(kt[k][0], 4) for k in ROW_KERNELS if k in kt}, all_kernels_ms=round(sum(v[0] for v in kt.values()), 3))
        if on:
            g = eng.groups()
            keep = g['right'] >= g['left']
            slots = int(eng.params['n_tpc'])             # (no HE rows in these configurations)
            win = (g['right'] - g['left'] + 1)[keep]
            full_samples = int(win.sum()) * slots            # an upper bound: left is moved down to an even sample
            r['window_samples_all_rows'] = full_samples
            if 'k_row_empty' in kt and full_samples > c['n_raw_samples']:
                r['ns_per_sample_row_empty'] = round(1e6 * kt['k_row_empty'][0] / (full_samples - int(c['n_raw_samples'])), 5)
            if 'k_row_pulse' in kt and c['n_raw_samples'] > 0:
                r['ns_per_sample_row_pulse_upper'] = round(1e6 * kt['k_row_pulse'][0] / int(c['n_raw_samples']), 5)      # (raw_samples also counts accumulator rows)
        res[leg] = r
        eng.close()
    if args.parent_json and 'mixed_off' in res:
        parent = []
        for name in args.parent_json.split(','):          # (several runs of the parent, taken before and after this one)
            with open(name) as f:
                parent += json.load(f)['mixed_off']['ms_per_step']
        res['mixed_off_parent_ms_per_step'] = parent
        res['mixed_off_inside_parent_spread'] = bool(min(parent) <= res['mixed_off']['median_ms'] <= max(parent))
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
