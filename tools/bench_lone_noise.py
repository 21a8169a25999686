"""Side benchmark: what the noise-hit seeds of the lone-hit rows cost (config 'noise_lone_hits').

1. The scan.  ``Engine.lone_hits`` over one simulated second (10^8 samples of 10 ns) against no rows, without dark-count rates, for the
   noise kinds 3 (white), 4 (taps and common streams) and 5 (slow levels on top), on a 494-channel TPC engine and a 120-channel veto
   engine: the kernel time of ``k_lone_noise_scan`` (profiling timers) as ns per scanned sample, the wall time of the pass beside it.
   Beside it the per-sample time of ``k_row_empty<NK>`` in the same process: an S1 batch under ``full_readout`` with the same model, the
   kernel's time over the samples of the rows without a pulse (tools/bench_full_readout.py measures it the same way).  That kernel makes
   the same draws and stores on top.  Every figure is taken ``--repeats`` times: minimum, median and maximum are reported.
2. The pass in a run.  The mixed workload of tools/bench_lone_hits.py (S1 + S2 pairs 1 ms apart, PMT afterpulses and noise on, the noise
   from the model {'sigma': 2.2}, 40 Hz per tube) through ``RawData.iter_batches`` with both keys off, 'dark_count_lone_hits' alone,
   'noise_lone_hits' alone and both: seconds per run behind a warm-up, records of either kind.

Prints one JSON line.

usage: python tools/bench_lone_noise.py [--repeats 3] [--instructions 2000] [--out profiles/lone_noise.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

SECOND = 10 ** 8                                    # samples of 10 ns


def models(n_ch):
    """the three models of the scan: the white Gaussian, the same with four taps and a common stream per board of eight channels, the
    same with two slow levels -- at the ordinary threshold next to nothing crosses, so the pass is the scan"""
    white = {'sigma': 2.2}
    taps = np.array([0.8, 0.4, 0.2, 0.1])
    colour = dict(white, taps=taps / np.sqrt((taps ** 2).sum()), common=dict(groups=(np.arange(n_ch) // 8).astype(np.int64), gain=0.5, sigma=1.0))
    slow = dict(colour, slow=dict(shifts=[6, 10], amplitude=[0.3, 0.3]))
    return {3: white, 4: colour, 5: slow}


def spread(x):
    return dict(min=float(np.min(x)), median=float(np.median(x)), max=float(np.max(x)), all=[float(v) for v in x])


def time_scan(eng, n_ch, repeats):
    eng.lone_hits(0, SECOND // 100)                 # (buffers and code objects)
    wall, kern, n_rec = [], [], 0
    eng.set_profiling(True)
    seen = eng.kernel_times().get('k_lone_noise_scan', (0.0, 0))[0]
    for _ in range(repeats):
        t0 = time.perf_counter()
        rec = eng.lone_hits(0, SECOND)
        wall.append(1e3 * (time.perf_counter() - t0))
        total = eng.kernel_times()['k_lone_noise_scan'][0]      # (the timers of the passes add up until the next run)
        kern.append(total - seen)
        seen = total
        n_rec = len(rec)
    eng.set_profiling(False)
    samples = n_ch * SECOND
    return dict(channels=n_ch, samples=samples, records=n_rec, rows=int(len(eng.lone_hit_rows())), pass_ms=spread(wall), scan_kernel_ms=spread(kern),
                scan_ns_per_sample=spread([1e6 * k / samples for k in kern]))


def time_row_empty(model, repeats, instructions):
    """ns per sample of k_row_empty<NK> on the rows without a pulse of a fully read-out S1 batch"""
    from wfsim_amd import workloads as W
    from wfsim_amd.engine import Engine
    from wfsim_amd.physics import instruction_params
    from wfsim_amd.resource import Resource
    from wfsim_amd.scheduler import schedule
    cfg = W.mixed_config(seed=3, full_readout=True, noise_model=model)
    res = Resource(cfg)
    ins = W.s1_batch(instructions)
    order, key, cluster = schedule(ins, cfg)
    eng = Engine(cfg, res)
    ip = instruction_params(ins[order], cfg, res, device_maps=eng.device_maps)
    eng.load_instructions(ins[order], order.astype(np.uint32), cluster, key, ip)
    eng.run()
    eng.set_profiling(True)
    out = []
    for _ in range(repeats):
        c = eng.run()
        kt = eng.kernel_times()
        g = eng.groups()
        keep = g['right'] >= g['left']
        full = int((g['right'] - g['left'] + 1)[keep].sum()) * int(eng.params['n_tpc'])
        out.append(1e6 * kt['k_row_empty'][0] / (full - int(c['n_raw_samples'])))
    eng.close()
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--instructions', type=int, default=2000, help='instructions of the mixed run (1 ms per pair: 2000 are a simulated second)')
    ap.add_argument('--legs', default='scan,mixed')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  (torch.cuda before the library, engine.load_library)
    import wfsim_amd
    from wfsim_amd import workloads as W
    from wfsim_amd.engine import Engine
    from wfsim_amd.resource import Resource
    res = dict(repeats=args.repeats, simulated_second_samples=SECOND)
    if 'scan' in args.legs.split(','):
        res['scan'] = {}
        for kind in (3, 4, 5):
            leg = {}
            for name, make, n_ch in (('tpc_494ch', W.mixed_config, 494), ('veto_120ch', W.nveto_config, 120)):
                cfg = make(seed=3, enable_noise=True, noise_model=models(n_ch)[kind])
                eng = Engine(cfg, Resource(cfg))
                eng.set_lone_noise_hits(True)           # (the switch alone: the veto configuration's right_raw_extension is below RawData's bound)
                assert eng.dark_count_rate is None
                leg[name] = time_scan(eng, n_ch, args.repeats)
                eng.close()
            leg['row_empty_ns_per_sample'] = time_row_empty(models(494)[kind], args.repeats, 10000)
            leg['scan_over_row_empty_tpc'] = leg['tpc_494ch']['scan_ns_per_sample']['median'] / leg['row_empty_ns_per_sample']['median']
            res['scan'][f'kind_{kind}'] = leg
    if 'mixed' in args.legs.split(','):
        ins = W.mixed_batch(args.instructions)
        res['mixed'] = dict(instructions=len(ins))
        for name, keys in (('off', {}), ('dark_count_lone_hits', dict(dark_count_lone_hits=True)), ('noise_lone_hits', dict(noise_lone_hits=True)),
                           ('both', dict(dark_count_lone_hits=True, noise_lone_hits=True))):
            cfg = W.mixed_config(seed=3, dark_count_rate=40.0, noise_model={'sigma': 2.2}, **keys)
            rd = wfsim_amd.RawData(cfg, resource=Resource(cfg))
            secs, n_rec, n_lone = [], 0, 0
            for _ in range(args.repeats + 1):           # (the first run warms up and is dropped)
                t0 = time.perf_counter()
                n_rec = n_lone = 0
                for b in rd.iter_batches(ins):
                    n_rec += int(b['first'][-1])
                    n_lone += len(b.get('lone_records', ()))
                secs.append(time.perf_counter() - t0)
            res['mixed'][name] = dict(seconds=secs[1:], records=n_rec, lone_records=n_lone)
            rd.engine.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
