"""Side benchmark: what lone-hit rows cost (config 'dark_count_lone_hits').

1. ``Engine.lone_hits`` over one simulated second (10^8 samples of 10 ns) against no rows: 494 TPC channels at 40 Hz and 120 veto
   channels at 1 kHz.  Reports ms per simulated second, cells (64 samples of a channel) per second, and that rate against one Philox
   call per cell at the rate ``k_row_empty<3>`` makes its calls (0.0020 ns per sample, a call per four samples).
2. The mixed workload (workloads.mixed_config / mixed_batch: S1 + S2 pairs 1 ms apart, PMT afterpulses and noise on) through
   ``RawData.iter_batches`` at 40 Hz per tube with the key off and on: seconds per run, records of either kind.

Prints one JSON line.

usage: python tools/bench_lone_hits.py [--repeats 3] [--instructions 2000] [--out profiles/lone_hits.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

SECOND = 10 ** 8                                    # samples of 10 ns
ROW_EMPTY3_CALLS_PER_S = 1.0 / (4 * 0.0020e-9)      # Philox calls per second of k_row_empty<3>


def time_pass(eng, repeats):
    eng.lone_hits(0, SECOND // 100)                 # (buffers and code objects)
    ms, n = [], 0
    for _ in range(repeats):
        t0 = time.perf_counter()
        rec = eng.lone_hits(0, SECOND)
        ms.append(1e3 * (time.perf_counter() - t0))
        n = len(rec)
    return ms, n, len(eng.lone_hit_rows())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--instructions', type=int, default=2000, help='instructions of the mixed run (1 ms per pair: 2000 are a simulated second)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  (torch.cuda before the library, engine.load_library)
    import wfsim_amd
    from wfsim_amd import workloads as W
    from wfsim_amd.engine import Engine
    from wfsim_amd.resource import Resource
    res = dict(repeats=args.repeats, simulated_second_samples=SECOND, row_empty3_calls_per_s=ROW_EMPTY3_CALLS_PER_S)
    for name, cfg in (('tpc_494ch_40Hz', W.mixed_config(seed=3, dark_count_rate=40.0)),
                      ('veto_120ch_1kHz', W.nveto_config(seed=3, dark_count_rate=1000.0))):
        eng = Engine(cfg, Resource(cfg))
        n_ch = len(eng.dark_count_rate)
        ms, n_rec, n_rows = time_pass(eng, args.repeats)
        cells = n_ch * (SECOND // 64)
        best = min(ms)
        res[name] = dict(channels=n_ch, ms_per_simulated_second=ms, cells=cells, cells_per_s=cells / (best * 1e-3), records=n_rec, rows=n_rows,
                         of_one_philox_call_per_cell=cells / (best * 1e-3) / ROW_EMPTY3_CALLS_PER_S)
        eng.close()
    ins = W.mixed_batch(args.instructions)
    res['mixed'] = dict(instructions=len(ins))
    for key in (False, True):
        cfg = W.mixed_config(seed=3, dark_count_rate=40.0, dark_count_lone_hits=key)
        rd = wfsim_amd.RawData(cfg, resource=Resource(cfg))
        secs, n_rec, n_lone = [], 0, 0
        for _ in range(args.repeats + 1):           # (the first run warms up and is dropped)
            t0 = time.perf_counter()
            n_rec = n_lone = 0
            for b in rd.iter_batches(ins):
                n_rec += int(b['first'][-1])
                n_lone += len(b.get('lone_records', ()))
            secs.append(time.perf_counter() - t0)
        res['mixed']['on' if key else 'off'] = dict(seconds=secs[1:], records=n_rec, lone_records=n_lone)
        rd.engine.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
