"""Side benchmark: what PMT dark counts cost (config 'dark_count_rate'), and that switched off they cost nothing.

The headline batch (workloads.bench_config, 10^3 S2 of 10^4 electrons) and the mixed batch (workloads.mixed_config, S1 + S2 pairs, PMT
afterpulses and noise on) through three engines each: ``off`` (no key), ``100Hz`` (every PMT at 100 Hz) and ``limit`` (every PMT at
the largest rate the setter takes, 1/8 photon per cell of 64 samples: 195 kHz at 10 ns samples).  Prints one JSON line: ms per step of
each (several repeats) and, from one profiled step (wfs_kernel_times), the time of the kernels that finish rows.

``--root DIR`` imports the package from another checkout of the project -- the parent commit, built there -- for the comparison of
the off path: ``--variants off`` touches nothing the parent lacks.  Run the two alternately, several times each, on one machine; the
spread of the parent's own repeats is the yardstick.

usage: python tools/bench_dark_counts.py [--workloads s2,mixed] [--variants off,100Hz,limit] [--steps 10] [--warmup 3] [--repeats 3]
                                         [--root DIR] [--out profiles/dark_counts.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROW_KERNELS = ('k_zle', 'k_pack', 'k_row_pulse', 'k_pack_res', 'k_row_empty')
CELL_NS = 64 * 10           # a cell of 64 samples of 10 ns


def make(W, workload, n, **overrides):
    from wfsim_amd.engine import Engine
    from wfsim_amd.physics import instruction_params
    from wfsim_amd.resource import Resource
    from wfsim_amd.scheduler import schedule
    if workload == 's2':
        cfg, ins = W.bench_config(seed=3, **overrides), W.s2_batch(n)
    else:
        cfg, ins = W.mixed_config(seed=3, **overrides), W.mixed_batch(n)
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    eng = Engine(cfg, res)
    ip = instruction_params(ins[order], cfg, res, device_maps=eng.device_maps)
    eng.load_instructions(ins[order], order.astype(np.uint32), cluster, key, ip)
    return eng


def timed(eng, steps, warmup, repeats):
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
    ap.add_argument('--workloads', default='s2,mixed')
    ap.add_argument('--variants', default='off,100Hz,limit')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--root', default=None, help='checkout to import wfsim_amd from (default: this one)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  (torch.cuda before the library, engine.load_library)
    from wfsim_amd import workloads as W
    rates = {'off': None, '100Hz': 100.0, 'limit': 0.125 / (CELL_NS * 1e-9)}
    res = dict(root=args.root or '.', steps=args.steps, warmup=args.warmup, repeats=args.repeats)
    for workload in args.workloads.split(','):
        n = 1000 if workload == 's2' else 10000
        res[workload] = dict(instructions=n)
        for name in args.variants.split(','):
            ov = {} if rates[name] is None else dict(dark_count_rate=rates[name])
            eng = make(W, workload, n, **ov)
            assert name == 'off' or eng.dark_count_rate is not None
            ms, c = timed(eng, args.steps, args.warmup, args.repeats)
            eng.set_profiling(True)
            eng.run()
            kt = eng.kernel_times()
            eng.set_profiling(False)
            res[workload][name] = dict(ms_per_step=[round(x, 3) for x in ms], records=int(c['n_records']), intervals=int(c['n_intervals']),
                                       rows=int(c['n_rows']), kernels_ms={k: round(kt[k][0], 4) for k in ROW_KERNELS if k in kt},
                                       row_kernels_ms=round(sum(kt[k][0] for k in ROW_KERNELS if k in kt), 4),
                                       all_kernels_ms=round(sum(v[0] for v in kt.values()), 3))
            eng.close()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
