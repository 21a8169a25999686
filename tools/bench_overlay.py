"""Side benchmark: what the overlay pass costs (config 'overlay_records'), and that the key changes nothing when absent.

1. ``steps``: the headline step (``bench.py --workload s2``) and the mixed step (``--workload mixed``) with the key absent, each run
   ``--repeats`` times in a process of its own; ms per step of every run.  ``--root DIR`` takes bench.py and the package from another
   checkout of the project -- the parent commit, built there -- on the same machine; run the two alternately.  ``--parent-json`` names
   results of this leg on the parent: the verdict ``inside_parent_spread`` compares the median of this checkout's repeats with the
   minimum and maximum of the parent's own, and both lists are recorded.
2. ``pass``: one mixed batch on an engine, then ``Engine.overlay_records`` against the records of that run where the device holds them,
   with 0, 10^4 and 10^6 background records: pulses of 1 .. 3 fragments placed uniformly over the batch's time span on the TPC
   channels, no two of a channel sharing a sample.  Wall time of the pass (upload of the background and copy of the output included),
   the kernels' own time from the profiling timers (the three radix sorts and three scans between them are rocPRIM's and are not
   bracketed), records in and out.  Measured, not promised.

Prints one JSON line.

usage: python tools/bench_overlay.py [--legs steps,pass] [--repeats 3] [--steps 10] [--warmup 3] [--root DIR] [--parent-json f[,g]] [--out profiles/overlay.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(x):
    return dict(min=float(np.min(x)), median=float(np.median(x)), max=float(np.max(x)), all=[float(v) for v in x])


def bench_steps(root, workload, repeats, steps, warmup):
    out = []
    for _ in range(repeats):
        q = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--workload', workload,
                            '--cpu-sample', '0'], cwd=root, capture_output=True, text=True, timeout=900)
        if q.returncode != 0:
            raise RuntimeError(f'bench.py --workload {workload} failed ({q.returncode}): {q.stderr[-2000:]}')
        line = [ln for ln in q.stdout.splitlines() if ln.startswith('{')][-1]
        out.append(json.loads(line)['ms_per_step'])
    return out


def background(rng, n_records, n_ch, s_lo, s_hi, baseline, dt):
    """about n_records background records: per channel its share of pulses of 1 .. 3 fragments, laid one behind the other with random gaps
    (no two share a sample), spread over [s_lo, s_hi)"""
    from wfsim_amd.overlay import DTYPE, sort_records
    if n_records == 0:
        return np.zeros(0, dtype=DTYPE)
    per_ch = max(n_records // (2 * n_ch), 1)                 # (two records per pulse on average)
    span = s_hi - s_lo
    parts = []
    for ch in range(n_ch):
        length = rng.choice([60, 110, 170, 220, 300], size=per_ch)
        room = span - int(length.sum())
        if room <= per_ch:
            raise ValueError('the batch spans too few samples for that many background pulses per channel')
        gaps = np.diff(np.sort(rng.integers(0, room, size=per_ch)), prepend=0) + 1
        start = s_lo + np.cumsum(gaps) + np.concatenate([[0], np.cumsum(length)[:-1]])
        nfrag = (length + 109) // 110
        n = int(nfrag.sum())
        rec = np.zeros(n, dtype=DTYPE)
        pulse = np.repeat(np.arange(per_ch), nfrag)
        f = np.arange(n) - np.repeat(np.cumsum(nfrag) - nfrag, nfrag)
        rec['time'], rec['dt'], rec['channel'] = (start[pulse] + 110 * f) * dt, dt, ch
        rec['pulse_length'], rec['record_i'] = length[pulse], f
        rec['length'] = np.minimum(length[pulse] - 110 * f, 110)
        rec['data'] = baseline + rng.integers(-3, 4, size=(n, 110))
        rec['data'][np.arange(110)[None, :] >= rec['length'][:, None]] = 0
        parts.append(rec)
    return sort_records(np.concatenate(parts))


def bench_pass(repeats, instructions):
    import torch  # noqa: F401  (torch.cuda before the library, engine.load_library)
    from wfsim_amd import workloads as W
    from wfsim_amd.engine import Engine
    from wfsim_amd.physics import instruction_params
    from wfsim_amd.resource import Resource
    from wfsim_amd.scheduler import schedule
    cfg = W.mixed_config(seed=3)
    res = Resource(cfg)
    ins = W.mixed_batch(instructions)
    order, key, cluster = schedule(ins, cfg)
    eng = Engine(cfg, res)
    ip = instruction_params(ins[order], cfg, res, device_maps=eng.device_maps)
    eng.load_instructions(ins[order], order.astype(np.uint32), cluster, key, ip)
    counts = eng.run()
    own = eng.records()
    p = eng.params
    s_lo, s_hi = int(own['time'].min()) // p['dt'], int(own['time'].max()) // p['dt'] + 110
    out = dict(instructions=len(ins), simulated_records=int(counts['n_records']), span_samples=s_hi - s_lo, rates={})
    rng = np.random.default_rng(5)
    for n_bg in (0, 10 ** 4, 10 ** 6):
        bg = background(rng, n_bg, int(p['n_tpc']), s_lo, s_hi, int(p['baseline']), int(p['dt']))
        merged = eng.overlay_records(bg)                     # (buffers and code objects)
        wall, kern = [], []
        for _ in range(repeats):
            eng.run()                                        # (the timers of the passes add up until the next run)
            eng.set_profiling(True)
            t0 = time.perf_counter()
            merged = eng.overlay_records(bg)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append({k: v[0] for k, v in eng.kernel_times().items() if k.startswith('k_ov_')})
            eng.set_profiling(False)
        out['rates'][str(n_bg)] = dict(background_records=len(bg), records_out=len(merged), pass_ms=spread(wall),
                                       kernels_ms={k: spread([q.get(k, 0.0) for q in kern]) for k in sorted(kern[0])})
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='steps,pass')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--instructions', type=int, default=10000, help='instructions of the mixed batch of the pass leg')
    ap.add_argument('--root', default=HERE, help='the checkout whose bench.py and package are measured (default: this one)')
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    res = dict(repeats=args.repeats, steps=args.steps, warmup=args.warmup)
    legs = args.legs.split(',')
    if 'steps' in legs:
        for name, workload in (('headline', 's2'), ('mixed', 'mixed')):
            ms = bench_steps(root, workload, args.repeats, args.steps, args.warmup)
            res[name + '_off'] = dict(ms_per_step=ms, median_ms=float(np.median(ms)))
        if args.parent_json:
            for name in ('headline', 'mixed'):
                parent = []
                for f in args.parent_json.split(','):       # (several runs of the parent, taken before and after this one)
                    with open(f) as fh:
                        parent += json.load(fh)[name + '_off']['ms_per_step']
                res[name + '_off_parent_ms_per_step'] = parent
                res[name + '_off_inside_parent_spread'] = bool(min(parent) <= res[name + '_off']['median_ms'] <= max(parent))
    if 'pass' in legs:
        res['pass'] = bench_pass(args.repeats, args.instructions)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
