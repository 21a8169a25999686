"""Side benchmark: what the bottom-array sum channel (config 'emit_sum_signal') costs on the headline S2 batch and on the mixed batch.

Per workload, the same loaded batch through four engines: switch off; switch on; switch on with k_sum_signal skipped
(WFS_SUM_SKIP_KERNEL: what is left is the loss of resident bottom rows and one more row per window through ZLE and packing); and
row_resident = 0 with the switch off (every row through the accumulators).  Prints one JSON line per workload: ms per step of each,
k_sum_signal's own time (wfs_kernel_times), the bytes it moves and the fraction of the device-copy bandwidth that is.

usage: python tools/bench_sum_signal.py [--steps 10] [--warmup 3] [--out profiles/sum_signal.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wfsim_amd import workloads as W                          # noqa: E402
from wfsim_amd.config import kernel_params                    # noqa: E402
from wfsim_amd.engine import Engine                           # noqa: E402
from wfsim_amd.physics import instruction_params              # noqa: E402
from wfsim_amd.resource import Resource                       # noqa: E402
from wfsim_amd.scheduler import schedule                      # noqa: E402


def make(workload, n, debug=False, **overrides):
    if workload == 's2':
        cfg, ins = W.bench_config(seed=3, **overrides), W.s2_batch(n)
    else:
        cfg, ins = W.mixed_config(seed=3, **overrides), W.mixed_batch(n)
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    eng = Engine(cfg, res)
    ip = instruction_params(ins[order], cfg, res, device_maps=eng.device_maps)
    eng.load_instructions(ins[order], order.astype(np.uint32), cluster, key, ip)
    if debug:
        eng.set_debug(True)
    return eng, cfg


def timed(eng, steps, warmup, repeats=3):
    out = []
    for _ in range(repeats):
        for _ in range(warmup):
            eng.run()
        t0 = time.perf_counter()
        for _ in range(steps):
            c = eng.run()                 # (ends with a read-back of the batch's counters: the stream is idle when it returns)
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return out, c


def copy_bandwidth():
    """device-to-device copy of 1 GiB: bytes read + written per second"""
    import torch
    a = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    b = torch.empty_like(a)
    b.copy_(a); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        b.copy_(a)
    torch.cuda.synchronize()
    return 2 * 5 * (1 << 30) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (torch.cuda before the library, engine.load_library)
    bw = copy_bandwidth()
    lines = []
    for workload, n in (('s2', 1000), ('mixed', 10000)):
        # share of the bottom rows among the samples of all rows, from a small batch with the finished rows kept
        small, cfg = make(workload, max(n // 50, 4), debug=True, row_resident=0)
        small.run()
        r, p = small.rows(), kernel_params(cfg)
        length = r['right'] - r['left'] + 1
        bottom = (r['channel'] >= p['n_top']) & (r['channel'] <= p['last_bottom'])
        share = float(length[bottom].sum() / max(length.sum(), 1))
        small.close()
        res = dict(workload=workload, instructions=n, copy_bandwidth_GBs=round(bw / 1e9, 1), bottom_share_of_samples=round(share, 4))
        variants = [('off', {}, False), ('on', dict(emit_sum_signal=True), False), ('on_kernel_skipped', dict(emit_sum_signal=True), True),
                    ('off_row_resident_0', dict(row_resident=0), False), ('on_row_resident_0', dict(emit_sum_signal=True, row_resident=0), False)]
        for name, ov, skip in variants:
            os.environ.pop('WFS_SUM_SKIP_KERNEL', None)
            if skip:
                os.environ['WFS_SUM_SKIP_KERNEL'] = '1'
            eng, _ = make(workload, n, **ov)
            ms, c = timed(eng, args.steps, args.warmup)
            res[name + '_ms'] = [round(x, 3) for x in ms]
            res[name + '_raw_samples'] = int(c['n_raw_samples'])
            if name == 'on':
                eng.set_profiling(True)
                eng.run()
                kt = eng.kernel_times()
                eng.set_profiling(False)
                res['k_sum_signal_ms'] = round(kt['k_sum_signal'][0], 4)
                res['kernels_on_ms'] = {k: round(v[0], 3) for k, v in sorted(kt.items(), key=lambda kv: -kv[1][0])[:8]}
            eng.close()
        os.environ.pop('WFS_SUM_SKIP_KERNEL', None)
        s_sum = res['on_row_resident_0_raw_samples'] - res['off_row_resident_0_raw_samples']
        read = share * res['off_row_resident_0_raw_samples'] * 4
        res['sum_samples'] = s_sum
        res['k_sum_signal_bytes'] = dict(read=int(read), written=int(4 * s_sum))
        res['k_sum_signal_GBs'] = round((read + 4 * s_sum) / (res['k_sum_signal_ms'] * 1e-3) / 1e9, 1)
        res['fraction_of_copy_bandwidth'] = round(res['k_sum_signal_GBs'] * 1e9 / bw, 3)
        lines.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == '__main__':
    main()
