"""Side benchmark: what digitiser noise costs on the mixed batch, three ways (config 'noise_model').

The mixed batch of workloads.mixed_config (S1 + S2 pairs, PMT afterpulses and noise on) through three engines:

* ``table_3000``   its 3000-sample noise table, replayed from a random offset per window (what every workload here does);
* ``table_1e6``    a 10^6-sample table of the same distribution: long enough not to repeat inside a row, 2 B of HBM per sample read;
* ``model``        noise_model = {'sigma': 2.2}: drawn per sample, no table (noise kind 3);
* ``colour_L4``, ``colour_L16``, ``colour_L4_common``, ``colour_L16_common``  the same with unit-power FIR taps of 4 / 16 samples, without and
  with one common stream shared by all channels (gain 0.5): noise kind 4, one or two streams per row;
* ``slow_1``, ``slow_8``, ``slow_8_common``, ``colour_L16_common+slow_8``  the white model with one (shift 8) or eight (shifts 4 .. 11) slow
  levels of amplitude 0.25, then with a common stream that has the eight levels too, then on top of ``colour_L16_common``: noise kind 5.

``--variants a,b`` runs a subset.  Prints one JSON line: ms per step of each (several repeats), and the per-kernel times of k_zle, k_pack, k_row_pulse and k_pack_res from
one profiled step (wfs_kernel_times).  Report only: the three compute different noise, so records and intervals differ in number.

usage: python tools/bench_noise_model.py [--instructions 10000] [--steps 10] [--warmup 3] [--variants model,colour_L4] [--out profiles/noise_model_cost.json]
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

ROW_KERNELS = ('k_zle', 'k_pack', 'k_row_pulse', 'k_pack_res')


def make(n, **overrides):
    cfg, ins = W.mixed_config(seed=3, **overrides), W.mixed_batch(n)
    res = Resource(cfg)
    order, key, cluster = schedule(ins, cfg)
    eng = Engine(cfg, res)
    ip = instruction_params(ins[order], cfg, res, device_maps=eng.device_maps)
    eng.load_instructions(ins[order], order.astype(np.uint32), cluster, key, ip)
    return eng


def long_noise(n_samples, chunk=100000):
    """workloads.synthetic_noise at length, made in chunks (a 10^6-sample array of float64 draws is 4 GB before it is rounded)"""
    return np.concatenate([W.synthetic_noise(seed=5 + k, n_samples=min(chunk, n_samples - k * chunk)) for k in range((n_samples + chunk - 1) // chunk)])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instructions', type=int, default=10000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--variants', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (torch.cuda before the library, engine.load_library)
    variants = [('table_3000', {}),
                ('table_1e6', dict(noise_data=long_noise(10 ** 6))),
                ('model', dict(noise_model={'sigma': 2.2}))]
    from wfsim_amd.noise_model import unit_power
    n_ch = len(W.mixed_config(seed=3)['gains'])
    for L in (4, 16):
        taps = unit_power(np.hanning(L + 2)[1:-1])
        common = dict(groups=np.zeros(n_ch, dtype=np.int64), gain=0.5, sigma=2.2, taps=taps)
        variants += [(f'colour_L{L}', dict(noise_model={'sigma': 2.2, 'taps': taps})),
                     (f'colour_L{L}_common', dict(noise_model={'sigma': 2.2, 'taps': taps, 'common': common}))]
    slow8 = dict(shifts=list(range(4, 12)), amplitude=[0.25] * 8)
    variants += [('slow_1', dict(noise_model={'sigma': 2.2, 'slow': dict(shifts=[8], amplitude=[0.25])})),
                 ('slow_8', dict(noise_model={'sigma': 2.2, 'slow': slow8})),
                 ('slow_8_common', dict(noise_model={'sigma': 2.2, 'slow': slow8, 'common': dict(groups=np.zeros(n_ch, dtype=np.int64), gain=0.5, sigma=2.2,
                                                                                                   slow=[0.25] * 8)})),
                 ('colour_L16_common+slow_8', dict(noise_model={'sigma': 2.2, 'taps': taps, 'slow': slow8, 'common': dict(common, slow=[0.25] * 8)}))]
    if args.variants:
        variants = [v for v in variants if v[0] in args.variants.split(',')]
    res = dict(workload='mixed', instructions=args.instructions, steps=args.steps, warmup=args.warmup)
    for name, ov in variants:
        eng = make(args.instructions, **ov)
        assert (eng.noise_model is not None) == (not name.startswith('table')) and (eng.noise_colour is not None) == (name.startswith('colour') or 'common' in name)
        assert (eng.noise_slow is not None) == ('slow' in name)
        ms, c = timed(eng, args.steps, args.warmup)
        eng.set_profiling(True)
        eng.run()
        kt = eng.kernel_times()
        eng.set_profiling(False)
        res[name] = dict(ms_per_step=[round(x, 3) for x in ms], records=int(c['n_records']), intervals=int(c['n_intervals']),
                         raw_samples=int(c['n_raw_samples']), rows=int(c['n_rows']),
                         kernels_ms={k: round(kt[k][0], 4) for k in ROW_KERNELS if k in kt},
                         all_kernels_ms=round(sum(v[0] for v in kt.values()), 3))
        eng.close()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
