"""Side benchmark: BASELINE config[4] shape -- nVeto optical instructions at ~1 MHz, ~10 photons each, 120 channels -- above the engine:
(a) RawDataOptical.iter_windows (host scheduling + GPU, records per digitise window) and (b) the plugin RawRecordsFromFaxnVeto end to end
(strax_interface.py:1009-1013: chunks of raw_records_nv + truth_nv through the chunker).  Prints one JSON line; not the headline metric.

    python tools/bench_nveto.py [n] [--pmt-afterpulses] [--engine] [--tpc-s1]

--pmt-afterpulses: PMT afterpulses behind the supplied photons (the golden tables, tests/golden/pmt_ap_tables.npz, attached to the resource:
  their first 120 rows for the nVeto).  --engine: the engine step alone (one loaded batch, run repeatedly) with its kernel times, in
  place of (a) and (b).  --tpc-s1: the optical-TPC case instead of the nVeto one: 10^3 S1s x 5 000 supplied photons on 494 channels
  (engine step only)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import wfsim_amd
from wfsim_amd import ministrax
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype, optical_extra_dtype
from wfsim_amd.scheduler import schedule
from wfsim_amd.workloads import nveto_config, optical_instructions

ap = argparse.ArgumentParser()
ap.add_argument('n', nargs='?', type=int, default=None)
ap.add_argument('--pmt-afterpulses', action='store_true')
ap.add_argument('--engine', action='store_true')
ap.add_argument('--tpc-s1', action='store_true')
args = ap.parse_args()


def golden_afterpulse_tables(rows=None):
    d = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'pmt_ap_tables.npz'))
    out = {}
    for name in ['He', 'Xe', 'Uniform']:
        dc, ac = d[f'{name}_delaytime_cdf'], d[f'{name}_amplitude_cdf']
        if rows is not None:
            dc, ac = dc[:rows], (ac[:rows] if ac.ndim == 2 else ac)
        out[name] = dict(delaytime_cdf=np.ascontiguousarray(dc), amplitude_cdf=np.ascontiguousarray(ac),
                         delaytime_bin_size=float(d[f'{name}_delaytime_bin_size']), amplitude_bin_size=float(d[f'{name}_amplitude_bin_size']))
    return out


def tpc_s1_input(n, photons, seed=3):
    """n optical S1s in the TPC, 1 ms apart, `photons` supplied photons each over 494 channels, arrival times exponential with 60 ns"""
    rng = np.random.default_rng(seed)
    ins = np.zeros(n, dtype=instruction_dtype + optical_extra_dtype)
    ins['type'], ins['time'], ins['event_number'], ins['amp'] = 1, 1_000_000 * (1 + np.arange(n)), np.arange(n), photons
    ins['_last'] = photons * (1 + np.arange(n))
    ins['_first'] = ins['_last'] - photons
    return ins, rng.integers(0, 494, n * photons), rng.exponential(60, n * photons).astype(np.int64)


def engine_step(cfg, ins, channels, timings, reps=5):
    """one loaded batch run `reps` times: best wall time of a step, then the kernel times of one profiled step"""
    rd = wfsim_amd.RawDataOptical(cfg, channels=channels, timings=timings)
    eng = rd.engine
    order, key, cluster = schedule(ins, cfg)
    eng.load_optical(ins[order], order.astype(np.uint32), cluster, key, channels, timings, cfg.get('nveto_time_max_cutoff', int(1e6)))
    counts = eng.run()
    best = None
    for rep in range(reps):
        t0 = time.perf_counter()
        eng.run()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    eng.set_profiling(True)
    eng.run()
    kt = eng.kernel_times()
    top = dict(sorted(((k, round(v[0], 4)) for k, v in kt.items()), key=lambda x: -x[1])[:12])
    named = {k: round(kt[k][0], 4) for k in ('k_optical_finish', 'k_optical_ap_screen', 'k_ap_finish', 'k_ap_count', 'k_ap_place', 'k_tile_order_scan',
                                              'k_tile_order', 'k_tile_order_big', 'k_tile_order_huge') if k in kt}
    return dict(ms_per_step=round(best * 1e3, 4), photons=int(counts['n_photons']), records=int(counts['n_records']),
                boundaries=kt.get('k_publish', (0, 0))[1], kernels_ms=named, top_kernels_ms=top)


kw = dict(enable_pmt_afterpulses=True) if args.pmt_afterpulses else {}
if args.tpc_s1:
    n = args.n or 1000
    if args.pmt_afterpulses:
        kw['uniform_to_pmt_ap'] = golden_afterpulse_tables()
    ins, channels, timings = tpc_s1_input(n, 5000)
    out = dict(case='optical TPC S1', instructions=n, photons=int(len(timings)), pmt_afterpulses=args.pmt_afterpulses)
    out['engine'] = engine_step(xenonnt_test_config(seed=31, **kw), ins, channels, timings)
    print(json.dumps(out))
    sys.exit(0)

n = args.n or 200_000
if args.pmt_afterpulses:
    kw['uniform_to_pmt_ap'] = golden_afterpulse_tables(rows=120)
ins, channels, timings = optical_instructions(n, 1000.0, 3)
out = dict(instructions=n, photons=int(len(timings)), rate_hz=1e6, pmt_afterpulses=args.pmt_afterpulses)
if args.engine:
    out['engine'] = engine_step(nveto_config(seed=31, **kw), ins, channels, timings)
    print(json.dumps(out))
    sys.exit(0)

rd = wfsim_amd.RawDataOptical(nveto_config(seed=31, **kw), channels=channels, timings=timings)
list(rd.iter_windows(ins[:2000]))                         # warm-up
best = None
for rep in range(3):
    t0 = time.perf_counter()
    n_rec = n_win = 0
    for w in rd.iter_windows(ins):
        n_rec += len(w['records']); n_win += 1
    dt = time.perf_counter() - t0
    best = dt if best is None else min(best, dt)
out['rawdata_iter_windows'] = dict(seconds=round(best, 4), instructions_per_s=round(n / best), windows=n_win, records=n_rec)

best = None
for rep in range(3):
    cfg = nveto_config(seed=31, chunk_size=0.05, instructions=ins, channels=channels, timings=timings, **kw)
    plugin = wfsim_amd.RawRecordsFromFaxnVeto(cfg)
    t0 = time.perf_counter()
    res = ministrax.run_plugin(plugin)
    dt = time.perf_counter() - t0
    best = dt if best is None else min(best, dt)
    n_chunks = len(res['raw_records_nv']); n_rr = sum(len(c.data) for c in res['raw_records_nv']); n_truth = sum(len(c.data) for c in res['truth_nv'])
out['plugin_RawRecordsFromFaxnVeto'] = dict(seconds=round(best, 4), instructions_per_s=round(n / best), chunks=n_chunks, raw_records_nv=n_rr, truth_nv=n_truth)
print(json.dumps(out))
