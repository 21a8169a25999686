"""usage: python tools/trace_gaps.py <dir with *kernel_trace.csv>   -- per kernel: calls, mean duration; and the idle time between consecutive
dispatches on the GPU (launch gaps + host synchronisations) of the LAST batch in the trace (batches are split at k_counts, the last kernel of wfs_run).
The packers (k_pack_desc, k_pack_res, k_pack) may run on the pack stream, under the next batch: those of the batch before that lie in
this batch's span are taken off the timeline the gaps are measured on and reported on a line of their own, with the kernels they ran beside."""
import csv, glob, os, sys, collections
f = max(glob.glob(os.path.join(sys.argv[1], '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))
name = lambda r: r['Kernel_Name'].replace('void ', '').split('(')[0].split('<')[0]
start, end = lambda r: int(r['Start_Timestamp']), lambda r: int(r['End_Timestamp'])
PACKERS = ('k_pack_desc', 'k_pack_res', 'k_pack')
ends = [i for i, r in enumerate(rows) if name(r) == 'k_counts']
if len(ends) < 2:
    raise SystemExit('fewer than two batches in the trace')
batch = rows[ends[-2] + 1:ends[-1] + 1]
# the batch's own packers follow its last scan (record offsets); packers that start before it belong to the batch before, and so do
# those in front of the split whose k_pack_desc started before that batch's k_counts did
scans = [start(r) for r in batch if name(r) == 'k_scan_down']
early = [r for r in batch if name(r) in PACKERS and scans and start(r) < scans[-1]]
# (the main timeline keeps the batch's own packers only where they are serial: finished when its k_counts starts)
main = [r for r in batch if r not in early and (name(r) not in PACKERS or end(r) <= start(batch[-1]))]
t0, t1 = start(main[0]), max(end(r) for r in main)
before = [r for r in rows[(ends[-3] + 1 if len(ends) > 2 else 0):ends[-2] + 1] if name(r) in PACKERS and end(r) > t0] + early
busy = sum(end(r) - start(r) for r in main)
gaps = [(start(b) - end(a), name(a), name(b)) for a, b in zip(main[:-1], main[1:])]
print(f'last batch: {len(main)} dispatches, span {(t1 - t0) / 1e6:.3f} ms, kernels {busy / 1e6:.3f} ms, idle {(t1 - t0 - busy) / 1e6:.3f} ms')
if before:
    inside = lambda p: min(end(p), t1) - max(start(p), t0)
    beside = collections.defaultdict(int)
    for p in before:
        for r in main:
            o = min(end(p), end(r)) - max(start(p), start(r))
            if o > 0:
                beside[name(r)] += o
    tile = [start(r) for r in main if name(r) in ('k_s2_tile', 'k_s2_bright', 'k_s2_tile_gen')]
    print(f'  packers of the batch before inside this span: {sum(inside(p) for p in before) / 1e3:.1f} us ('
          + ', '.join(f'{name(p)} {inside(p) / 1e3:.1f} of {(end(p) - start(p)) / 1e3:.1f}' for p in before) + f'), the last ends {(max(end(p) for p in before) - t0) / 1e3:.1f} us into the span'
          + (f', the first tile kernel starts at {(min(tile) - t0) / 1e3:.1f} us' if tile else ''))
    print('  beside: ' + ', '.join(f'{k} {v / 1e3:.1f} us' for k, v in sorted(beside.items(), key=lambda kv: -kv[1])[:8]))
else:
    print('  packers of the batch before inside this span: none')
pub = [i for i, r in enumerate(main) if name(r) == 'k_publish']
print(f'  boundaries (k_publish): {len(pub)}, after ' + ', '.join(name(main[i - 1]) if i else '-' for i in pub))
for g, a, b in sorted(gaps, reverse=True)[:12]:
    print(f'  gap {g / 1e3:8.1f} us  after {a}  before {b}')
per = collections.defaultdict(list)
for r in batch:
    per[name(r)].append(end(r) - start(r))
for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:14]:
    print(f'  {k:24s} {len(v):3d} x {sum(v) / len(v) / 1e3:9.1f} us = {sum(v) / 1e6:7.3f} ms')
