"""MSV stage alone, one register tile at a time: one synthetic profile of each length against 1,600,000 synthetic 300-aa
targets through SequenceDatabase.filters(om, msv=True), every target scored by the lane-per-target kernel of the model's
tile, nothing else on the device; one untimed call and five timed ones per model.  (25,000 groups of 64 targets: six to
twelve per wavefront slot of the device.  200,000 targets are 3,125 groups, fewer than the 4,096 wavefronts a tier-0 launch
keeps resident: such a dispatch lasts as long as one wavefront needs for one group and says nothing about throughput;
--targets N sets the number.)  The default lengths are one per tier and
both ends of tier 0: 60, 100, 180 (R = 32, 52, 92), 262 (R = 132), 440 (R = 224), 600 (K = 2), 1020 (K = 4), 1500 (K = 8).
Run it under rocprofv3 --kernel-trace and read the kernels' own durations back:

  rocprofv3 --kernel-trace --stats -d DIR -o alone -- python scripts/msv_alone.py [--targets N] [--length L] 60 100 180
  python scripts/msv_alone.py --db DIR/.../alone_results.db

The second form prints, per MSV kernel, the median of the last five dispatches.  Counters go in runs of their own
(rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES -- python scripts/msv_alone.py ..., then
scripts/rocprof_pmc_summary.py).  The wall-clock times the first form prints include the copy of the scores to the host.
The checksum of xJ is the same for every build that computes the same scores: compare two builds, not two settings."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

if len(sys.argv) > 2 and sys.argv[1] == "--db":
    import sqlite3, statistics
    by = {}
    for name, dur in sqlite3.connect(sys.argv[2]).execute("select name, duration from kernels where name like '%msv%' order by start"):
        by.setdefault(name, []).append(dur / 1e6)
    for name, d in by.items():
        print(f"{name}: {len(d)} dispatches, median of the last five {statistics.median(d[-5:]):.3f} ms, all {[round(x, 3) for x in d]}")
    sys.exit(0)

import numpy as np
import bench, bench_workloads as bw
from pyhmmer_amd import plan7
args = sys.argv[1:]
N, L = 1_600_000, 300
if args and args[0] == "--targets":
    N, args = int(args[1]), args[2:]
if args and args[0] == "--length":       # targets of another length (290: the last tile's second half is pad in every lane)
    L, args = int(args[1]), args[2:]
Ms = [int(x) for x in args] or [60, 100, 180, 262, 440, 600, 1020, 1500]
templates = bw.load_templates()
bg = plan7.Background(templates[0].alphabet)
flat, offsets, lengths, planted = bench.make_workload(templates[0], N, L, seed=42)
db = plan7.SequenceDatabase.from_packed(templates[0].alphabet, flat, offsets, lengths, device=0)
for M in Ms:
    om = plan7.OptimizedProfile(bw.make_entry(templates, 3, M), bg, 300)
    ms, xj = [], None
    for rep in range(6):
        t0 = time.perf_counter()
        xj = db.filters(om, msv=True)["xJ"]
        ms.append(1e3 * (time.perf_counter() - t0))
    t = float(np.median(ms[1:]))
    cells = float(np.sum(lengths)) * M
    print(f"M {M:5d}: filters(msv) {t:8.2f} ms (median of five, wall clock) = {cells / t / 1e6:8.1f} GCUPS; checksum {int(xj.astype(np.int64).sum())}", flush=True)
