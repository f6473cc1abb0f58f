"""Viterbi filter alone on models beyond 640 nodes: one synthetic profile of each length against 200,000 synthetic 300-aa
targets through SequenceDatabase.filters(viterbi=True), every target scored, nothing else on the device; one untimed call
and five timed ones per model.  Run it under rocprofv3 --kernel-trace and read the kernels' own durations back:

  rocprofv3 --kernel-trace --stats -d DIR -o alone -- python scripts/vit_wide_alone.py 1000 2000
  python scripts/vit_wide_alone.py --db DIR/.../alone_results.db

The second form prints, per Viterbi kernel, the median of the last five dispatches.  The wall-clock times the first form
prints include the copy of the scores to the host.  Option "vit_wide" is left alone: compare two builds, not two settings."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

if len(sys.argv) > 2 and sys.argv[1] == "--db":
    import sqlite3, statistics
    by = {}
    for name, dur in sqlite3.connect(sys.argv[2]).execute("select name, duration from kernels where name like '%vit%' order by start"):
        by.setdefault(name, []).append(dur / 1e6)
    for name, d in by.items():
        print(f"{name}: {len(d)} dispatches, median of the last five {statistics.median(d[-5:]):.3f} ms, all {[round(x, 3) for x in d]}")
    sys.exit(0)

import numpy as np
import bench, bench_workloads as bw
from pyhmmer_amd import plan7
Ms = [int(x) for x in sys.argv[1:]] or [1000, 2000]
templates = bw.load_templates()
bg = plan7.Background(templates[0].alphabet)
flat, offsets, lengths, planted = bench.make_workload(templates[0], 200_000, 300, seed=42)
db = plan7.SequenceDatabase.from_packed(templates[0].alphabet, flat, offsets, lengths, device=0)
for M in Ms:
    om = plan7.OptimizedProfile(bw.make_entry(templates, 3, M), bg, 300)
    ms, xc = [], None
    for rep in range(6):
        t0 = time.perf_counter()
        xc = db.filters(om, msv=False, viterbi=True)["xC"]
        ms.append(1e3 * (time.perf_counter() - t0))
    t = float(np.median(ms[1:]))
    cells = float(np.sum(lengths)) * M
    print(f"M {M:5d}: filters(viterbi) {t:8.2f} ms (median of five, wall clock) = {cells / t / 1e6:8.1f} GCUPS; checksum {int(xc.astype(np.int64).sum())}", flush=True)
