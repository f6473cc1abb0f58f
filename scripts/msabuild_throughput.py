"""Time of the passes of Builder.build_msa over a deep alignment: an emit_alignment of PF02826 whose rows are repeated to
N rows (default 100,000; the columns and the gap pattern are those of the 3,000 sampled rows).  Device: the upload and the
four kernels from device events, and the whole call; host twin (up to 16 threads): its four passes by the wall clock, and
the whole call.  Median of 5 runs (3 from a million rows on) after one warm-up; the achieved share of HBM bandwidth counts the N x L bytes each pass reads.  Run from the repository root on the
GPU: python scripts/msabuild_throughput.py [N]   (figures: profiles/r18_msabuild.md)."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pyhmmer_amd import _lib, easel, plan7  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
HBM = 8.0e12            # bytes per second, MI355X peak

with plan7.HMMFile(ROOT / "tests" / "golden" / "hmms" / "PF02826.hmm") as f:
    hmm = next(iter(f))
base = hmm.emit_alignment(3000, easel.Randomness(7))
rows = [base._rows[i % 3000] for i in range(N)]
msa = easel.DigitalMSA._from_rows([f"r{i}" for i in range(N)], rows, [""] * N, [""] * N, alphabet=hmm.alphabet)
msa.name = "deep"
builder = plan7.Builder(hmm.alphabet)
L = len(msa)
print(f"{N} rows x {L} columns = {N * L / 1e6:.1f} MB", flush=True)


def run(host):
    _lib.set_debug_option("host_build", 1 if host else -1)
    t0 = time.perf_counter()
    c = builder._msa_counts(msa)
    dt = time.perf_counter() - t0
    _lib.set_debug_option("host_build", -1)
    return dt, c.upload_ns, c.kernel_ns, c.M


# the Python side (text rows to codes) is outside the C call but inside dt: measured apart
t0 = time.perf_counter()
msa._codes()
print(f"rows to codes (Python): {1e3 * (time.perf_counter() - t0):.1f} ms", flush=True)
REPS = 5 if N < 1000000 else 3
for label, host, reps in (("device", False, REPS), ("host twin, 16 threads", True, REPS)):
    run(host)
    runs = [run(host) for _ in range(reps)]
    call = statistics.median(r[0] for r in runs)
    line = f"{label}: M {runs[0][3]}, call (with rows to codes) {1e3 * call:.1f} ms"
    ks = [statistics.median(r[2][i] for r in runs) * 1e-9 for i in range(4)]
    if not host:
        up = statistics.median(r[1] for r in runs) * 1e-9
        line += f" | upload {1e3 * up:.2f} ms ({N * L / up / 1e9:.1f} GB/s)"
    for name, k in zip(("column counts", "weights", "weighted counts", "transitions"), ks):
        line += f" | {name} {1e3 * k:.3f} ms" + (f" ({N * L / max(k, 1e-12) / HBM * 100:.1f} % of HBM)" if not host else "")
    line += f" | passes {1e3 * sum(ks):.2f} ms"
    print(line, flush=True)
