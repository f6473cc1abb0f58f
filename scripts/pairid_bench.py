"""Rates of the pairwise-identity unit (p7x_msapair.hip) on generated alignments: a few ancestors mutated at several rates,
a tenth of the cells gaps.  Per N x L: the kernel alone (device events; pair-cells = pairs compared x L), the C call, and
the Python method end to end (DigitalMSA.identity_filter / compute_weights("blosum"), which also turns the text rows into
codes and selects the rows kept); the host twin, one thread, on a smaller alignment for orientation.  Median of 3 after one
warm-up.  Reads nothing outside the repository.  Run from the repository root on the GPU:
python scripts/pairid_bench.py [quick]   (figures: profiles/r19_pairid.md)."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pyhmmer_amd import _lib, easel  # noqa: E402

AMINO = easel.Alphabet.amino()
QUICK = len(sys.argv) > 1 and sys.argv[1] == "quick"


def generated(n, alen, seed=1):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 20, size=(50, alen), dtype=np.uint8)
    ax = anc[rng.integers(0, 50, size=n)]
    rate = np.array([0.02, 0.1, 0.3, 0.5])[rng.integers(0, 4, size=n)]
    hit = rng.random((n, alen)) < rate[:, None]
    ax[hit] = rng.integers(0, 20, size=int(hit.sum()), dtype=np.uint8)
    ax[rng.random((n, alen)) < 0.1] = 20
    return ax


def as_msa(ax):
    sym = np.frombuffer(AMINO.symbols.encode(), dtype=np.uint8)
    n = ax.shape[0]
    return easel.DigitalMSA._from_rows([f"r{i}" for i in range(n)], [sym[r].tobytes().decode() for r in ax], [""] * n, [""] * n, alphabet=AMINO)


def c_filter(ax, maxid):
    n, alen = ax.shape
    order, keep, stats = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.uint8), np.zeros(4, dtype=np.int64)
    t0 = time.perf_counter()
    st = _lib.lib().p7x_msa_idfilter(3, ax.ctypes.data, n, alen, order.ctypes.data, maxid, 0, keep.ctypes.data, stats.ctypes.data)
    assert st == 0, _lib.last_error()
    return time.perf_counter() - t0, stats, int(keep.sum())


def c_linkage(ax, maxid):
    import ctypes as C
    n, alen = ax.shape
    cluster, ncl, stats = np.zeros(n, dtype=np.int32), C.c_int64(), np.zeros(4, dtype=np.int64)
    t0 = time.perf_counter()
    st = _lib.lib().p7x_msa_linkage(3, ax.ctypes.data, n, alen, maxid, 0, cluster.ctypes.data, C.byref(ncl), stats.ctypes.data)
    assert st == 0, _lib.last_error()
    return time.perf_counter() - t0, stats, int(ncl.value)


def median_of(call, reps=3):
    call()
    runs = [call() for _ in range(reps)]
    return runs[len(runs) // 2] if reps == 1 else sorted(runs, key=lambda r: r[0])[len(runs) // 2]


def report(label, alen, run):
    dt, stats, result = run
    cells = float(stats[0]) * alen
    line = f"  {label}: result {result}, pairs {int(stats[0])}, call {1e3 * dt:.1f} ms = {cells / dt:.3g} pair-cells/s"
    if stats[3]:
        line += f" | kernels {1e-6 * stats[1]:.2f} ms = {cells / (1e-9 * max(int(stats[1]), 1)):.3g} pair-cells/s | upload {1e-6 * stats[2]:.2f} ms"
    print(line, flush=True)


shapes = [(4000, 300)] if QUICK else [(4000, 300), (20000, 300), (50000, 300), (100000, 200), (20000, 1200)]
for n, alen in shapes:
    ax = np.ascontiguousarray(generated(n, alen))
    print(f"{n} rows x {alen} columns", flush=True)
    report("filter 0.8, C call", alen, median_of(lambda: c_filter(ax, 0.8)))
    report("filter 0.3 (few rows kept), C call", alen, median_of(lambda: c_filter(ax, 0.3)))
    report("clusters 0.62, C call", alen, median_of(lambda: c_linkage(ax, 0.62)))
    if n <= 20000:
        msa = as_msa(ax)
        for name, call in (("identity_filter(0.8, origorder)", lambda: msa.identity_filter(0.8, preference="origorder")),
                           ("identity_filter(0.8) [conscover]", lambda: msa.identity_filter(0.8)),
                           ('compute_weights("blosum")', lambda: msa.compute_weights("blosum"))):
            call()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                out = call()
                ts.append(time.perf_counter() - t0)
            stats = (out if name.startswith("identity") else msa)._pair_stats
            print(f"  {name}: {1e3 * statistics.median(ts):.1f} ms end to end = {float(stats[0]) * alen / statistics.median(ts):.3g} pair-cells/s", flush=True)

# the host twin, one thread
n, alen = 3000, 300
ax = np.ascontiguousarray(generated(n, alen))
_lib.set_debug_option("host_pairid", 1)
print(f"host twin, one thread, {n} rows x {alen} columns", flush=True)
report("filter 0.8", alen, median_of(lambda: c_filter(ax, 0.8), reps=1))
report("clusters 0.62", alen, median_of(lambda: c_linkage(ax, 0.62), reps=1))
_lib.set_debug_option("host_pairid", -1)
