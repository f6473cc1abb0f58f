"""Sequences and residues per second of the device emitter (p7x_emit_block) for 500,000 sequences from KR.hmm (262 nodes,
amino) and from bmyD.hmm (1,203 nodes, DNA), and for comparison from PF02826's first 100 nodes (tables staged in LDS, and
the same through L2), beside the host twin on 16 threads.  Kernel time is from device events around the emit kernel's
launches; call time is the whole C call (tables up, both passes, scan, compaction, the packed block down).  Median of 5
runs after one warm-up.  Run from the repository root on the GPU: python scripts/emit_throughput.py
(figures: profiles/r18_emit.md)."""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pyhmmer_amd import _lib, plan7  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 500000
lib = _lib.lib()


def load(name):
    with plan7.HMMFile(ROOT / "tests" / "golden" / "hmms" / f"{name}.hmm") as f:
        return next(iter(f))


def head(hmm, M):
    """The first M nodes of a model as a model of its own (node M closed as the last node of a model is)."""
    cut = plan7.HMM(hmm.alphabet, M, f"{hmm.name}[1..{M}]")
    cut.transition_probabilities[:] = hmm.transition_probabilities[:M + 1]
    cut.match_emissions[:] = hmm.match_emissions[:M + 1]
    cut.insert_emissions[:] = hmm.insert_emissions[:M + 1]
    t = cut.transition_probabilities
    t[M, 0], t[M, 2] = t[M, 0] + t[M, 2], 0.0
    t[M, 5], t[M, 6] = 1.0, 0.0
    return cut


def run(em, device, threads=16):
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = lib.p7x_emit_block(em.handle, 0, N, 42, 0, C.byref(h)) if device else lib.p7x_emit_block_host(em.handle, N, 42, 0, threads, C.byref(h))
    dt = time.perf_counter() - t0
    assert rc == 0, _lib.last_error()
    out = (dt, lib.p7x_emitted_info(h, 6) * 1e-6, lib.p7x_emitted_info(h, 1), lib.p7x_emitted_info(h, 3), lib.p7x_emitted_info(h, 2))
    lib.p7x_emitted_destroy(h)
    return out


def report(label, em, device):
    run(em, device)
    runs = [run(em, device) for _ in range(5)]
    call = statistics.median(r[0] for r in runs)
    nres, redrawn, cap = runs[0][2], runs[0][3], runs[0][4]
    line = f"{label}: {N} sequences, {nres} residues, slots of {cap}, {redrawn} redrawn | call {1e3 * call:.1f} ms = {N / call:.3g} seq/s, {nres / call:.3g} res/s"
    if device:
        kern = max(statistics.median(r[1] for r in runs), 1e-9)
        line += f" | kernel {1e3 * kern:.2f} ms = {N / kern:.3g} seq/s, {nres / kern:.3g} res/s (runs: " + " ".join(f"{1e3 * r[1]:.2f}" for r in runs) + ")"
    print(line, flush=True)


for name, hmm in (("KR (262 nodes, amino)", load("KR")), ("bmyD (1,203 nodes, DNA)", load("bmyD")),
                  ("PF02826[1..100] (100 nodes, amino)", head(load("PF02826"), 100))):
    em = hmm._emit_model()
    report(f"{name} device", em, True)
    if "PF02826" in name:
        _lib.set_debug_option("emit_lds", 0)
        report(f"{name} device, tables through L2", em, True)
        _lib.set_debug_option("emit_lds", -1)
    report(f"{name} host twin, 16 threads", em, False)
