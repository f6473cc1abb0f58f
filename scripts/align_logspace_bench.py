"""hmmalign's float64 log-space path: a block of three-copy KR-prefix tandems through the device kernel (p7x_alignlog.hip) and
through the host log twin (seam "host_align" = 1) on <cpus> threads.  Prints both times and the flagged share.

    python scripts/align_logspace_bench.py [--n 256] [--cpus 16] [--repeat 3]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import tandem_targets as T  # noqa: E402
from pyhmmer_amd import _lib, plan7  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    hmm = T.model("KR")
    piece = T.consensus(hmm)[:T.PREFIX_NODES]
    named = [(f"tandem{r}", T._tandem(np.random.default_rng([7, r]), [piece] * 3)) for r in range(args.n)]
    block = T.block(hmm.alphabet, named)
    aligner = plan7.TraceAligner(cpus=args.cpus, logspace=True)

    def timed(label):
        best, traces = None, None
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            traces = aligner.compute_traces(hmm, block)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print(f"[align-logspace] {label}: {args.n} sequences of {len(named[0][1])} residues, M = {hmm.M}: best of {args.repeat} "
              f"{best * 1e3:.1f} ms; nlogspace {traces.nlogspace}, flagged {traces.nlogspace_flagged}, device traces {traces.ndevice}, "
              f"rounds {traces.rounds}, workspace {traces.workspace_bytes / 1e6:.0f} MB", flush=True)
        return traces

    dev = timed("device path")
    _lib.set_debug_option("host_align", 1)
    try:
        host = timed(f"host log twin on {args.cpus} threads")
    finally:
        _lib.set_debug_option("host_align", -1)
    same = sum(1 for d, h in zip(dev, host) if np.array_equal(d.st, h.st) and np.array_equal(d.k, h.k) and np.array_equal(d.i, h.i))
    print(f"[align-logspace] traces equal to the twin's: {same} of {args.n}")


if __name__ == "__main__":
    main()
