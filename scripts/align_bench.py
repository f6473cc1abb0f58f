"""hmmalign throughput: one model against N sequences, traces on the device (p7x_align.hip, wall time of
TraceAligner.compute_traces with the upload and the host's repeats of flagged sequences) and by the host twin in
upstream's order (test seam host_align = 1, 16 worker threads).  GCUPS = M x (sum of sequence lengths) / time.
usage: align_bench.py [--hmm tests/golden/hmms/KR.hmm] [--n 2100] [--reps 3] [--host-threads 16]
Sequences: the fixture proteome (tests/golden/seqs/938293...faa), repeated to N."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyhmmer_amd import _lib, easel, plan7

ap = argparse.ArgumentParser()
ap.add_argument("--hmm", default=os.path.join(ROOT, "tests", "golden", "hmms", "KR.hmm"))
ap.add_argument("--n", type=int, default=2100)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-threads", type=int, default=16)
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()

hmm = next(iter(plan7.HMMFile(args.hmm)))
with easel.SequenceFile(os.path.join(ROOT, "tests", "golden", "seqs", "938293.PRJEB85.HG003687.faa"), digital=True,
                        alphabet=hmm.alphabet) as f:
    prot = list(f.read_block())
seqs = easel.DigitalSequenceBlock(hmm.alphabet, [prot[i % len(prot)] for i in range(args.n)])
cells = hmm.M * sum(len(s) for s in seqs)
aligner = plan7.TraceAligner(cpus=args.host_threads)


def best(fn):
    fn()                                                   # warm-up: device context, kernel load, host pool
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


t_dev, tr = best(lambda: aligner.compute_traces(hmm, seqs))
print(f"{hmm.name} M={hmm.M} n={len(seqs)} residues={cells // hmm.M}: device {t_dev * 1e3:.1f} ms = {cells / t_dev / 1e9:.1f} GCUPS "
      f"(flagged -> host twin {tr.nflagged})", flush=True)
if not args.no_host:
    _lib.set_debug_option("host_align", 1)
    try:
        t_host, _ = best(lambda: aligner.compute_traces(hmm, seqs))
    finally:
        _lib.set_debug_option("host_align", -1)
    print(f"{hmm.name}: host twin ({args.host_threads} threads) {t_host * 1e3:.1f} ms = {cells / t_host / 1e9:.2f} GCUPS; "
          f"device / host {t_host / t_dev:.1f}x", flush=True)
