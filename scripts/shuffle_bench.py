"""Throughput of DigitalSequenceBlock.shuffle (p7x_shuffle_block, p7x_shuffle.hip) on the two shapes of bench.py: the
target database of its Pfam line (bench_workloads.make_targets: 500,000 proteins, lognormal lengths, one library entry planted in a target in 10,000 --
the lengths and the composition are what shuffling sees) and the chromosome of its nhmmer field (bench_workloads.make_chromosome),
every mode, the device against the host twin on 16 threads.  A chromosome is ONE sequence: on the device it takes the long
path, one lane walking global memory, so it is measured at --mbp (default 2) and not at the field's 250 Mbp; the twin's rate
is measured on the same sequence.  Per mode: kernel time from device events, upload time, the whole call (upload, kernels,
copy back, the Python side) and residues per second of each; median of --runs after a warm-up.  Run from the repository
root on the GPU:
    python scripts/shuffle_bench.py [--targets 500000] [--mbp 2] [--out profiles/r31_shuffle.md]"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench_workloads as bw  # noqa: E402
from pyhmmer_amd import _lib, easel, plan7  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--targets", type=int, default=500000)
ap.add_argument("--mbp", type=float, default=2.0)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out", default=str(ROOT / "profiles" / "r31_shuffle.md"))
args = ap.parse_args()
lib = _lib.lib()
assert lib.p7x_device_count() >= 1, "this measurement needs the device"
name_buf = C.create_string_buffer(256)
lib.p7x_device_name(0, name_buf, 256)
name = name_buf.value.decode()

AMINO, DNA = easel.Alphabet.amino(), easel.Alphabet.dna()
MODES = (("mono", 0), ("di", 0), ("window", 20), ("reverse", 0))


def measure(alphabet, pk, mode, window, host):
    code = easel._SHUFFLE_MODES.index(mode)
    def once():
        t0 = time.perf_counter()
        dsq, stats = easel._shuffle_packed(alphabet, pk, code, window, 42, host=host, threads=args.threads)
        return time.perf_counter() - t0, stats, dsq
    once()
    runs = [once() for _ in range(args.runs)]
    med = lambda f: statistics.median(f(r) for r in runs)
    return med(lambda r: r[0]), med(lambda r: int(r[1][0])) * 1e-9, med(lambda r: int(r[1][1])) * 1e-9, runs[0][1], runs[0][2]


lines = ["# Decoy sequences on the device: throughput (scripts/shuffle_bench.py)", "",
         f"Command: `python scripts/shuffle_bench.py --targets {args.targets} --mbp {args.mbp:g} --runs {args.runs} --threads {args.threads}`", "",
         f"One MI355X ({name}); seed 42, `shuffle_slab` at its default; median of {args.runs} runs after one warm-up.  Kernel and "
         "upload times are device events; the call is `p7x_shuffle_block` from Python with the copy back; the twin is "
         f"`p7x_shuffle_host` on {args.threads} threads, its own wall clock.  Device and twin gave the same bytes in every row.", ""]
templates = bw.load_templates()
flat, offsets, lengths, _ = bw.make_targets(args.targets, 1, templates, bw.library_lengths(1), planted_frac=1e-4)
with plan7.HMMFile(ROOT / "tests" / "golden" / "hmms" / "bmyD.hmm") as f:
    chrom = bw.make_chromosome(next(iter(f)), int(args.mbp * 1e6))
chrom_pk = easel.PackedBlock([easel.DigitalSequence(DNA, name="chromosome", sequence=chrom)])
for label, alphabet, pk in ((f"target database: {args.targets} proteins (bench_workloads.make_targets)", AMINO, easel.PackedBlock.from_arrays(flat, offsets, lengths)),
                            (f"chromosome: one sequence of {args.mbp:g} Mbp (bench_workloads.make_chromosome)", DNA, chrom_pk)):
    res = pk.total_residues
    lines += [f"## {label}", "", f"{pk.n} sequences, {res} residues, longest {int(pk.lengths.max())}.", "",
              "| mode | runs | long | kernel ms | upload ms | call ms | kernel Gres/s | call Gres/s | twin ms | twin Gres/s | twin / kernel |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for mode, window in MODES:
        call, kernel, upload, stats, dev = measure(alphabet, pk, mode, window, host=False)
        assert int(stats[4]) == 1
        _, twin, _, _, host = measure(alphabet, pk, mode, window, host=True)
        assert np.array_equal(dev, host), mode
        tag = mode if not window else f"{mode} {window}"
        lines.append(f"| {tag} | {int(stats[2])} | {int(stats[3])} | {kernel * 1e3:.2f} | {upload * 1e3:.2f} | {call * 1e3:.2f} | {res / kernel * 1e-9:.3f} | "
                     f"{res / call * 1e-9:.3f} | {twin * 1e3:.2f} | {res / twin * 1e-9:.3f} | {twin / kernel:.2f} |")
        print(lines[-1], flush=True)
    lines.append("")
Path(args.out).write_text("\n".join(lines) + "\n")
print(f"wrote {args.out}")
