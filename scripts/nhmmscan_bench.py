"""nhmmscan against the loop it replaces: a library of N synthetic DNA models against one target.

  (a) the only way before nhmmscan: hmmer.nhmmer per model over the same N models, eight searches in flight, the target
      resident.
  (b) hmmer.nhmmscan of the whole library, end to end (profiles and device tables of the library prepared inside).
  (c) inside (b), from the result's own timing slots (TopHits.timings_ms): the batched scan's kernel time (HIP events),
      scan + seed bookkeeping, the tails, and the scan kernel's cell rate (rows x nodes, warm-up not counted) beside the
      single-model kernel's 30.8 TCUPS on a full chromosome.

The models: lengths drawn as bench_workloads.library_lengths draws the protein library's (lognormal around 120, 20 ..
2,000); three of four are bmyD resampled to that length (9-12 score units lost per row: the maximum on every second row),
every fourth a Dirichlet-sampled model (60-110 units: the maximum on every row).  Targets: BGC0001090 (44,660 nt), the 391 kb
contig, and a 10 Mbp slice of the benchmark's synthetic chromosome.  One warm-up, then --repeats (nhmmscan) and --loop-repeats (the loop) timed
runs: median and spread [min .. max].

usage: nhmmscan_bench.py [--sizes 64 512 2048] [--targets bgc contig chr10m] [--repeats 3] [--loop-repeats 2] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import bench_workloads as bw
from conftest import random_hmm
from pyhmmer_amd import _lib, easel, hmmer, plan7

DNA = easel.Alphabet.dna()
GOLDEN = os.path.join(ROOT, "tests", "golden")


def window_length(hmm):
    view, keep = hmm._view()
    w = C.c_int32()
    assert _lib.lib().p7x_hmm_max_length(C.byref(view), 1e-7, C.byref(w)) == 0
    return int(w.value)


def resampled(tpl, M, e):
    """<tpl> resampled to M nodes (bench_workloads.make_entry's node map, no perturbation)."""
    src = np.clip(np.rint(np.arange(M + 1) * (tpl.M / M)), 1, tpl.M).astype(np.int64)
    h = plan7.HMM(tpl.alphabet, M, f"dna{e:05d}_{M}")
    h.transition_probabilities[1:] = np.asarray(tpl.transition_probabilities)[src[1:]]
    h.transition_probabilities[0] = tpl.transition_probabilities[0]
    h.match_emissions[1:] = np.asarray(tpl.match_emissions)[src[1:]]
    h.insert_emissions[:] = np.asarray(tpl.insert_emissions)[np.concatenate([[0], src[1:]])]
    t = np.array(h.transition_probabilities[M])
    t[0], t[2] = t[0] + t[2], 0.0
    t[5], t[6] = 1.0, 0.0
    h.transition_probabilities[M] = t
    h.composition = tpl.composition
    h.consensus = "".join(tpl.consensus[k - 1] for k in src[1:])
    h._evparam[:] = tpl._evparam
    return h


def make_library(n):
    with plan7.HMMFile(os.path.join(GOLDEN, "hmms", "bmyD.hmm")) as hf:
        tpl = next(iter(hf))
    out = []
    for e, M in enumerate(bw.library_lengths(n)):
        h = random_hmm(int(M), seed=7000 + e, alphabet=DNA) if e % 4 == 3 else resampled(tpl, int(M), e)
        h.name = f"dna{e:05d}_{int(M)}"
        h.max_length = window_length(h)         # what a search with an HMM query would replace it by
        out.append(h)
    return tpl, out


def read(name):
    with easel.SequenceFile(os.path.join(GOLDEN, "seqs", name), digital=True, alphabet=DNA) as f:
        return f.read_block()[0]


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 512, 2048])
    ap.add_argument("--targets", nargs="*", default=["bgc", "contig", "chr10m"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-repeats", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tpl, library = make_library(max(args.sizes))
    targets = {}
    if "bgc" in args.targets:
        targets["BGC0001090 (44,660 nt)"] = read("BGC0001090.gbk")
    if "contig" in args.targets:
        targets["contig OFHT01000022 (391,023 nt)"] = read("1390.SAMEA104415756.OFHT01000022.fna")
    if "chr10m" in args.targets:
        targets["chrSyn0[0:10 Mbp]"] = easel.DigitalSequence(DNA, name="chrSyn0_10M", sequence=bw.make_chromosome(tpl, int(250e6), planted=50, seed=45)[:10_000_000])
    report = {"library_nodes": {n: int(sum(h.M for h in library[:n])) for n in args.sizes}, "results": []}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# nhmmscan_bench: sizes {args.sizes}, batch {args.batch}; one warm-up, then timed runs; seconds, median [min .. max]")
    for tname, seq in targets.items():
        block = easel.DigitalSequenceBlock(DNA, [seq])
        cells_per_node = 2.0 * len(seq)                          # both strands
        list(hmmer.nhmmer(library[:8], block, devices=[0]))          # warm-up of the loop: kernels loaded, the target resident
        for n in args.sizes:
            lib = library[:n]
            # (a) the loop over the same n models
            loop = []
            for rep in range(args.loop_repeats):
                t0 = time.perf_counter()
                nh = sum(len(h) for h in hmmer.nhmmer(lib, block, devices=[0], searches_in_flight=8))
                loop.append(time.perf_counter() - t0)
            # (b) the public entry point, end to end: profiles and tables of the library prepared inside, the query uploaded
            list(hmmer.nhmmscan([seq], lib, batch=args.batch))           # warm-up: kernels loaded, LDS grants, slabs
            wall, kern, scan_seeds, tails, rate = [], [], [], [], []
            nhits = 0
            for rep in range(args.repeats):
                t0 = time.perf_counter()
                hits = next(hmmer.nhmmscan([seq], lib, batch=args.batch))
                wall.append(time.perf_counter() - t0)
                # (c) the result's own timing slots, summed over the batches (TopHits.timings_ms, the long-target meanings)
                tm = hits.timings_ms
                kern.append(tm["msv_kernel"] * 1e-3); scan_seeds.append(tm["msv"] * 1e-3); tails.append(tm["host_domaindef"] * 1e-3)
                rate.append(cells_per_node * report["library_nodes"][n] / max(kern[-1], 1e-9) / 1e12)
                nhits = len(hits)
            a, b, bk, bs, bt, br = map(stats, (loop, wall, kern, scan_seeds, tails, rate))
            fmt = lambda x, d=3: f"{x['median']:.{d}f} [{x['min']:.{d}f} .. {x['max']:.{d}f}]"
            say(f"{tname}: N = {n} ({report['library_nodes'][n]} nodes): (a) nhmmer loop, 8 in flight, {a['n']} runs: {fmt(a)} s ({nh} hits) | "
                f"(b) nhmmscan, {b['n']} runs: {fmt(b)} s = {a['median'] / b['median']:.2f} x (a) | (c) of (b): scan kernels {fmt(bk, 4)} s = {fmt(br, 2)} TCUPS "
                f"(single-model kernel on a full chromosome: 30.8), scan + seed bookkeeping {fmt(bs)} s, tails {fmt(bt)} s; {nhits} hits")
            report["results"].append({"target": tname, "N": n, "nhmmer_loop": a, "nhmmscan": b, "scan_kernels": bk, "scan_and_seeds": bs,
                                      "tails": bt, "scan_tcups": br, "hits": nhits})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n\n" + json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
