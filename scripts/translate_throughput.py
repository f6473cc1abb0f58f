"""Throughput of the six-frame ORF finder (p7x_orfs_find, p7x_translate.hip) on the two shapes it has to fill the device
with: the chromosome of bench.py's nhmmer field (bench_workloads.make_chromosome, 250 Mbp) and 1,000,000 random reads of
150 nt; both strands, min_length 20.  Per pass: kernel time from device events (both strands), nucleotides per second,
the bytes the pass reads and writes (computed from the shapes, below), and that traffic set against a device-to-device
copy that moves as many bytes, timed in this script with device events.  Beside them the host twin on 16 threads and the
whole `DigitalSequenceBlock.translate_orfs` call (upload, the four passes, the two host scans, copy-back, the Python
side).  Median of 5 runs after a warm-up.  Run from the repository root on the GPU:
    python scripts/translate_throughput.py [--mbp 250] [--reads 1000000] [--out profiles/r28_translate.md]"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402  (the copy yardstick; before the library, which binds to the HIP runtime torch has loaded)
assert torch.cuda.is_available(), "this measurement needs the device"
import bench_workloads as bw  # noqa: E402
from pyhmmer_amd import _lib, easel, plan7  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mbp", type=float, default=250.0)
ap.add_argument("--reads", type=int, default=1000000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=str(ROOT / "profiles" / "r28_translate.md"))
args = ap.parse_args()
lib = _lib.lib()
assert lib.p7x_device_count() >= 1, "this measurement needs the device"

DNA = easel.Alphabet.dna()
PASSES = ("summaries", "counts", "heads", "continuations")


def packed(seqs_or_arrays):
    dsq, offsets, lengths = seqs_or_arrays
    return easel.PackedBlock.from_arrays(dsq, offsets, lengths)


def reads_block(n, L, seed=3):
    rng = np.random.default_rng(seed)
    dsq = np.full(n * (L + 1) + 1, 255, dtype=np.uint8)
    dsq[1:].reshape(n, L + 1)[:, :L] = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
    offsets = 1 + np.arange(n, dtype=np.int64) * (L + 1)
    lengths = np.full(n, L, dtype=np.int32)
    names = [f"read{i}".encode() for i in range(n)]
    name_off = np.zeros(n, dtype=np.int64)
    name_off[1:] = np.cumsum([len(b) + 1 for b in names[:-1]])
    strtab = np.frombuffer(b"".join(b + b"\0" for b in names) + b"\0", dtype=np.uint8)
    return easel._LazyDigitalSequenceBlock(DNA, packed((dsq, offsets, lengths)), strtab, name_off, np.full(n, strtab.shape[0] - 1, dtype=np.int64))


def chromosome_block(L):
    with plan7.HMMFile(ROOT / "tests" / "golden" / "hmms" / "bmyD.hmm") as f:
        hmm = next(iter(f))
    return easel.DigitalSequenceBlock(DNA, [easel.DigitalSequence(DNA, name="chromosome", sequence=bw.make_chromosome(hmm, L))])


def find(pk, host_threads=0):
    h = C.c_void_p()
    t0 = time.perf_counter()
    if host_threads:
        rc = lib.p7x_orfs_find_host(1, pk.dsq.ctypes.data, pk.offsets.ctypes.data, pk.lengths.ctypes.data, pk.n, pk.total_residues, 20, 0, host_threads, C.byref(h))
    else:
        rc = lib.p7x_orfs_find(1, 0, pk.dsq.ctypes.data, pk.offsets.ctypes.data, pk.lengths.ctypes.data, pk.n, pk.total_residues, 20, 0, C.byref(h))
    dt = time.perf_counter() - t0
    assert rc == 0, _lib.last_error()
    info = [int(lib.p7x_orfs_info(h, k)) for k in range(11)]
    lib.p7x_orfs_destroy(h)
    return dt, info


def copy_seconds(nbytes):
    """A device-to-device copy of nbytes (it reads nbytes and writes nbytes), median of 5 after a warm-up, device events."""
    nbytes = max(int(nbytes), 1 << 20)
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    b.copy_(a)
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    del a, b
    return statistics.median(times)


def traffic(T, nseq, chunks, orfs, residues, strands=2):
    """Bytes each pass reads + writes, both strands: every pass reads the packed block once per strand; the per-chunk and
    per-sequence arrays are those of OrfArgs (p7x_translate.hip); the heads pass writes a 37-byte record per ORF, and
    heads and continuations together write every residue and sentinel of the output once."""
    out_bytes = residues + orfs + 1
    return {
        "summaries": strands * (T + 32 * chunks),
        "counts": strands * (T + 48 * chunks + 16 * chunks + 16 * (nseq + 1)),
        "heads": strands * (T + (24 + 24 + 16) * chunks + 24 * chunks + 16 * nseq) + 37 * orfs + out_bytes,
        "continuations": strands * (T + (24 + 24 + 24) * chunks),
    }


lines = ["# Six-frame ORFs on the device: throughput (scripts/translate_throughput.py)", "",
         f"One MI355X ({torch.cuda.get_device_name(0)}); both strands, `min_length` 20, table 1, `orf_chunk` at its default; median of "
         f"{args.runs} runs after one warm-up.  Kernel times are device events around each pass's launches (two strands, one "
         "launch each).  Traffic is computed from the shapes, not counted by the hardware; the copy beside it is a "
         "device-to-device copy that moves the same number of bytes (half read, half written), timed here with device events.", ""]
for label, block in ((f"chromosome, {args.mbp:g} Mbp (bench_workloads.make_chromosome)", chromosome_block(int(args.mbp * 1e6))),
                     (f"{args.reads} reads of 150 nt", reads_block(args.reads, 150))):
    pk = block.packed()
    T = pk.total_residues + pk.n + 1
    find(pk)
    runs = [find(pk) for _ in range(args.runs)]
    info = runs[0][1]
    orfs, residues, chunks, chunk = info[0], info[1], info[2], info[5]
    assert info[4] == 1
    med = lambda k: statistics.median(r[1][k] for r in runs) * 1e-6
    tr = traffic(T, pk.n, chunks, orfs, residues)
    lines += [f"## {label}", "",
              f"{pk.n} sequences, {pk.total_residues} nucleotides, {chunks} chunks of {chunk} per pass and strand; {orfs} ORFs, {residues} residues.", "",
              "| pass | kernel ms | Gnt/s (both strands) | MB read + written | GB/s | copy of as many bytes, ms | copy time / pass time |",
              "|---|---|---|---|---|---|---|"]
    total_k = 0.0
    for k, name in enumerate(PASSES):
        t = max(med(6 + k), 1e-9)
        total_k += t
        c = copy_seconds(tr[name] // 2)
        lines.append(f"| {name} | {1e3 * t:.2f} | {2 * pk.total_residues / t / 1e9:.2f} | {tr[name] / 1e6:.0f} | {tr[name] / t / 1e9:.0f} | {1e3 * c:.2f} | {c / t:.2f} |")
    call = statistics.median(r[0] for r in runs)
    lines += ["", f"All four passes: {1e3 * total_k:.1f} ms of kernels = {2 * pk.total_residues / total_k / 1e9:.2f} Gnt/s over both strands; "
              f"host scans between them {1e3 * med(10):.1f} ms; the C call (upload, passes, scans, copy-back) {1e3 * call:.0f} ms "
              f"= {pk.total_residues / call / 1e6:.0f} Mnt/s."]
    find(pk, 16)
    host = statistics.median(find(pk, 16)[0] for _ in range(args.runs))
    lines.append(f"Host twin, 16 threads (ranges of whole sequences; one contig is one range): {1e3 * host:.0f} ms = {pk.total_residues / host / 1e6:.0f} Mnt/s.")
    block.translate_orfs(min_length=20)
    py = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        got = block.translate_orfs(min_length=20)
        py.append(time.perf_counter() - t0)
        assert len(got) == orfs
    pyt = statistics.median(py)
    lines += [f"`DigitalSequenceBlock.translate_orfs`, whole call: {1e3 * pyt:.0f} ms = {pk.total_residues / pyt / 1e6:.0f} Mnt/s "
              f"({1e3 * (pyt - call):.0f} ms more than the C call: the copy into the block's numpy arrays).", ""]
    print("\n".join(lines[-14:]), flush=True)
    del block, pk, got
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text("\n".join(lines) + "\n")
print(f"wrote {args.out}")
