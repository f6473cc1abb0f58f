"""Where the rounds of hmmer.jackhmmer spend their time: 64 queries (the sequences of PKSI.faa and LuxC.faa, repeated under
new names up to 64) against the fixture proteome, five rounds at most, one batch.  Per round: the batched search, the host
steps (sort, compare_ranking, to_msa of every query), the models of the alignments that go on (counting passes, priors;
this includes turning the alignments into code matrices) and their one calibration -- hmmer.jackhmmer_rounds() and
hmmer.pipeline_stats().  Run twice after a warm-up: with the code matrix the alignments keep, and with the seam "msa_codes" =
0, under which every alignment encodes its text rows as before.  Run from the repository root on the GPU:
python scripts/jackhmmer_rounds.py   (figures: profiles/r24_jackhmmer_rounds.md)."""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pyhmmer_amd import _lib, easel, hmmer  # noqa: E402

abc = easel.Alphabet.amino()
seqs = ROOT / "tests" / "golden" / "seqs"
with easel.SequenceFile(seqs / "938293.PRJEB85.HG003687.faa", digital=True, alphabet=abc) as sf:
    proteome = sf.read_block()
pool = []
for name in ("PKSI.faa", "LuxC.faa"):
    with easel.SequenceFile(seqs / name, digital=True, alphabet=abc) as sf:
        pool.extend(sf)
queries = []
for i in range(64):
    q = pool[i % len(pool)].copy()
    q.name = f"{q.name}#{i // len(pool)}" if i >= len(pool) else q.name
    queries.append(q)
print(f"{len(queries)} queries ({len(pool)} different), {sum(len(q) for q in queries)} residues; {len(proteome)} targets, "
      f"{sum(len(s) for s in proteome)} residues", flush=True)


def run(label, codes):
    _lib.set_debug_option("msa_codes", codes)
    t0 = time.perf_counter()
    results = list(hmmer.jackhmmer(queries, proteome, checkpoints=True))
    wall = time.perf_counter() - t0
    _lib.set_debug_option("msa_codes", -1)
    rounds = hmmer.jackhmmer_rounds()
    print(f"== {label}: {1e3 * wall:.0f} ms, rounds per query {sorted(set(len(r) for r in results))}, "
          f"converged {sum(r[-1].converged for r in results)} of {len(results)}", flush=True)
    print(f"round 0: {rounds[0]['queries']:2d} queries | models of the query sequences {1e3 * rounds[0]['build_models']:.1f} ms | "
          f"calibrate {1e3 * rounds[0]['calibrate']:.1f} ms", flush=True)
    for r, rec in enumerate(rounds[1:], 1):
        rows = [len(res[r - 1].msa.names) for res in results if len(res) >= r]
        cols = [len(res[r - 1].msa) for res in results if len(res) >= r]
        p = rec["pipeline"]
        print(f"round {rec['round']}: {rec['queries']:2d} queries | search {1e3 * rec['search']:7.1f} ms (batches {p.get('batches')}, "
              f"feeder device wait {1e3 * p.get('feeder_device_wait', 0):.1f}, host stages {1e3 * p.get('finish', 0):.1f}) | "
              f"host steps {1e3 * rec['host_steps']:6.1f} ms | build models {1e3 * rec['build_models']:6.1f} ms | "
              f"calibrate {1e3 * rec['calibrate']:6.1f} ms | alignments: rows {min(rows)}..{max(rows)} (sum {sum(rows)}), "
              f"columns {min(cols)}..{max(cols)}", flush=True)
    return rounds


run("warm-up", -1)
run("code matrix kept", -1)
run("code matrix off (msa_codes = 0)", 0)
