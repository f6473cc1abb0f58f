"""Nucleotide and protein models of the same kernel tier in one process, in both orders.

The dynamic LDS of the wave-per-target and the packed Viterbi kernels depends on the residue rows of the alphabet (Kp + 1:
19 for DNA, 30 for amino acids), and beyond 64 KiB a kernel needs a grant per device before it is launched
(p7x_launch.hpp).  A grant or an occupancy remembered from the first model of an instantiation would be too small for a
later model of the wider alphabet: at M = 500 fwd_kernel<8> / bck_kernel<8> take 55,296 bytes with DNA (no grant) and
77,824 with amino acids; at M = 800 fwd_kernel<16> / bck_kernel<16> take 110,592 and 155,648, vit_kernel<16> and
vitpk_kernel<32, 13> 55,296 / 52,224 and 77,824 / 74,752.

Each order runs in a fresh child process (this file as a script).  A part is: filters() with every stage and a search,
as test_gpu_filters.test_nucleotide_alphabets_through_every_filter runs them, on a block small enough for the
wave-per-target kernels, and filters() once more through the lane kernels ("small_block" = 0: the packed Viterbi filter).
Order A: the DNA part, the amino part, and the amino filters() with "vit_wide" = 0 (vit_kernel<16> from the lane path);
order B: the amino part (and its "vit_wide" = 0 run), then the DNA part.  Both orders must print the same, and what they
print must agree with the oracle as in that test."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CHILD_LIMIT_S = 120
LENGTHS = (500, 800)
SEED = 73          # the oracle's cascade on the CPU: all 10 fragments of each of the four blocks pass Viterbi and Forward


def _abc(kind):
    from pyhmmer_amd import easel
    return easel.Alphabet.dna() if kind == "dna" else easel.Alphabet.amino()


@functools.lru_cache(maxsize=None)
def _case(kind, M):
    """Model and block of (alphabet, M): 60 background targets and 10 fragments emitted from the model."""
    from conftest import random_hmm
    from test_gpu_filters import _model_block
    hmm = random_hmm(M, SEED, alphabet=_abc(kind))
    return hmm, _model_block(hmm, 60, 10, SEED)


def _child(order):
    sys.path.insert(0, str(ROOT / "tests"))
    import conftest  # noqa: F401  (puts the repository and the oracle on the path)
    from pyhmmer_amd import _lib, plan7

    def filters(hmm, blk, **opts):
        for name, value in opts.items():
            _lib.set_debug_option(name, value)
        try:        # the device image is laid out by the options in force when a profile is first used: a profile per call
            om = plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400)
            got = plan7.SequenceDatabase(blk).filters(om, msv=True, viterbi=True, forward=True, bias=True)
        finally:
            for name in opts:
                _lib.set_debug_option(name, -1)
        return {"xJ": np.asarray(got["xJ"]).astype(np.float64).tolist(), "xC": np.asarray(got["xC"]).astype(np.float64).tolist(),
                "fwd": np.asarray(got["fwd"], dtype=np.float32).view(np.uint32).tolist(),
                "filtersc": np.asarray(got["filtersc"], dtype=np.float32).view(np.uint32).tolist()}

    def part(kind, M, out):
        hmm, blk = _case(kind, M)
        out[f"{kind}{M}"] = filters(hmm, blk)
        hits = plan7.Pipeline(hmm.alphabet, E=1e3).search_hmm(hmm, blk)
        out[f"{kind}{M}_hits"] = {"stage_counts": dict(hits.stage_counts),
                                  "hits": [[h.name, h.score, [[d.env_from, d.env_to] for d in h.domains]] for h in hits]}
        out[f"{kind}{M}_lane"] = filters(hmm, blk, small_block=0)
        if kind == "amino":
            out[f"{kind}{M}_narrow"] = filters(hmm, blk, vit_wide=0)

    out = {}
    for M in LENGTHS:
        for kind in (("dna", "amino") if order == "A" else ("amino", "dna")):
            part(kind, M, out)
    print("RESULT " + json.dumps(out))


def _run_child(order):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", order], capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    assert r.returncode == 0, f"child of order {order}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-1500:]
    return json.loads(line[0][len("RESULT "):])


def _floats(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32).astype(np.float64)


@pytest.mark.gpu
def test_both_orders_of_the_alphabets_give_the_same_scores_and_the_oracles(oracle):
    from test_gpu_filters import BIAS_TOL_NATS, FWD_TOL_NATS, _oracle_scores
    from pyhmmer_amd import plan7
    got = {}
    for order in ("A", "B"):          # one after the other; a child that fails ends the test before the next one starts
        got[order] = _run_child(order)
    assert got["A"].keys() == got["B"].keys() and len(got["A"]) == 2 * (3 + 4)
    for key in got["A"]:
        assert got["A"][key] == got["B"][key], key
    for M in LENGTHS:
        for kind in ("dna", "amino"):
            hmm, blk = _case(kind, M)
            want = _oracle_scores(oracle.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400), blk)
            ok = np.isfinite(want["fwd"])
            for run in ("", "_lane") + (("_narrow",) if kind == "amino" else ()):
                res = got["A"][f"{kind}{M}{run}"]
                xJ, xC, fwd, filtersc = np.array(res["xJ"]), np.array(res["xC"]), _floats(res["fwd"]), _floats(res["filtersc"])
                print(f"{kind} M={M}{run}: fwd err {np.abs(fwd[ok] - want['fwd'][ok]).max():.3g}, bias err {np.abs(filtersc - want['bias']).max():.3g}")
                assert np.array_equal(xJ, want["msv"]) and np.array_equal(xC, want["vit"]), (kind, M, run)
                assert np.all(np.abs(fwd[ok] - want["fwd"][ok]) < FWD_TOL_NATS + 1e-5 * np.abs(want["fwd"][ok])), (kind, M, run)
                assert np.max(np.abs(filtersc - want["bias"])) < BIAS_TOL_NATS, (kind, M, run)
            search = got["A"][f"{kind}{M}_hits"]
            assert search["stage_counts"]["vit"] >= 8 and len(search["hits"]) >= 4, (kind, M, search["stage_counts"], len(search["hits"]))


if __name__ == "__main__" and "--child" in sys.argv:
    _child(sys.argv[sys.argv.index("--child") + 1])
