"""A multi-class cascade against a large block gives the same results on every stream layout, with four hardware queues
and with eight.

The smallest shape that reaches the code: a block of more than 256 groups of 64 targets (20,000 short ones) takes the
class-by-class branch of cascade_enqueue, and twelve fixture models of M = 83 .. 400 fall into three tiers of MSV register
tiles (msv_pick / msv_tier: M <= 182 one lane and up to 92 row registers, M <= 270 up to 136, beyond more), so the batch
has several classes and three tier launches.  The search runs in two fresh child processes (this file as a script), one
with GPU_MAX_HW_QUEUES=4 in its environment and one with 8: the runtime reads the variable once, when it initialises."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NTARGETS = 20_000
CHILD_LIMIT_S = 240


def _child():
    sys.path.insert(0, str(ROOT))
    import ctypes as C

    import numpy as np

    from pyhmmer_amd import _lib, hmmer, plan7

    def load(name):
        with plan7.HMMFile(ROOT / "tests" / "golden" / "hmms" / f"{name}.hmm") as f:
            return list(f)

    queries = load("RREFam")[:8] + load("PF02826") + load("Thioesterase") + load("KR") + load("LuxC")
    abc = queries[0].alphabet
    rng = np.random.default_rng(20251)
    bg = plan7.Background(abc).residue_frequencies.astype(np.float64)
    cum = np.cumsum(bg / bg.sum())
    lengths = rng.integers(60, 121, size=NTARGETS).astype(np.int32)
    offsets = (1 + np.concatenate([[0], np.cumsum(lengths[:-1].astype(np.int64) + 1)])).astype(np.int64)
    flat = np.full(int(offsets[-1] + lengths[-1] + 1), 255, dtype=np.uint8)
    res = np.minimum(np.searchsorted(cum, rng.random(int(lengths.sum()))), abc.K - 1).astype(np.uint8)
    pos = 0
    for t in range(NTARGETS):
        flat[offsets[t]: offsets[t] + lengths[t]] = res[pos: pos + lengths[t]]
        pos += int(lengths[t])
    # a few targets carry a stretch of a model's consensus: hits, with domains, for most of the models
    planted = rng.choice(NTARGETS, size=48, replace=False)
    for i, t in enumerate(planted):
        q = queries[i % len(queries)]
        cons = [abc.symbols.index(c.upper()) for c in q.consensus if c.upper() in abc.symbols[:abc.K]]
        n = min(len(cons), int(lengths[t]) - 8, 70)
        a = int(rng.integers(0, len(cons) - n + 1))
        flat[offsets[t] + 4: offsets[t] + 4 + n] = np.array(cons[a: a + n], dtype=np.uint8)
    db = plan7.SequenceDatabase.from_packed(abc, flat, offsets, lengths, device=0)
    assert (NTARGETS + 63) // 64 > 256

    def rows(tophits):
        return [[t.stage_counts, [[h.seqidx, h.score, [[d.env_from, d.env_to, d.alignment.target_from, d.alignment.target_to,
                                                          d.alignment.hmm_from, d.alignment.hmm_to, d.score] for d in h.domains]] for h in t]]
                for t in tophits]

    hw = C.c_int32(-99)
    _lib.lib().p7x_debug_stream_plan(None, 0, C.byref(hw))
    out = {"hw_queues_seen": hw.value, "env": os.environ.get("GPU_MAX_HW_QUEUES")}
    out["batch"] = rows(hmmer.hmmsearch(queries, db, devices=[0], batch=len(queries)))
    out["single"] = [rows(hmmer.hmmsearch([q], db, devices=[0]))[0] for q in queries]
    for key, opts in (("streams_1", {"cascade_streams": 1}), ("streams_2", {"cascade_streams": 2}),
                      ("streams_2_split", {"cascade_streams": 2, "cascade_split": 1}), ("streams_8", {"cascade_streams": 8})):
        for name, value in opts.items():
            _lib.set_debug_option(name, value)
        try:
            out[key] = rows(hmmer.hmmsearch(queries, db, devices=[0], batch=len(queries)))
        finally:
            for name in opts:
                _lib.set_debug_option(name, -1)
    print("RESULT " + json.dumps(out))


def _run_child(queues):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(queues))
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    assert r.returncode == 0, f"child with {queues} queues: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-1500:]
    return json.loads(line[0][len("RESULT "):])


@pytest.mark.gpu
def test_stream_layouts_and_queue_counts_give_identical_results():
    got = {}
    for queues in (4, 8):          # one after the other; a child that fails ends the test before the next one starts
        got[queues] = res = _run_child(queues)
        assert res["env"] == str(queues) and res["hw_queues_seen"] == queues
        want = res["batch"]
        assert len(want) == 12
        nhits = sum(len(t[1]) for t in want)
        ndom = sum(len(h[2]) for t in want for h in t[1])
        print(f"{queues} queues: {nhits} hits, {ndom} domains, past MSV {[t[0]['msv'] for t in want]}")
        assert nhits >= 24 and ndom >= nhits and sum(1 for t in want if t[1]) >= 8
        assert res["single"] == want                       # one model at a time: the single-class path
        for key in ("streams_1", "streams_2", "streams_2_split", "streams_8"):
            assert res[key] == want, key
    assert got[4]["batch"] == got[8]["batch"]


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
