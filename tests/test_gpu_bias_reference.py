"""bias_kernel (p7x_pipeline.hip) against the float64 reference of tests/bias_reference.py: its scores through the seam
p7x_filters_batch on the targets of tests/bias_targets.py, and the decisions a search takes with them.

The bounds come from tests/test_host_bias_reference.py: what the float32 engines on the host (the same operations in the
same order as the kernel) differ from the reference on the same model's family, times DEVICE_FACTOR -- the kernel may
contract multiply-adds the host engines do not -- with the float32 floor REL_SCORE x S of a running sum under it.  Nothing
the device computes is compared with the device's own output."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import bias_reference as R
import bias_targets as T
from pyhmmer_amd import _lib, easel, plan7
from test_host_bias_reference import MEASURED, REL_SCORE

pytestmark = pytest.mark.gpu

DEVICE_FACTOR = 4.0
LANES_PER_BLOCK, BLOCKS_PER_CU = 64, 4           # p7x_filters_batch launches bias_kernel with num_cu * 4 blocks of 64


def device_bound(key, family, S):
    return np.maximum(DEVICE_FACTOR * MEASURED[key][family], REL_SCORE * np.asarray(S))


@pytest.fixture
def say(capsys):
    """One line on the terminal whatever the capture mode: the device's distances belong to the run's output."""
    def emit(line):
        with capsys.disabled():
            print("\n[bias-reference] " + line, end="", flush=True)
    return emit


# ------------------------------------------------------------------------------------------------ scores through the seam
@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_scores_of_families_a_b_c_against_the_reference(key, say):
    """One block per model: the lengths around the kernel's 16-residue blocks and their prefetch with two empty targets
    between them, the composition-dominated repeats, every degenerate and special code at the block edges.  An empty
    target has no slot on the device: the seam answers 0 for it (the null score of no residues: 0 ln p1 + ln 1), and its
    neighbours' scores are those of the block without it."""
    hmm, bg = T.model(key)
    om = T.profile(key)
    named = [(f"{f}:{name}", seq) for f in "abc" for name, seq in T.targets(key, f)]
    got = plan7.SequenceDatabase(T.block(hmm.alphabet, named)).filters(om, msv=False, bias=True)["filtersc"]
    assert got.shape == (len(named),) and got.dtype == np.float32
    refs = {f"{f}:{name}": (T.label(f, seq), ref) for f in "abc" for name, seq, ref in T.reference(key, f)}
    worst = {f: 0.0 for f in T.FAMILIES[:-1]}
    failures = []
    empties = 0
    for t, (name, seq) in enumerate(named):
        if len(seq) == 0:
            empties += 1
            assert got[t] == 0.0 and not np.signbit(got[t]), (name, got[t])
            assert len(named[t - 1][1]) and len(named[t + 1][1])                    # scored neighbours on both sides
            continue
        fam, ref = refs[name]
        err = abs(float(got[t]) - ref.filtersc)
        worst[fam] = max(worst[fam], err)
        if not err <= device_bound(key, fam, ref.S):
            failures.append((name, float(got[t]), ref.filtersc, err, float(device_bound(key, fam, ref.S))))
    assert empties == 2
    say(f"{key} (M {hmm.M}) device / oracle: " + ", ".join(f"{f} {worst[f]:.2e} / {MEASURED[key][f]:.1e}" for f in worst))
    assert not failures, failures


@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_scores_of_many_short_targets_against_the_reference(key, say):
    """Family d: 70,000 targets of 1-40 residues, more than the grid of the seam's launch holds lanes, so that the kernel's
    loop over the work list takes a second trip; then the family's first 1, 63, 64 and 65 targets as blocks of their own
    (a wavefront's worth of lanes, one less, one more).  The reference is vectorised by length."""
    hmm, bg = T.model(key)
    om = T.profile(key)
    dsq, offsets, lengths = T.family_d(key)
    name = C.create_string_buffer(256)
    assert _lib.lib().p7x_device_name(0, name, 256) == 0
    num_cu = int(re.search(r"(\d+) CUs", name.value.decode()).group(1))
    assert T.MANY > LANES_PER_BLOCK * BLOCKS_PER_CU * num_cu, num_cu
    want, S = T.reference_d(key)
    bound = device_bound(key, "d", S)
    line = []
    for n in (T.MANY,) + T.SMALL_BLOCKS:
        db = plan7.SequenceDatabase.from_packed(hmm.alphabet, dsq[:offsets[n - 1] + lengths[n - 1] + 1], offsets[:n], lengths[:n])
        got = db.filters(om, msv=False, bias=True)["filtersc"]
        assert got.shape == (n,)
        err = np.abs(got.astype(np.float64) - want[:n])
        line.append(f"n {n}: {err.max():.2e}")
        bad = np.nonzero(~(err <= bound[:n]))[0]
        assert bad.size == 0, (n, bad[:10], got[bad[:10]], want[bad[:10]], bound[bad[:10]])
    say(f"{key} (M {hmm.M}) family d device / oracle {MEASURED[key]['d']:.1e}: " + ", ".join(line))


# ------------------------------------------------------------------------------------------------ decisions through the cascade
@pytest.fixture(scope="module")
def cascade(oracle):
    """The decision block through p7x_search_batch_raw for the three models in one batch, bias filter on and off, and the
    oracle's records of the same block."""
    dsq, offsets, lengths = T.decision_block()
    abc = easel.Alphabet.amino()
    pli = plan7.Pipeline(abc)
    bg = pli.background
    hmms = [T.model(k)[0] for k in T.DECISION_KEYS]
    assert all(np.array_equal(T.model(k)[1].residue_frequencies, bg.residue_frequencies) for k in T.DECISION_KEYS)
    oms = [T.profile(k) for k in T.DECISION_KEYS]
    db = plan7.SequenceDatabase.from_packed(abc, dsq, offsets, lengths)
    nq, n = len(oms), len(lengths)
    handles = (C.c_void_p * nq)(*[om._handle for om in oms])
    bgf = np.ascontiguousarray(bg.residue_frequencies, dtype=np.float32)
    out = {}
    for do_bias in (1, 0):
        cfg = pli._cfg()
        cfg.do_biasfilter = do_bias
        xJ, xC, stage = np.zeros((nq, n), dtype=np.int32), np.zeros((nq, n), dtype=np.int32), np.zeros((nq, n), dtype=np.uint8)
        st = _lib.lib().p7x_search_batch_raw(C.byref(cfg), handles, nq, bgf.ctypes.data, db._handle, xJ.ctypes.data, xC.ctypes.data, stage.ctypes.data)
        assert st == 0, _lib.last_error()
        out[do_bias] = (xJ, stage)
    pk = easel.PackedBlock.from_arrays(dsq, offsets, lengths)
    records = [np.frombuffer(oracle.OracleProfile(h, bg, 400).cascade_block(pk, want_records=True)[0], dtype=np.dtype(oracle.Record)).copy() for h in hmms]
    return pli, hmms, (dsq, offsets, lengths), out, records


def test_bias_filter_decisions_in_the_cascade_are_the_references(cascade, say):
    """20,000 targets of 50-400 residues, every third with a stretch of a model's composition, three models in one batch,
    default thresholds.  xJ is the oracle's, and with it usc (a function of xJ and L alone; a sample goes through the
    single-sequence entry point too).  For every MSV survivor P is formed in float64 from the reference's filtersc and that
    usc: the device lets the target past the bias filter exactly when P <= F1, except inside a margin of the device bound
    of the scores test (from the figure the host test records for these very survivors) -- at most 1 % of the survivors,
    and at least 100 survivors on each side of F1 for every model."""
    pli, hmms, (dsq, offsets, lengths), out, records = cascade
    xJ, stage = out[1]
    for q, key in enumerate(T.DECISION_KEYS):
        rec, hmm = records[q], hmms[q]
        assert np.array_equal(xJ[q], rec["xJ_msv"]), (key, int(np.sum(xJ[q] != rec["xJ_msv"])))
        survivors = np.nonzero(stage[q] >= 1)[0]
        assert np.array_equal(survivors, np.nonzero(rec["stage"] >= 1)[0]), key
        usc = rec["usc"]
        om = T.profile(key)
        for t in survivors[:: max(1, len(survivors) // 12)]:
            seq = easel.DigitalSequence(hmm.alphabet, name="t", sequence=dsq[offsets[t]:offsets[t] + lengths[t]].copy())
            assert np.float32(om.msv_filter(seq)) == usc[t], (key, int(t))
        rm = T.ref_model(key)
        refs = [R.filter_score(rm, dsq[offsets[t]:offsets[t] + lengths[t]]) for t in survivors]
        E = [float(device_bound(key, "dec", r.S)) for r in refs]
        left, npass, nfail = T.check_decisions(key, stage[q] >= 2, usc, [r.filtersc for r in refs], survivors, E, pli.F1)
        worst = max(abs(float(rec["filtersc"][t]) - r.filtersc) for t, r in zip(survivors, refs))
        say(f"decisions {key} (M {hmm.M}): {len(survivors)} MSV survivors, {npass} past the bias filter, {nfail} stopped, {left} left out "
            f"({100.0 * left / len(survivors):.2f} %); oracle's filtersc within {worst:.2e} of the reference on them")
        assert left <= 0.01 * len(survivors), (key, left, len(survivors))
        assert npass >= 100 and nfail >= 100, (key, npass, nfail)


def test_decisions_with_the_bias_filter_off_follow_null1_alone(cascade, say):
    """do_biasfilter = 0 on the same block: whoever survives MSV goes on, and who survives MSV is decided by the null1 score
    alone -- for all 20,000 targets, stage >= 1 and stage >= 2 both equal P <= F1 with P from usc and the length's null1 in
    float64 (the margin: REL_SCORE x |null1|, the rounding of the float32 table entry)."""
    pli, hmms, (dsq, offsets, lengths), out, records = cascade
    xJ, stage = out[0]
    p1 = [float(np.float32(L) / np.float32(L + 1)) for L in range(1, 401)]
    null1 = np.array([0.0] + [L * math.log(p) + math.log(1.0 - p) for L, p in enumerate(p1, start=1)])       # no target is empty
    everyone = np.arange(len(lengths))
    for q, key in enumerate(T.DECISION_KEYS):
        rec, hmm = records[q], hmms[q]
        assert np.array_equal(xJ[q], rec["xJ_msv"]), key
        nullsc = null1[lengths]
        T.check_decisions(key, stage[q] >= 1, rec["usc"], nullsc, everyone, REL_SCORE * np.abs(nullsc), pli.F1)
        left, npass, nfail = T.check_decisions(key, stage[q] >= 2, rec["usc"], nullsc, everyone, REL_SCORE * np.abs(nullsc), pli.F1)
        say(f"decisions {key}, bias filter off: {npass} of {len(lengths)} go on, {left} left out")
        assert left <= 0.0001 * len(lengths) and npass >= 100 and nfail >= 100, (key, left, npass, nfail)
