"""hmmalign's float64 log-space path on the host (seam "host_align" = 1: the host log twin, p7x_logdp.cpp) against the
float64 reference of tests/dp_reference.py and the optimal accuracy of tests/oa_reference.py, on the tandem targets of
tests/tandem_targets.py: where posterior decoding overflows (family b: `OverflowError` without the path), where Backward
leaves Forward's scale factors (family a), ragged lengths (family c), and the KR prefix sweep through the zone in which the
scaled float32 path degrades before it overflows.

Bounds.  A trace posterior is the float64 posterior rounded to float32: rounding a value <= 1 costs at most 2^-25, and
float64 accumulation over at most L + M log-sums of |value| <= 3,000 costs under 1e-8, so every posterior lies within
2^-24 of the reference's.  The trace is optimal for posteriors that each differ from the reference's by less than that, so
its expected accuracy under the reference's posteriors is at least the reference's optimum minus 2 L 2^-24."""
import numpy as np
import pytest

import dp_reference as R
import oa_reference
import tandem_targets as T
from pyhmmer_amd import _lib, plan7
from test_gpu_align import PP_TOL
from test_host_dp_reference import MEASURED

PP_BOUND = 2.0 ** -24
SWEEP = tuple(range(60, 131, 10))


@pytest.fixture
def report(capsys):
    def emit(line):
        with capsys.disabled():
            print("\n[align-logspace] " + line, end="", flush=True)
    return emit


@pytest.fixture
def host_align(libp7x):
    _lib.set_debug_option("host_align", 1)
    yield
    _lib.set_debug_option("host_align", -1)
    _lib.set_debug_option("align_logspace", -1)


def check_against_reference(key, named, traces):
    """(worst |pp - reference|, worst optimal-accuracy shortfall in units of its bound) over the traces; asserts both."""
    rm = T.ref_model(key)
    worst_pp = worst_oa = 0.0
    for (name, seq), tr in zip(named, traces):
        ref = T.reference(key, name, seq, False, cells=True)
        want = R.trace_posteriors(ref, tr)
        err = float(np.abs(np.asarray(tr.posterior_probabilities, dtype=np.float64) - want).max())
        assert err <= PP_BOUND, (name, err)
        best = oa_reference.optimal_accuracy(rm, ref)
        slack = 2.0 * len(seq) * PP_BOUND
        short = best - float(want.sum())
        assert short <= slack, (name, best, float(want.sum()))
        worst_pp, worst_oa = max(worst_pp, err), max(worst_oa, short / slack)
    return worst_pp, worst_oa


def fine_for(key):
    return T.targets("rnd40" if key == "rnd45" else key, "a")


@pytest.mark.parametrize("key", T.OVERFLOW_KEYS)
def test_family_b_overflows_without_the_path_and_aligns_with_it(libp7x, host_align, key, report):
    hmm = T.model(key)
    named = T.targets(key, "b")
    block = T.block(hmm.alphabet, named)
    with pytest.raises(OverflowError):
        plan7.TraceAligner().compute_traces(hmm, block)
    aligner = plan7.TraceAligner(logspace=True)
    traces = aligner.compute_traces(hmm, block)
    assert len(traces) == len(named) and all(len(t.st) for t in traces)
    assert traces.nlogspace >= len(named) and all(t._logspace for t in traces)
    e_pp, e_oa = check_against_reference(key, named, traces)
    aligner.align_traces(hmm, block, traces)
    report(f"host log twin {key} family b: worst |pp - reference| {e_pp:.3e} (bound {PP_BOUND:.3e}), optimal-accuracy "
           f"shortfall {e_oa:.3e} of its bound, nlogspace {traces.nlogspace}")


@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_family_a_takes_the_path_under_the_flag(libp7x, host_align, key, report):
    """Backward leaves Forward's scale factors on every family-a target: the trigger that needs no threshold."""
    hmm = T.model(key)
    named = T.targets(key, "a")
    block = T.block(hmm.alphabet, named)
    aligner = plan7.TraceAligner(logspace=True)
    traces = aligner.compute_traces(hmm, block)
    assert traces.nlogspace == len(named) and traces.nlogspace_flagged == 0
    e_pp, e_oa = check_against_reference(key, named, traces)
    aligner.align_traces(hmm, block, traces)
    report(f"host log twin {key} family a (own scales): worst |pp - reference| {e_pp:.3e}, optimal-accuracy shortfall {e_oa:.3e} of its bound")


@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_every_sequence_through_the_path_by_the_seam(libp7x, host_align, key, report):
    hmm = T.model(key)
    named = T.targets(key, "a") + T.targets(key, "c")
    block = T.block(hmm.alphabet, named)
    _lib.set_debug_option("align_logspace", 1)
    aligner = plan7.TraceAligner()
    traces = aligner.compute_traces(hmm, block)
    _lib.set_debug_option("align_logspace", -1)
    assert traces.nlogspace == len(named)
    e_pp, e_oa = check_against_reference(key, named, traces)
    aligner.align_traces(hmm, block, traces)
    report(f"host log twin {key} families a + c (seam): worst |pp - reference| {e_pp:.3e}, optimal-accuracy shortfall {e_oa:.3e} of its bound")


def sweep_target(n):
    piece = T.consensus(T.model("KR"))[:n]
    return f"KR_sweep{n}", T._tandem(T._rng("KR", 1000 + n), [piece, piece])


def test_kr_sweep_through_the_degraded_zone(libp7x, host_align, report):
    """Two copies of consensus[:n] of KR, n = 60 .. 130: with the flag every trace is within the scaled path's own bound of
    the reference (the short ones may stay on the scaled path), nothing raises, and from n = 90 -- where the scaled path
    returns wrong posteriors or overflows -- every target takes the log-space path.  Without the flag: what there is to see."""
    hmm = T.model("KR")
    rm = T.ref_model("KR")
    bound = max(MEASURED["KR"]["pp"] + PP_TOL, PP_BOUND)
    for n in SWEEP:
        name, seq = sweep_target(n)
        block = T.block(hmm.alphabet, [(name, seq)])
        ref = R.forward_backward(rm, seq, False, cells=True)
        one = R.forward_backward(rm, T.consensus(hmm)[:n], False).fwd
        traces = plan7.TraceAligner(logspace=True).compute_traces(hmm, block)
        err = float(np.abs(traces[0].posterior_probabilities - R.trace_posteriors(ref, traces[0])).max())
        try:
            plain = plan7.TraceAligner().compute_traces(hmm, block)
            e0 = float(np.abs(plain[0].posterior_probabilities - R.trace_posteriors(ref, plain[0])).max())
            without = f"aligned, worst |pp - reference| {e0:.1e}"
        except OverflowError:
            without = "OverflowError"
        report(f"KR sweep n = {n}: one copy {one:.1f} nats; flag off: {without}; flag on: {err:.1e}, nlogspace {traces.nlogspace}")
        assert err <= bound, (n, err)
        if n >= 90:
            assert traces.nlogspace == 1, n


@pytest.mark.parametrize("key", T.OVERFLOW_KEYS)
def test_flag_off_is_unchanged(libp7x, host_align, key):
    """Without the flag: the error and its message on family b, deterministic traces on the sequences that align, none of
    them from the log-space path."""
    hmm = T.model(key)
    aligner = plan7.TraceAligner()
    assert aligner.logspace is False and repr(aligner) == "TraceAligner()"
    for name, seq in T.targets(key, "b"):
        with pytest.raises(OverflowError) as err:
            aligner.compute_traces(hmm, T.block(hmm.alphabet, [fine_for(key)[0], (name, seq)]))
        assert str(err.value) == (f"hmmalign: posterior decoding overflowed on sequence {name!r} (L = {len(seq)}); "
                                  "upstream's generic-DP fallback is not implemented")
    named = fine_for(key) + (T.targets(key, "c") if key != "rnd45" else T.targets("rnd40", "c"))
    block = T.block(hmm.alphabet, named)
    first, second = aligner.compute_traces(hmm, block), aligner.compute_traces(hmm, block)
    assert first == second and first.nlogspace == 0 and first.nlogspace_flagged == 0
    assert not any(t._logspace for t in first)
    # with the flag the sequences that stay on the scaled path keep their traces bit for bit
    flagged = plan7.TraceAligner(logspace=True).compute_traces(hmm, block)
    for a, b in zip(first, flagged):
        assert b._logspace or a == b


def test_the_flag_travels(libp7x):
    import pickle
    a = plan7.TraceAligner(device=0, cpus=3, logspace=True)
    for b in (pickle.loads(pickle.dumps(a)), a.copy()):
        assert (b.device, b.cpus, b.logspace) == (0, 3, True)
    assert "logspace=True" in repr(a)
