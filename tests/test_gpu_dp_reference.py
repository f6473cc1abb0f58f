"""The device's Forward / Backward parsers, hmmalign and the search's domain decoding against the float64 log-space reference
(tests/dp_reference.py) on the targets of tests/tandem_targets.py: Backward on its own scale factors (family a), posterior
decoding that overflows (family b), ragged lengths around the Backward kernel's 64-row blocks (family c).

Every bound comes from tests/test_host_dp_reference.py: what the ORACLE (upstream's striped float32 order) was measured to
differ from the reference on the same model's targets, times DEVICE_FACTOR -- the device sums the same float32 terms in another
association (lane chunks, then a wave reduction), which may cost a few times the oracle's own distance and no more.  The
existing tolerances against the oracle (FWD_TOL_NATS, PP_TOL) stay in their tests."""
import ctypes as C
import gc
import sys

import numpy as np
import pytest

import dp_reference as R
import host_pipeline
import tandem_targets as T
from conftest import synthetic_block
from pyhmmer_amd import _lib, easel, plan7
from test_gpu_align import PP_TOL
from test_host_dp_reference import MEASURED, region_scan

pytestmark = pytest.mark.gpu

DEVICE_FACTOR = 4.0
REL_SCORE = 1e-6          # a float32 score of |s| nats is not known better than a few ulps: 1e-6 |s|


def _families(key, which="abc"):
    have = ("ac" if key in T.FRAGMENT_NODES else "") + ("b" if key in T.OVERFLOW_KEYS else "")
    return [t for f in which if f in have for t in T.targets(key, f)]


def _profile(key):
    hmm = T.model(key)
    return hmm, plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400)


def _check_parsers(key, label):
    hmm, om = _profile(key)
    named = _families(key)
    block = T.block(hmm.alphabet, named)
    fwd = plan7.SequenceDatabase(block).filters(om, msv=False, forward=True)["fwd"]
    worst_f = worst_b = 0.0
    for (name, seq), s, got_f in zip(named, block, fwd):
        ref = T.reference(key, name, seq, True)
        got_b = om.backward_parser(s)
        ef, eb = abs(float(got_f) - ref.fwd), abs(got_b - ref.bck)
        print(f"[dp-reference] {label} {name}: L={len(seq)} fwd {float(got_f):.6f} ref {ref.fwd:.6f} diff {ef:.2e}; "
              f"bck {got_b:.6f} ref {ref.bck:.6f} diff {eb:.2e}", file=sys.stderr)
        worst_f, worst_b = max(worst_f, ef), max(worst_b, eb)
        assert ef <= max(DEVICE_FACTOR * MEASURED[key]["fwd"], REL_SCORE * abs(ref.fwd)), (name, float(got_f), ref.fwd)
        assert eb <= max(DEVICE_FACTOR * MEASURED[key]["bck"], REL_SCORE * abs(ref.bck)), (name, got_b, ref.bck)
    print(f"[dp-reference] {label}: {len(named)} targets, worst Forward {worst_f:.2e} Backward {worst_b:.2e} nats "
          f"(oracle {MEASURED[key]['fwd']:.1e} / {MEASURED[key]['bck']:.1e})", file=sys.stderr)


@pytest.mark.parametrize("key", T.MODEL_KEYS + ("rnd45",))
def test_parsers_against_the_reference(key):
    """SequenceDatabase.filters(forward=True) and OptimizedProfile.backward_parser on families a, b, c: within
    max(4 x the oracle's own distance from the reference, 1e-6 |score|) of the reference's multihit scores.

    (Not repeated under the seam fwd_grouped = 1: filters() always launches the wave-per-target kernel, and in a search the
    grouped kernel's scores only decide who survives the Forward filter -- the score a hit reports is the rows pass's, the
    wave-per-target kernel again.  No entry point returns a score of p7x_fwdpk.hip that the reference could be held against;
    its survivors are pinned by tests/test_gpu_filters.py.)"""
    _check_parsers(key, f"parsers {key}")


# ------------------------------------------------------------------------------------------------ hmmalign
def _host_traces(hmm, block):
    _lib.set_debug_option("host_align", 1)
    try:
        return plan7.TraceAligner().compute_traces(hmm, block)
    finally:
        _lib.set_debug_option("host_align", -1)


@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_hmmalign_posteriors_against_the_reference(key):
    """Families a (Backward on its own scales, scaleproduct *= fS / bS in the decoding) and c: the device's traces are the host
    twin's (flagged sequences are the host twin's anyway), and every posterior of every trace the device kept is within
    E_pp + PP_TOL of the reference's posterior of the same cell.  At most half of the sequences may be flagged."""
    hmm = T.model(key)
    named = _families(key, "ac")
    block = T.block(hmm.alphabet, named)
    dev = plan7.TraceAligner().compute_traces(hmm, block)
    host = _host_traces(hmm, block)
    assert len(dev) == len(host) == len(named)
    ndev = sum(1 for t in dev if t._device)
    assert ndev == dev.ndevice and ndev + dev.nflagged == len(named)
    worst, worst_a = 0.0, 0.0
    for (name, seq), d, h in zip(named, dev, host):
        assert np.array_equal(d.st, h.st) and np.array_equal(d.k, h.k) and np.array_equal(d.i, h.i), name
        if not d._device:
            continue
        want = R.trace_posteriors(T.reference(key, name, seq, False, cells=True), d)
        err = float(np.abs(np.asarray(d.posterior_probabilities, dtype=np.float64) - want).max())
        worst = max(worst, err)
        if name.endswith(("_a2", "_a4")):
            worst_a = max(worst_a, err)
    print(f"[dp-reference] hmmalign {key}: device traces {ndev} of {len(named)}, flagged {dev.nflagged}; worst |pp - reference| "
          f"{worst:.2e} (family a {worst_a:.2e}); bound {MEASURED[key]['pp'] + PP_TOL:.2e}", file=sys.stderr)
    assert 2 * dev.nflagged <= len(named), (dev.nflagged, len(named))
    assert any(d._device for (name, _), d in zip(named, dev) if name.endswith(("_a2", "_a4"))), "no own-scales trace came from the device"
    assert worst <= MEASURED[key]["pp"] + PP_TOL


def _memory_stats():
    out = (C.c_int64 * 4)()
    assert _lib.lib().p7x_debug_memory_stats(0, out) == 0, _lib.last_error()
    return tuple(out)


@pytest.mark.parametrize("key", T.OVERFLOW_KEYS)
def test_hmmalign_overflow_names_the_same_sequence_as_the_host_twin(key):
    """Family b on the device: OverflowError, naming the sequence the host twin names for the same block -- two overflowing
    sequences, the shorter one first, between two that align (the device works longest first, the host twin in input
    order).  The neighbours alone align afterwards on the buffers the failed calls gave back."""
    hmm = T.model(key)
    fine = T.targets("rnd40" if key == "rnd45" else key, "a")
    both = sorted(T.targets(key, "b"), key=lambda t: len(t[1]))
    assert len(both[0][1]) < len(both[1][1])
    bad = T.block(hmm.alphabet, [fine[0]] + both + [fine[1]])
    good = T.block(hmm.alphabet, fine)
    aligner = plan7.TraceAligner()
    first = aligner.compute_traces(hmm, good)
    messages = []
    for host in (True, False, False):
        _lib.set_debug_option("host_align", 1 if host else -1)
        try:
            with pytest.raises(OverflowError) as err:
                aligner.compute_traces(hmm, bad)
        finally:
            _lib.set_debug_option("host_align", -1)
        messages.append(str(err.value))
        del err                     # (its traceback holds the call's optimized profile, whose device image would stay out of the pool)
        gc.collect()
        if not host:
            messages.append(_memory_stats())
    host_msg, dev_msg, stats1, dev_msg2, stats2 = messages
    assert repr(both[0][0]) in host_msg and f"L = {len(both[0][1])}" in host_msg, host_msg
    assert dev_msg == host_msg == dev_msg2, (dev_msg, host_msg)
    again = aligner.compute_traces(hmm, good)
    stats3 = _memory_stats()
    print(f"[dp-reference] overflow {key}: {dev_msg!r}; memory after the failed calls {stats1} {stats2}, after the next {stats3}", file=sys.stderr)
    assert again == first and all(len(t.st) for t in again)
    assert (stats2[0], stats2[2]) == (stats1[0], stats1[2])          # the second failed call found the first one's buffers
    assert (stats3[0], stats3[2]) == (stats1[0], stats1[2])          # and the neighbours theirs


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_search_domain_decoding_against_the_reference(key, oracle):
    """Families a and b among 50 random targets under the default pipeline.  nexpected against the reference's btot[L]:
    every term exp(fB + bB - total) is formed from three special-state logs, each within E_row max(|log|, 1) of the
    reference's in the oracle, so its relative error is at most 3 E_row S (S: the largest |log| of the target's special
    states), the device may take DEVICE_FACTOR times that, and a float32 running sum of L positive terms adds at most
    L 2^-24.  The regions and every domain's envelope are the host stage's (p7x_postprocess_targets on the oracle's rows)."""
    hmm = T.model(key)
    named = _families(key, "ab")
    block = easel.DigitalSequenceBlock(hmm.alphabet, list(T.block(hmm.alphabet, named)) + list(synthetic_block(50, 200, seed=hmm.M)))
    hits = plan7.Pipeline(hmm.alphabet).search_hmm(hmm, plan7.SequenceDatabase(block))
    twin = host_pipeline.host_search(oracle, hmm, block)
    fields = lambda hs: {h.name: (h.nregions, [(d.env_from, d.env_to) for d in h.domains]) for h in hs}
    got, want = fields(hits), fields(twin)
    assert got == want
    by_name = {h.name: h for h in hits}
    worst = 0.0
    for name, seq in named:
        assert name in by_name, name
        ref = T.reference(key, name, seq, True)
        btot, etot, mocc = ref.domain_decoding()
        S = max(1.0, float(np.abs(ref.fx[np.isfinite(ref.fx)]).max()), float(np.abs(ref.bx[np.isfinite(ref.bx)]).max()))
        rel = DEVICE_FACTOR * 3.0 * MEASURED[key]["row"] * S + len(seq) * 2.0 ** -24
        h = by_name[name]
        err = abs(h.nexpected - btot[-1])
        worst = max(worst, err / btot[-1])
        print(f"[dp-reference] search {name}: nexpected {h.nexpected:.6f} btot[L] {btot[-1]:.6f} rel diff {err / btot[-1]:.2e} "
              f"bound {rel:.2e}; regions {h.nregions}", file=sys.stderr)
        assert err <= rel * btot[-1], (name, h.nexpected, btot[-1])
        assert h.nregions == len(region_scan(btot, etot, mocc)), name
    print(f"[dp-reference] search {key}: {len(named)} tandem targets among {len(block)}, worst relative nexpected difference {worst:.2e}", file=sys.stderr)
