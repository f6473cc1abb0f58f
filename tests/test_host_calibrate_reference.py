"""The references of the calibration tests, on the host: the redraw rule of a model whose sample overflows a filter
(calibration_cases.own_stream: the oracle's filters and the two host seams), and the oracle's Forward scores of the
calibration samples against the float64 log-space reference of tests/dp_reference.py.

tests/test_gpu_calibrate_edges.py holds the device to both.  The float64 reference covers the models of up to
calibration_cases.REFERENCE_MAX_M = 1,025 nodes (about 4 s of numpy per model there); a longer model keeps the oracle and
test_gpu_calibrate.FWD_TOL as its only Forward bound."""
import numpy as np
import pytest

import calibration_cases as cc
import dp_reference as R
from conftest import random_hmm
from pyhmmer_amd import _lib, easel, plan7
from test_host_builder import N, fit, oracle_scores, sample, stream_of
from test_host_dp_reference import CPU_FACTOR

# max over the 200 Forward samples of |oracle's float32 score - float64 reference| in nats, on the model's own final stream
# (seed 42), multihit, length model 100: what test_oracle_forward_against_the_reference measured.  The CPU bound is
# CPU_FACTOR times the figure; the device's bound (tests/test_gpu_calibrate_edges.py) is derived from it.
MEASURED = {
    "msv5": 1.1e-6, "vit50": 9.7e-7, "both": 1.1e-6, "msv5+msv6": 1.1e-6, "vit199": 9.8e-7, "vit50half": 8.9e-7,
    "gappy64": 1.2e-6, "gappy65": 1.4e-6, "gappy320": 1.3e-6, "gappy641": 1.2e-6, "gappy1024": 1.1e-6, "gappy1025": 1.1e-6,
    "PF02826": 8.1e-7, "KR": 1.2e-6, "LuxC": 1.1e-6, "RREFam/0": 7.5e-7, "RREFam/1": 8.7e-7,
    "dna50": 9.1e-7, "dna64": 8.6e-7, "dna65": 1.0e-6, "dna129": 8.6e-7,                 # (the RNA models are the DNA models
    "rna50": 9.1e-7, "rna64": 8.6e-7, "rna65": 1.0e-6, "rna129": 8.6e-7,                 #  under the other alphabet code)
    "gappy64/uniform": 1.1e-6, "gappy65/uniform": 1.0e-6, "gappy320/uniform": 1.0e-6,
    "PF02826/uniform": 1.0e-6, "KR/uniform": 1.2e-6, "RREFam/0/uniform": 1.2e-6, "RREFam/1/uniform": 1.0e-6,
}


@pytest.fixture
def report(capsys):
    def emit(line):
        with capsys.disabled():
            print("\n[calibrate-reference] " + line, end="", flush=True)
    return emit


def _reference_models():
    gappy = cc.gappy_models(sorted({M for M in cc.GAPPY_HOST_M + cc.GAPPY_GPU_M if M <= cc.REFERENCE_MAX_M}))
    plain = [(n, h, False) for n, h in cc.overflow_models() + gappy + cc.fixture_models() + cc.nucleotide_models()]
    uniform = [(n, h, True) for n, h in gappy + cc.fixture_models() if h.M <= cc.UNIFORM_MAX_M]
    return [(n + ("/uniform" if u else ""), n, h, u) for n, h, u in plain + uniform if h.M <= cc.REFERENCE_MAX_M]


# ------------------------------------------------------------------------------------------------ the redraw rule
def test_overflow_models_take_the_streams_of_the_table(libp7x, oracle):
    """Every overflow model: the kept sample that overflows first in every round and the draws thrown away at the end are
    the table's, the final stream has no overflow left and fits.  `both` (kept 249 is draw 250 once draw 5 is gone) and
    `msv5+msv6` (kept 5 overflows twice: draws 5 and 6) tell a draw's number from a kept sample's; in `vit199` the redraw
    pulls 200 residues across the Viterbi / Forward boundary, so every Forward sample is another one."""
    abc = cc.amino()
    common = stream_of(plan7.Background(abc))
    for name, hmm in cc.overflow_models():
        o = cc.own_stream_of(oracle, name, hmm)
        firsts, skipped = cc.OVERFLOW_TABLE[name]
        assert (o.firsts, o.skipped) == (firsts, skipped), (name, o.firsts, o.skipped)
        assert not o.ovf.any() and o.status == 0 and np.all(np.isfinite(o.ev)), name
        assert int(o.raw[0].min()) >= 0 and int(o.raw[1].max()) < 32767, name
        assert np.array_equal(o.stream, cc.redraw(plan7.Background(abc), 3, 42, skipped)), name
        assert not np.array_equal(o.stream, common), name
    o = cc.own_stream_of(oracle, "vit199", dict(cc.overflow_models())["vit199"])
    assert all(not np.array_equal(sample(o.stream, 2, i), sample(common, 2, i)) for i in range(N))
    assert np.array_equal(sample(o.stream, 1, 199), np.concatenate([sample(common, 2, 0), sample(common, 2, 1)]))


def test_common_stream_is_refused_for_an_overflow_model(libp7x, oracle):
    """`msv5` against the common stream: sample 5 is marked, and the fit returns the range status naming it."""
    name, hmm = cc.overflow_models()[0]
    bg = plan7.Background(hmm.alphabet)
    sc, ovf, raw = oracle_scores(oracle.OracleProfile(hmm, bg, 100), stream_of(bg))
    assert cc.first_overflow(ovf) == 5
    mh = _lib.lib().p7x_oprofile_match_relent(plan7.OptimizedProfile(hmm, bg, 100)._handle)
    st, _ = fit(sc, ovf, mh)
    assert st == 16 and "sample 5 " in _lib.last_error()


def test_gap_rich_and_nucleotide_models_through_own_stream(libp7x, oracle, report):
    """gappy_hmm(M, 5) and random_hmm(M, 3, dna / rna): whether or not a sample overflows, own_stream ends on a stream that
    the oracle scores without overflow, that is the redraw of its skipped draws, and that fits; nucleotide streams hold
    canonical residues only."""
    for name, hmm in cc.gappy_models(cc.GAPPY_HOST_M) + cc.nucleotide_models():
        bg = cc.background_of(hmm)
        o = cc.own_stream_of(oracle, name, hmm)
        report(f"{name}: M = {hmm.M}, skipped {o.skipped}, tau {float(o.ev[4]):.4f}")
        assert len(o.skipped) < cc.MAX_ROUNDS and o.skipped == sorted(set(o.skipped)), name
        assert not o.ovf.any() and o.status == 0 and np.all(np.isfinite(o.ev)), name
        assert int(o.stream.max()) < hmm.alphabet.K, name
        assert np.array_equal(o.stream, cc.redraw(bg, hmm.alphabet.type_code, 42, o.skipped)), name
        sc, ovf, raw = oracle_scores(oracle.OracleProfile(hmm, bg, 100), o.stream)
        assert np.array_equal(raw, o.raw) and np.array_equal(sc, o.sc) and not ovf.any(), name


# ------------------------------------------------------------------------------------------------ float64 Forward
def test_forward_reference_is_the_sum_over_all_paths(libp7x, report):
    """Where the reference and not the oracle decides: on models of two and three nodes and Forward samples cut to four
    residues, forward_backward under the length model of 100 equals the sum over the enumerated paths."""
    worst, n = 0.0, 0
    for abc in (cc.amino(), easel.Alphabet.dna()):
        stream = stream_of(plan7.Background(abc), abc_type=abc.type_code)
        for M in (2, 3):
            hmm = random_hmm(M, seed=910 + M, alphabet=abc)
            om = plan7.OptimizedProfile(hmm, plan7.Background(abc), 100)
            rm = R.RefModel.from_oprofile(om)
            for i in (0, 1, 199):
                seq = sample(stream, 2, i)[:4]
                got = R.forward_backward(rm, seq, True, length=100, backward=False).fwd
                want = R.enumerate_paths(rm, seq, True, length=100)
                worst, n = max(worst, abs(got - want) / abs(want)), n + 1
                assert abs(got - want) <= 1e-12 * abs(want), (abc, M, i, got, want)
    report(f"Forward (length model 100) = sum over enumerated paths on {n} cases, worst relative {worst:.1e}")
    # and forward_reference is that function over the 200 whole samples
    abc = cc.amino()
    hmm = random_hmm(3, seed=913)
    om = plan7.OptimizedProfile(hmm, plan7.Background(abc), 100)
    stream = stream_of(plan7.Background(abc))
    ref = cc.forward_reference(om, stream)
    assert ref.shape == (N,) and ref.dtype == np.float64 and cc.forward_reference(om, stream) is ref
    rm = R.RefModel.from_oprofile(om)
    for i in (0, 7, 199):
        assert ref[i] == R.forward_backward(rm, sample(stream, 2, i), True, length=100, backward=False).fwd


@pytest.mark.parametrize("key,name,hmm,uniform", [pytest.param(*c, id=c[0]) for c in _reference_models()])
def test_oracle_forward_against_the_reference(libp7x, oracle, report, key, name, hmm, uniform):
    """All 200 Forward samples of the model's final stream: the oracle's float32 score within CPU_FACTOR times the recorded
    distance from the float64 reference."""
    o = cc.own_stream_of(oracle, name, hmm, uniform)
    om = plan7.OptimizedProfile(hmm, cc.background_of(hmm, uniform), 100)
    ref = cc.forward_reference(om, o.stream)
    d = float(np.max(np.abs(o.sc[2].astype(np.float64) - ref)))
    report(f"{key}: M = {hmm.M}, max |oracle - float64| {d:.2e} nat over {N} samples (recorded {MEASURED[key]:.1e}), max |score| {float(np.abs(ref).max()):.2f}")
    assert np.all(np.isfinite(ref))
    assert d <= CPU_FACTOR * MEASURED[key], (key, d, MEASURED[key])
