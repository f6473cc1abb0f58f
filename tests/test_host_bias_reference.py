"""The float32 bias filter on the host -- the oracle's p7o_bias_filter and the product's host twin bias_filter_score (seam
p7x_debug_bias_filter_host; what the F3 guard and the long-target windows score with) -- against the float64 reference of
tests/bias_reference.py, on the targets of tests/bias_targets.py.

The reference is pinned by itself first: its Forward equals the sum over all enumerated state paths, and its two forms
(one target at a time, all targets of a length at a time) agree.  The bounds below are CPU_FACTOR times what these tests
measured (profiles/r20_bias_reference.md; the engines are deterministic, the factor leaves room for another libm), with
the float32 floor of a running sum under them; tests/test_gpu_bias_reference.py derives the device's bounds from them."""
import ctypes as C
import math

import numpy as np
import pytest

import bias_reference as R
import bias_targets as T
from pyhmmer_amd import _lib

# What these tests measured: nats, the larger of |oracle - reference| and |host twin - reference| over the scored targets
# of a family (the two engines agree bit for bit on every target here, see the note); family b by length (T.label); dec:
# the MSV survivors of the decision block, for the three models that search it.
MEASURED = {
    "rnd1": dict(a=1.6e-05, b17=3.0e-06, b300=9.2e-04, b5000=2.6e-01, c=4.6e-07, d=6.8e-07),
    "rnd7": dict(a=4.1e-06, b17=2.2e-06, b300=7.7e-04, b5000=3.0e-01, c=5.1e-07, d=6.4e-07),
    "rnd8": dict(a=7.7e-07, b17=2.8e-07, b300=1.2e-03, b5000=3.2e-01, c=2.2e-07, d=7.0e-07),
    "rnd9": dict(a=5.4e-06, b17=5.6e-06, b300=1.0e-03, b5000=3.2e-01, c=3.2e-07, d=7.1e-07),
    "rnd262": dict(a=1.3e-05, b17=1.7e-06, b300=9.7e-04, b5000=1.9e-01, c=4.8e-07, d=6.7e-07, dec=2.1e-05),
    "rnd2048": dict(a=1.9e-05, b17=2.0e-06, b300=1.1e-03, b5000=2.1e-01, c=2.9e-07, d=6.7e-07),
    "rnd8192": dict(a=2.4e-05, b17=1.4e-06, b300=1.4e-03, b5000=1.4e-01, c=3.5e-07, d=7.6e-07),
    "KR": dict(a=2.3e-05, b17=6.2e-08, b300=6.7e-06, b5000=4.0e-05, c=1.7e-07, d=6.0e-07),
    "LuxC": dict(a=8.5e-06, b17=1.9e-07, b300=1.6e-04, b5000=2.1e-02, c=5.6e-07, d=7.4e-07, dec=1.6e-06),
    "dna": dict(a=1.1e-06, b17=2.9e-07, b300=2.8e-05, b5000=1.1e-02, c=4.3e-07, d=6.6e-07),
    "zero": dict(a=1.9e-06, b17=7.0e-07, b300=7.0e-04, b5000=1.6e-01, c=4.2e-07, d=6.2e-07, dec=1.4e-05),
    "bg": dict(a=1.1e-05, b17=5.4e-06, b300=6.5e-04, b5000=3.7e-01, c=4.4e-07, d=1.1e-06),
}
CPU_FACTOR = 2.0
# A float32 running sum whose partial sums reach S is not known better than a few ulps of S, whatever the engine: the bound
# of a target is max(CPU_FACTOR x measured, REL_SCORE x S), S from the reference (the convention of the parsers' tests).
REL_SCORE = 1e-6
BIAS_TOL_NATS = 1e-3          # the flat tolerance of tests/test_gpu_filters.py, for the note only


def bound(key, family, S, factor=CPU_FACTOR):
    return max(factor * MEASURED[key][family], REL_SCORE * S)


@pytest.fixture
def report(capsys):
    """One line on the terminal whatever the capture mode: the measured figures belong to the run's output."""
    def emit(line):
        with capsys.disabled():
            print("\n[bias-reference] " + line, end="", flush=True)
    return emit


def twin(om, seq):
    """bias_filter_score of the product's host stage on seq (Easel layout: sentinel, residues, sentinel)."""
    d = np.full(len(seq) + 2, 255, dtype=np.uint8)
    d[1:-1] = seq
    sc = C.c_float()
    st = _lib.lib().p7x_debug_bias_filter_host(om._handle, d.ctypes.data, len(seq), C.byref(sc))
    assert st == 0, _lib.last_error()
    return sc.value


# ------------------------------------------------------------------------------------------------ the reference by itself
@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_reference_forward_is_the_sum_over_all_paths(libp7x, key, report):
    """Every target of 1-8 residues of a sweep -- canonical residues, every degenerate and special code, the residues with
    the extreme odds -- against the sum of the probabilities of all 2^L state paths, to 1e-12 relative."""
    rm = T.ref_model(key)
    abc = rm.alphabet
    rng = np.random.default_rng([sum(key.encode()), 9])
    order = np.argsort(rm.odds[:abc.K])
    sweep = []
    for L in range(1, 9):
        sweep += [rng.integers(0, abc.K, L), rng.integers(0, abc.Kp, L), np.full(L, order[0]), np.full(L, order[-1]),
                  np.resize(np.array([order[-1], order[0]]), L)]
    sweep += [np.array([x]) for x in range(abc.Kp)] + [np.array([order[-1], x, order[-1]]) for x in range(abc.K, abc.Kp)]
    worst = 0.0
    for seq in sweep:
        got, want = R.filter_score(rm, seq).forward, R.enumerate_paths(rm, seq)
        rel = abs(math.expm1(got - want))             # of the sums themselves (their logs can be 1e-8: one state, odds 1)
        worst = max(worst, rel)
        assert rel <= 1e-12, (key, seq.tolist(), got, want)
    report(f"self-check {key}: Forward = sum over enumerated paths on {len(sweep)} targets, worst relative {worst:.1e}")


def test_reference_parameters_are_the_float32_values(libp7x):
    """L1 = M / 8 for every M = 1 ... 8,192, the length model of every L up to 20,000, the odds table of a profile."""
    f32 = np.float32
    abc = T.model("KR")[0].alphabet
    flat = np.full(abc.K, 1.0 / abc.K, dtype=f32)
    for M in range(1, 8193):
        m = R.FilterModel(abc, M, flat, flat)
        L1 = M / 8.0                                               # exact in either precision
        assert m.t10 == float(f32(1.0) / f32(L1 + 1.0)) and m.t11 == float(f32(L1) / f32(L1 + 1.0)), M
        assert abs(m.t10 + m.t11 - 1.0) <= 2.0 ** -23, M
    for L in (1, 2, 3, 400, 20_000, 100_000):
        p1, q1 = R.FilterModel(abc, 8, flat, flat).length(L)
        assert p1 == float(f32(L) / f32(L + 1)) and q1 == float(f32(1.0) - f32(p1)) and abs(p1 - L / (L + 1.0)) <= 2.0 ** -24
    for key in T.MODEL_KEYS:
        hmm, bg = T.model(key)
        rm = T.ref_model(key)
        K = hmm.alphabet.K
        compo = T.composition(key)
        assert hmm.composition is None or np.array_equal(compo, hmm.composition.astype(f32)), key
        assert np.array_equal(rm.odds[:K], (compo / bg.residue_frequencies.astype(f32)).astype(np.float64)), key
        assert np.all(rm.odds[[K, rm.Kp - 2, rm.Kp - 1]] == 1.0)
        lo, hi = rm.odds[:K].min(), rm.odds[:K].max()
        assert np.all((rm.odds[K + 1:rm.Kp - 2] >= lo) & (rm.odds[K + 1:rm.Kp - 2] <= hi)), key       # a ratio of sums lies between the ratios
    assert np.count_nonzero(T.ref_model("zero").odds == 0.0) >= 2                         # U stands for C alone: three rows
    default = T.model("KR")[1].residue_frequencies
    assert np.abs(T.model("bg")[1].residue_frequencies / default - 1.0).max() > 0.5


def test_reference_by_length_equals_the_reference_of_one_target(libp7x):
    """The vectorised form used for the 70,000-target family against the scalar form, on the family's first 300 targets."""
    for key in ("rnd8", "dna", "zero"):
        dsq, offsets, lengths = T.family_d(key)
        rm = T.ref_model(key)
        sc, S = R.filter_scores_by_length(rm, dsq, offsets[:300], lengths[:300])
        for t in range(300):
            one = R.filter_score(rm, dsq[offsets[t]:offsets[t] + lengths[t]])
            assert abs(sc[t] - one.filtersc) <= 1e-13 * max(1.0, abs(one.filtersc)) and abs(S[t] - one.S) <= 1e-13 * max(1.0, one.S), (key, t)
        if key == "rnd8":          # the whole family in one call: the same figures for its first targets
            full = T.reference_d(key)
            assert full[0].shape == (T.MANY,) and np.allclose(full[0][:300], sc, rtol=1e-13, atol=1e-13) and np.allclose(full[1][:300], S, rtol=1e-13, atol=1e-13)
            assert int(lengths.min()) == 1 and int(lengths.max()) == 40 and (dsq[offsets - 1] == 255).all()


def test_gumbel_tail_in_float64():
    """ln P through expm1 against the two branches upstream takes, and |d ln P / d x| <= lambda (the decision test's margin)."""
    mu, lam = -9.0, 0.69
    for x in np.linspace(-20.0, 60.0, 321):
        lnp = R.gumbel_ln_survival(x, mu, lam)
        ey = -math.exp(-lam * (x - mu))
        direct = -ey if abs(ey) < 5e-9 else 1.0 - math.exp(ey)
        assert abs(math.exp(lnp) - direct) <= 3e-9 * direct + 3e-16          # upstream takes P = exp(-y) below 5e-9: off by P / 2 relative; above, 1 - exp() cancels
        slope = (R.gumbel_ln_survival(x + 1e-4, mu, lam) - lnp) / 1e-4
        assert -lam * (1.0 + 1e-6) <= slope <= 0.0
    assert R.ln_pvalue(math.inf, -3.0, mu, lam) == -math.inf


# ------------------------------------------------------------------------------------------------ engines against reference
def measure(key, engine):
    """{label: [(name, |engine - reference|, S)]} over the scored targets of families a, b, c and the first HOST_D of d."""
    rows = {f: [] for f in T.FAMILIES}
    for family in "abc":
        for name, seq, ref in T.reference(key, family):
            rows[T.label(family, seq)].append((name, abs(float(engine(seq)) - ref.filtersc), ref.S))
    dsq, offsets, lengths = T.family_d(key)
    sc, S = T.reference_d(key)
    for t in range(T.HOST_D):
        rows["d"].append((f"d{t}", abs(float(engine(dsq[offsets[t]:offsets[t] + lengths[t]])) - sc[t]), S[t]))
    return rows


@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_oracle_and_host_twin_against_the_reference(libp7x, oracle, key, report):
    """Families a, b (by length), c and d: every score of the oracle and of the host twin within max(CPU_FACTOR x the recorded
    figure, REL_SCORE x S) of the reference.  The line names the worst target, whether the two engines gave the same floats,
    which of the two terms bounds the family, and the targets on which the oracle itself is further from the reference
    than the flat tolerance of tests/test_gpu_filters.py."""
    hmm, bg = T.model(key)
    op = oracle.OracleProfile(hmm, bg, 400)
    om = T.profile(key)
    by_oracle, by_twin = measure(key, op.bias), measure(key, lambda s: twin(om, s))
    line, record, failures = [], [], []
    for f in T.FAMILIES:
        e_o, e_t = max(r[1] for r in by_oracle[f]), max(r[1] for r in by_twin[f])
        worst = max(by_oracle[f] + by_twin[f], key=lambda r: r[1])
        Smax = max(r[2] for r in by_oracle[f])
        same = all(o[1] == t[1] for o, t in zip(by_oracle[f], by_twin[f]))
        measured = MEASURED[key][f]
        governs = "floor" if REL_SCORE * Smax > CPU_FACTOR * measured else "measured"
        over = [name for name, err, _ in by_oracle[f] if err > BIAS_TOL_NATS]
        line.append(f"{f}: oracle {e_o:.2e} twin {e_t:.2e}{' (same floats)' if same else ''} at {worst[0]}, S <= {Smax:.0f}, bound: {governs}"
                    + (f", oracle over {BIAS_TOL_NATS:g} on {' '.join(over)}" if over else ""))
        record.append(f"{f}={max(e_o, e_t):.1e}")
        for who, rows in (("oracle", by_oracle[f]), ("twin", by_twin[f])):
            failures += [(f, who, name, err, bound(key, f, S)) for name, err, S in rows if not err <= bound(key, f, S)]
    report(f"{key} (M {hmm.M}): " + "; ".join(line))
    report(f"{key} measured: dict({', '.join(record)})")
    assert not failures, failures


def test_decision_block_against_the_oracle_on_the_host(libp7x, oracle, report):
    """The block of tests/test_gpu_bias_reference.py's decision test with the oracle in the device's place: its decisions
    are the reference's outside the margin of its own bound, the margin leaves out under 1 % of the MSV survivors, and at
    least 100 survivors of every model fall on each side of F1 (what the seed was chosen for)."""
    from pyhmmer_amd import easel, plan7
    dsq, offsets, lengths = T.decision_block()
    assert lengths.shape == (T.DECISION_N,) and int(lengths.min()) >= 50 and int(lengths.max()) <= 400
    pk = easel.PackedBlock.from_arrays(dsq, offsets, lengths)
    for key in T.DECISION_KEYS:
        hmm, bg = T.model(key)
        assert np.array_equal(bg.residue_frequencies, plan7.Background(hmm.alphabet).residue_frequencies)
        rec = np.frombuffer(oracle.OracleProfile(hmm, bg, 400).cascade_block(pk, want_records=True)[0], dtype=np.dtype(oracle.Record))
        survivors = np.nonzero(rec["stage"] >= 1)[0]
        refs = [R.filter_score(T.ref_model(key), dsq[offsets[t]:offsets[t] + lengths[t]]) for t in survivors]
        worst = max(abs(float(rec["filtersc"][t]) - r.filtersc) for t, r in zip(survivors, refs))
        E = [bound(key, "dec", r.S) for r in refs]
        left, npass, nfail = T.check_decisions(key, rec["stage"] >= 2, rec["usc"], [r.filtersc for r in refs], survivors, E, 0.02)
        report(f"decisions {key} (M {hmm.M}): {len(survivors)} MSV survivors, {npass} past the bias filter, {nfail} stopped, {left} left out; "
               f"oracle's filtersc within {worst:.2e} of the reference on them (recorded {MEASURED[key]['dec']:.1e})")
        assert worst <= CPU_FACTOR * MEASURED[key]["dec"]
        assert left <= 0.01 * len(survivors) and npass >= 100 and nfail >= 100, (key, left, npass, nfail)


def test_host_twin_scores_no_residue_of_an_empty_target(libp7x):
    """L = 0: the null1 score of an empty target (0 x ln 0 in float arithmetic: not a number, and never compared with a
    threshold -- a search gives empty targets no slot), whatever byte stands where residue 1 would; bad arguments are refused."""
    om = T.profile("KR")
    sc = C.c_float()
    for byte in (255, 3, 28):
        d = np.array([255, byte, 255], dtype=np.uint8)
        assert _lib.lib().p7x_debug_bias_filter_host(om._handle, d.ctypes.data, 0, C.byref(sc)) == 0
        with np.errstate(all="ignore"):
            want = np.float32(0.0) * np.log(np.float64(0.0)) + np.log(1.0)
        assert np.isnan(want) and np.isnan(sc.value)
    d = np.array([255, 29, 255], dtype=np.uint8)
    assert _lib.lib().p7x_debug_bias_filter_host(om._handle, d.ctypes.data, 1, C.byref(sc)) != 0
    assert _lib.lib().p7x_debug_bias_filter_host(om._handle, d.ctypes.data, -1, C.byref(sc)) != 0
    assert _lib.lib().p7x_debug_bias_filter_host(None, d.ctypes.data, 1, C.byref(sc)) != 0
