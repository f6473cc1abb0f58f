"""What a long-target search reports for an envelope -- orig (unihit Forward over the envelope with the profile's own odds,
the record's envsc), domcorrection (what the composition-adjusted odds take from it) and oasc (optimal accuracy under the
adjusted odds) -- from the float32 implementations on the host, the oracle (oracle_lib.lt_domains, oracle_lib.lt_envelope_scores)
and the product's host stage (host_pipeline.host_nhmmer, whose envelopes are the host workers'), against the float64 reference
of tests/lt_envelope_reference.py on the targets of tests/lt_envelope_targets.py.  Each envelope is taken at the coordinates
the implementation itself reports.

The reference is pinned by itself first: with s = 1 the adjusted table is the profile's own, Forward with overridden odds is
the sum over enumerated paths, a degenerate row and the fractional counts against values worked out by hand.

The bounds are CPU_FACTOR times what these tests measured on the oracle (MEASURED_LT, profiles/r16_lt_envelope_reference.md);
tests/test_gpu_lt_envelope_reference.py derives the device's from them.  Floors, where the oracle happens to sit on the
reference (floors()): 1e-6 |orig| for the score and Ld 2^-23 for oasc as in tests/test_host_envelope_reference.py; for
domcorrection Ld 2^-23 as there, plus Ld 2^-23 for each of the two roundings (logf, expf) that every emitted odds of the
per-envelope table has gone through and the profile's own table has not: 3 Ld 2^-23.  No bound comes from the code under
test."""
import math
import time

import numpy as np
import pytest

import dp_reference as R
import host_pipeline
import lt_envelope_reference as LR
import lt_envelope_targets as T
import lt_oracle_check
from conftest import random_hmm
from pyhmmer_amd import plan7

# Largest |oracle - reference| per label over its envelopes: orig and corr (domcorrection) in nats, oasc in posterior units.
MEASURED_LT = {
    "rnd48": dict(orig=3.3e-07, corr=1.7e-06, oasc=1.1e-05),
    "rnd64": dict(orig=1.1e-06, corr=1.5e-06, oasc=1.3e-05),
    "rnd65": dict(orig=1.7e-06, corr=2.1e-06, oasc=5.3e-05),
    "rnd128": dict(orig=2.1e-06, corr=4.0e-06, oasc=1.0e-04),
    "rnd129": dict(orig=2.0e-06, corr=3.5e-06, oasc=4.9e-05),
    "rnd192": dict(orig=5.2e-06, corr=4.8e-06, oasc=9.0e-05),
    "rnd193": dict(orig=3.2e-06, corr=3.8e-06, oasc=1.1e-04),
    "rnd256": dict(orig=3.7e-06, corr=5.6e-06, oasc=1.1e-04),
    "rnd257": dict(orig=2.4e-06, corr=3.6e-06, oasc=7.5e-05),
    "rnd320": dict(orig=1.1e-06, corr=6.6e-06, oasc=1.2e-04),
    "rnd321": dict(orig=6.1e-06, corr=8.7e-06, oasc=2.7e-04),
    "rnd384": dict(orig=3.7e-06, corr=1.3e-05, oasc=1.5e-04),
    "rnd385": dict(orig=4.4e-06, corr=3.0e-06, oasc=1.3e-04),
    "rnd512": dict(orig=6.0e-06, corr=1.0e-05, oasc=1.9e-04),
    "rnd513": dict(orig=4.9e-06, corr=8.2e-06, oasc=2.7e-04),
    "rnd640": dict(orig=6.9e-07, corr=4.6e-06, oasc=1.0e-04),
    "rnd641": dict(orig=1.9e-06, corr=3.9e-06, oasc=1.2e-04),
    "rnd768": dict(orig=2.3e-06, corr=3.6e-06, oasc=7.4e-05),
    "rnd769": dict(orig=9.2e-06, corr=8.3e-06, oasc=1.4e-04),
    "rnd1024": dict(orig=4.5e-06, corr=4.3e-06, oasc=1.3e-04),
    "rnd1025": dict(orig=6.0e-06, corr=5.9e-06, oasc=1.5e-04),
    "rnd1280": dict(orig=5.8e-06, corr=7.0e-06, oasc=1.2e-04),
    "rnd1281": dict(orig=2.1e-06, corr=4.7e-06, oasc=1.8e-04),
    "rnd1536": dict(orig=3.6e-06, corr=2.8e-06, oasc=2.1e-04),
    "rnd1537": dict(orig=1.7e-06, corr=9.5e-06, oasc=1.4e-04),
    "rnd2048": dict(orig=3.9e-06, corr=7.3e-06, oasc=1.6e-04),
    "rnd2049": dict(orig=3.2e-06, corr=1.0e-05, oasc=2.4e-04),
    "rnd3072": dict(orig=4.1e-06, corr=8.0e-06, oasc=4.6e-05),
    "rnd3073": dict(orig=2.9e-06, corr=7.9e-06, oasc=9.6e-05),
    "rnd4096": dict(orig=3.1e-06, corr=4.1e-06, oasc=1.6e-04),
    "rnd4097": dict(orig=1.6e-06, corr=1.2e-05, oasc=9.4e-05),
    "rnd6144": dict(orig=2.3e-06, corr=9.5e-06, oasc=7.6e-05),
    "rnd6145": dict(orig=3.0e-06, corr=8.6e-06, oasc=1.4e-04),
    "rnd8192": dict(orig=2.0e-06, corr=9.7e-06, oasc=9.8e-05),
    "rnd8193": dict(orig=2.5e-06, corr=3.0e-06, oasc=9.3e-05),
    "rnd12288": dict(orig=3.1e-06, corr=1.2e-05, oasc=2.2e-04),
    "rnd1100 long": dict(orig=8.5e-05, corr=1.1e-04, oasc=2.1e-03),
    "rnd300 edges": dict(orig=3.9e-06, corr=1.1e-05, oasc=3.4e-04),
    "rnd320 queue": dict(orig=6.5e-06, corr=1.8e-05, oasc=2.6e-04),          # T.QUEUE_LABEL: 17 envelopes of 16 fragments (profiles/r29_envelope_queue.md)
}
CPU_FACTOR = 2.0
DEVICE_FACTOR = 4.0               # another association of the same float32 terms
S1_TABLE_TOL = 2.0 ** -21         # log odds: the float32 roundings of the profile's table (quotient, logf, expf, the log read back)
_T0 = []
_oracle_cache = {}


def floors(ref):
    return dict(orig=1e-6 * abs(ref.orig), corr=3 * ref.Ld * 2.0 ** -23, oasc=ref.Ld * 2.0 ** -23)


def bounds(label, ref, factor):
    fl = floors(ref)
    return {what: max(factor * MEASURED_LT[label][what], fl[what]) for what in ("orig", "corr", "oasc")}


@pytest.fixture(autouse=True, scope="module")
def _clock():
    _T0.append(time.time())
    yield


@pytest.fixture
def report(capsys):
    def emit(line):
        with capsys.disabled():
            print(f"\n[lt-envelope-reference] {line}  ({time.time() - _T0[0]:.0f} s)", end="", flush=True)
    return emit


class Worst:
    """The largest distances of a set of envelopes from the reference."""

    def __init__(self):
        self.d = dict(orig=0.0, corr=0.0, oasc=0.0)
        self.n = 0

    def add(self, ref, orig, corr, oasc=None):
        got = dict(orig=abs(orig - ref.orig), corr=abs(corr - ref.domcorrection))
        if oasc is not None:
            got["oasc"] = abs(oasc - ref.oasc)
            self.n += 1
        for what, v in got.items():
            self.d[what] = max(self.d[what], v)
        return got

    def line(self):
        return f"{self.n} envelopes: orig {self.d['orig']:.2e} corr {self.d['corr']:.2e} nats, oasc {self.d['oasc']:.2e}"


# ------------------------------------------------------------------------------------------------ the reference by itself
def _small(M, seed):
    hmm = random_hmm(M, seed=seed, alphabet=T.dna())
    bg = plan7.Background(hmm.alphabet)
    return hmm, bg.residue_frequencies, R.RefModel.from_oprofile(plan7.OptimizedProfile(hmm, bg, 400))


def test_with_s_1_the_adjusted_table_is_the_profiles_own(libp7x, oracle, report):
    """s = 1: bgn is the background, so the adjusted odds are the profile's own -- canonical rows, the degenerate rows'
    expected scores and the -inf rows -- to the float32 rounding of the profile's table, and adj = orig to Ld times that."""
    degen = oracle.degeneracy_sets(4)
    worst = 0.0
    for M, seed in ((3, 1), (40, 2), (130, 3)):
        hmm, bg, rm = _small(M, seed)
        sub = np.random.default_rng(M).choice([0, 1, 2, 3, 15, 5, 10], size=60)
        bgn = LR.adjusted_background(sub, bg, degen, 1.0)
        assert np.array_equal(bgn, bg.astype(np.float64))
        e = LR.adjusted_emissions(hmm.match_emissions, bgn, degen)
        assert e.shape == rm.e.shape
        assert np.array_equal(np.isneginf(e), np.isneginf(rm.e))
        assert np.isneginf(e[[4, 16, 17], 1:M + 1]).all() and np.isfinite(e[:4, 1:M + 1]).all() and np.isfinite(e[5:16, 1:M + 1]).all()
        fin = np.isfinite(e)
        err = float((np.abs(e[fin] - rm.e[fin]) / np.maximum(1.0, np.abs(rm.e[fin]))).max())
        worst = max(worst, err)
        assert err <= S1_TABLE_TOL, (M, err)
        ref = LR.envelope(rm, hmm.match_emissions, bg, sub, degen, s=1.0)
        assert abs(ref.adj - ref.orig) <= len(sub) * S1_TABLE_TOL * 4.0, (M, ref.adj, ref.orig)      # |log odds| <= 4 on these models
        assert abs(ref.bck - ref.adj) <= 1e-9 * abs(ref.adj)
        same = LR.with_emissions(rm, rm.e)
        assert R.forward_backward(same, sub, False).fwd == ref.orig
    report(f"self-check: s = 1 table against the profile's own, worst relative difference of a log odds {worst:.1e}")


def test_forward_with_overridden_odds_is_the_sum_over_enumerated_paths(libp7x, oracle, report):
    """DNA models of 1-3 nodes, envelopes of 1-5 residues with degenerate codes among them: Forward (and Backward) under the
    adjusted odds, unihit, the envelope's own length model, equal the enumerated paths' sum to 1e-12."""
    degen = oracle.degeneracy_sets(4)
    worst, n = 0.0, 0
    for M in (1, 2, 3):
        for seed in (0, 1):
            hmm, bg, rm = _small(M, 950 + 10 * seed + M)
            for Ld in range(1, 6):
                sub = np.random.default_rng([M, seed, Ld]).choice([0, 1, 2, 3, 15, 6], size=Ld, p=[0.2, 0.2, 0.2, 0.2, 0.1, 0.1])
                ref = LR.envelope(rm, hmm.match_emissions, bg, sub, degen)
                madj = LR.with_emissions(rm, LR.adjusted_emissions(hmm.match_emissions, ref.bgn, degen))
                for got, model in ((ref.adj, madj), (ref.orig, rm)):
                    total = R.enumerate_paths(model, sub, False)
                    err = abs(got - total) / abs(total)
                    worst, n = max(worst, err), n + 1
                    assert err <= 1e-12, (M, seed, Ld, got, total)
                assert abs(ref.bck - ref.adj) <= 1e-12 * abs(ref.adj)
                assert ref.domcorrection == max(0.0, ref.orig - ref.adj) and 0.0 < ref.oasc <= Ld + 1e-12
    report(f"self-check: Forward with overridden odds = enumerated paths on {n} cases, worst relative {worst:.1e}")


def test_degenerate_rows_and_fractional_counts_by_hand(oracle):
    degen = oracle.degeneracy_sets(4)
    # A C N R Y gap * ~: A 1 + 1/4 + 1/2, C 1 + 1/4 + 1/2, G 1/4 + 1/2, T 1/4 + 1/2; the last three count nothing
    sub = np.array([0, 1, 15, 5, 6, 4, 16, 17])
    cnt = LR.composition_counts(sub, degen)
    assert np.allclose(cnt, [1.75, 1.75, 0.75, 0.75], rtol=0, atol=1e-15) and cnt.sum() == 5.0
    bg = np.array([0.25, 0.25, 0.25, 0.25], dtype=np.float32)
    bgn = LR.adjusted_background(sub, bg, degen, 0.25)
    want = 0.75 * np.array([0.35, 0.35, 0.15, 0.15]) + 0.0625
    assert np.allclose(bgn, want, rtol=0, atol=1e-15) and abs(bgn.sum() - 1.0) <= 1e-15
    assert LR.smoothing(1200) == LR.smoothing(100) == 0.25 and LR.smoothing(80) == 25.0 / 80 and LR.smoothing(10) == 0.5
    assert np.array_equal(LR.adjusted_background(np.array([4, 16, 17]), bg, degen, 0.25), bg.astype(np.float64))    # nothing to count
    mp = np.array([[0, 0, 0, 0], [0.7, 0.1, 0.1, 0.1], [0.05, 0.05, 0.6, 0.3]])
    e = LR.adjusted_emissions(mp, bgn, degen)
    assert e.shape == (18, 4)
    for k in (1, 2):
        sc = [math.log(mp[k, x] / want[x]) for x in range(4)]
        assert np.allclose(e[:4, k], sc, rtol=0, atol=1e-15)
        by_hand = {5: (0, 2), 6: (1, 3), 10: (0, 3), 12: (1, 2, 3), 15: (0, 1, 2, 3)}          # R Y W B N
        for code, members in by_hand.items():
            exp = sum(want[x] * sc[x] for x in members) / sum(want[x] for x in members)
            assert abs(e[code, k] - exp) <= 1e-15, (code, k)
    assert np.isneginf(e[[4, 16, 17]]).all() and np.isneginf(e[:, 0]).all() and np.isneginf(e[:, 3]).all()


def test_reported_numbers_follow_the_scoring_rule_of_the_oracle(libp7x, oracle):
    """LR.reported against oracle_lib.lt_domain_score (the rule the reference's nhmmer tables pin), to float32 rounding."""
    hmm, _, _ = _small(40, 2)
    op = oracle.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400)
    for env_len, ali_len, envsc, corr in ((250, 230, 180.25, 1.5), (1300, 1290, 700.5, 0.0), (101, 101, 55.125, 3.25)):
        want, bias, _ = oracle.lt_domain_score(op, 1200, env_len, ali_len, envsc, corr)
        sc, b = LR.reported(envsc, corr, env_len, ali_len, 1200)
        assert abs(sc - want) <= 2e-6 * abs(want) and abs(b - bias) <= 1e-6 * abs(bias), (sc, want, b, bias)


# ------------------------------------------------------------------------------------------------ the oracle's windows
def oracle_case(oracle, label):
    """Once per label: the oracle's Forward-passing windows of the label's target as (lo, hi, reverse strand, length) in target
    coordinates, and the oracle's envelopes in them as (lo, hi, reverse strand, orig, domcorrection, oasc, window length)."""
    if label in _oracle_cache:
        return _oracle_cache[label]
    hmm = T.model(label)
    seq, _ = T.target(label)
    pli = T.pipeline()
    op, max_length, units, _ = lt_oracle_check.oracle_windows(pli, hmm, seq)
    assert max_length == T.WINDOW_LENGTH
    wins, envs = [], []
    for (i, n, strand), win in units.items():
        blk = seq[i:i + n] if strand == 0 else host_pipeline.DNA_COMP[seq[i:i + n][::-1]]
        pos = (lambda b: i + b) if strand == 0 else (lambda b: i + n - b + 1)           # block coordinate -> target coordinate
        for w in win:
            ws, wl = int(w[0]), int(w[1])
            a, b = sorted((pos(ws), pos(ws + wl - 1)))
            wins.append((a, b, strand == 1, wl))
            rows, _ = oracle.lt_domains(op, blk[ws - 1:ws - 1 + wl], do_null2=pli.null2, seed=pli.seed)
            for e in rows:
                lo, hi = sorted((pos(ws - 1 + int(e[0])), pos(ws - 1 + int(e[1]))))
                envs.append((lo, hi, strand == 1, float(e[6]), float(e[7]), float(e[8]), wl))
    _oracle_cache[label] = (op, wins, envs)
    return _oracle_cache[label]


def windows_are_long(wins, lo, hi, rev):
    """The condition under which s = 0.25: an oracle window holds the envelope, and every one that does has 100 residues or
    more (the hit does not carry its window's length)."""
    held = [wl for (a, b, wrev, wl) in wins if wrev == rev and a <= lo and hi <= b]
    assert held and min(held) >= 100, (lo, hi, rev, held)


def all_planted_found(label, found):
    """found: [(lo, hi, reverse strand)] of what was reported."""
    for p in T.target(label)[1]:
        assert any(T.covers(p, *f) for f in found), (label, p, found)


# ------------------------------------------------------------------------------------------------ oracle against reference
def oracle_distances(oracle, label):
    op, wins, envs = oracle_case(oracle, label)
    seq, _ = T.target(label)
    w = Worst()
    for (lo, hi, rev, orig, corr, oasc, wl) in envs:
        assert wl >= 100
        ref = T.reference(label, lo, hi, rev)
        w.add(ref, orig, corr, oasc)
        sub = T.strand_residues(seq, lo, hi, rev)
        if sub.max() < 4:                       # lt_envelope_scores: canonical residues only
            o2, a2 = oracle.lt_envelope_scores(op, sub, wl)
            w.add(ref, o2, max(0.0, o2 - a2))
    all_planted_found(label, [e[:3] for e in envs])
    return w


@pytest.mark.parametrize("label", T.LABELS + (T.QUEUE_LABEL,))
def test_oracle_envelopes_against_the_reference(libp7x, oracle, label, report):
    w = oracle_distances(oracle, label)
    report(f"oracle {label}: {w.line()}")
    assert w.n >= len(T.target(label)[1])
    for what, got in w.d.items():
        assert got <= CPU_FACTOR * MEASURED_LT[label][what], (label, what, got, MEASURED_LT[label][what])


# ------------------------------------------------------------------------------------------------ a hit list against reference
def derived_check(h, d, ref, E):
    """The hit's score, the domain's bias and accuracy against the reference's, the bounds E of the three values carried
    through lt_window_hits' formula; 1e-6 relative for the float32 numbers the record holds (the score is formed in float32
    from terms of the magnitude of orig).  Returns the three distances."""
    a = d.alignment
    env_len, ali_len = ref.Ld, abs(a.target_to - a.target_from) + 1
    score, bias = LR.reported(ref.orig, ref.domcorrection, env_len, ali_len, T.WINDOW_LENGTH)
    e_score, e_bias, e_acc = abs(h.score - score), abs(d.bias - bias), abs(d.accuracy - ref.accuracy)
    assert e_bias <= E["corr"] / LR.LN2 + 1e-6 * abs(bias), (d.bias, bias, E)
    assert e_score <= (E["orig"] + E["corr"]) / LR.LN2 + 1e-6 * max(abs(score), abs(ref.orig) / LR.LN2), (h.score, score, E)
    assert d.score == h.score
    assert e_acc <= E["oasc"] / ref.Ld + 1e-6 * abs(ref.accuracy), (d.accuracy, ref.accuracy)
    return e_score, e_bias, e_acc


def hits_against_the_reference(label, hits, wins, factor, line=None):
    """Every hit of <hits> (one domain each) at its own envelope.  Returns (Worst, largest score / bias / accuracy distances)."""
    w = Worst()
    derived = np.zeros(3)
    found = []
    for h in hits:
        d = h.domains[0]
        lo, hi, rev = T.hit_envelope(d)
        windows_are_long(wins, lo, hi, rev)
        ref = T.reference(label, lo, hi, rev)
        got = w.add(ref, d._rec.envsc, d._rec.domcorrection, d._rec.oasc)
        E = bounds(label, ref, factor)
        if line is not None:
            line(f"{label} {lo}-{hi}{'-' if rev else '+'}: " + " ".join(f"{what} {got[what]:.2e} (bound {E[what]:.2e})" for what in got))
        for what, v in got.items():
            assert v <= E[what], (label, lo, hi, rev, what, v, E[what])
        derived = np.maximum(derived, derived_check(h, d, ref, E))
        if h.reported:
            found.append((lo, hi, rev))
    all_planted_found(label, found)
    return w, derived


@pytest.mark.parametrize("label", T.LABELS + (T.QUEUE_LABEL,))
def test_host_stage_envelopes_against_the_reference(libp7x, oracle, label, report):
    """The host workers (upstream's order of operations, the oracle's): the oracle's bound, CPU_FACTOR.  Score, bias and
    accuracy follow through lt_window_hits' formula."""
    _, wins, _ = oracle_case(oracle, label)
    hits = host_pipeline.host_nhmmer(oracle, T.model(label), T.block(label), pipeline=T.pipeline())
    w, derived = hits_against_the_reference(label, hits, wins, CPU_FACTOR)
    report(f"host stage {label}: {w.line()}; score {derived[0]:.2e} bias {derived[1]:.2e} bits, accuracy {derived[2]:.2e}")
    assert w.n >= len(T.target(label)[1])
