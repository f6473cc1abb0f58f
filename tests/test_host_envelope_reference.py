"""What a search reports for a domain envelope -- envsc (unihit Forward over the envelope), domcorrection (null2 by
expectation) and oasc (optimal accuracy) -- from the float32 implementations on the host, the oracle (oracle_lib.domains) and
the product's host stage (host_pipeline.host_search, in upstream's summation order and in the device's), against the float64
reference of tests/envelope_reference.py on the targets of tests/envelope_targets.py and on the fixture models' hits in the
fixture proteome.  Each envelope is taken at the coordinates the implementation itself reports.

The reference is pinned by itself first: null2 against the emitter usage of enumerated paths, sum_x f(x) null2[x] = 1 on
every envelope used, and the length argument of forward_backward.  The bounds are CPU_FACTOR times what these tests measured
(MEASURED_ENV, profiles/r15_envelope_reference.md); tests/test_gpu_envelope_reference.py derives the device's from them."""
import time

import numpy as np
import pytest

import dp_reference as R
import envelope_reference as ER
import envelope_targets as T
import host_pipeline
from conftest import load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, plan7

# Largest |oracle - reference| per label over its envelopes: envsc and corr (domcorrection) in nats, oasc in posterior units.
MEASURED_ENV = {
    "rnd5": dict(envsc=1.7e-07, corr=6.3e-07, oasc=2.8e-07),
    "rnd63": dict(envsc=3.8e-06, corr=2.3e-05, oasc=2.5e-05),
    "rnd64": dict(envsc=2.3e-06, corr=2.6e-05, oasc=2.3e-05),
    "rnd65": dict(envsc=6.3e-06, corr=2.7e-05, oasc=3.4e-05),
    "rnd128": dict(envsc=4.6e-06, corr=8.4e-05, oasc=7.8e-05),
    "rnd129": dict(envsc=1.3e-05, corr=1.0e-04, oasc=1.0e-04),
    "rnd192": dict(envsc=3.1e-05, corr=2.2e-04, oasc=2.5e-04),
    "rnd193": dict(envsc=2.4e-05, corr=2.7e-04, oasc=2.3e-04),
    "rnd256": dict(envsc=2.1e-05, corr=3.9e-04, oasc=2.9e-04),
    "rnd257": dict(envsc=5.0e-05, corr=3.9e-04, oasc=3.5e-04),
    "rnd320": dict(envsc=5.0e-05, corr=2.9e-04, oasc=3.8e-04),
    "rnd321": dict(envsc=3.3e-05, corr=1.3e-04, oasc=1.8e-04),
    "rnd384": dict(envsc=4.1e-05, corr=2.5e-04, oasc=3.5e-04),
    "rnd385": dict(envsc=2.3e-05, corr=3.7e-04, oasc=3.1e-04),
    "rnd512": dict(envsc=2.6e-05, corr=1.1e-04, oasc=5.9e-05),
    "rnd513": dict(envsc=4.4e-05, corr=2.9e-04, oasc=2.6e-04),
    "rnd640": dict(envsc=4.4e-05, corr=2.2e-04, oasc=2.1e-04),
    "rnd641": dict(envsc=6.8e-05, corr=3.0e-04, oasc=1.6e-04),
    "rnd768": dict(envsc=2.6e-05, corr=1.2e-04, oasc=1.8e-04),
    "rnd769": dict(envsc=3.2e-05, corr=4.2e-04, oasc=5.4e-04),
    "rnd1024": dict(envsc=5.3e-05, corr=3.1e-04, oasc=3.0e-04),
    "rnd1025": dict(envsc=4.9e-05, corr=4.4e-04, oasc=3.7e-04),
    "rnd1280": dict(envsc=3.0e-05, corr=2.4e-04, oasc=3.1e-04),
    "rnd1281": dict(envsc=6.2e-05, corr=4.2e-04, oasc=3.6e-04),
    "rnd1536": dict(envsc=4.3e-05, corr=1.5e-04, oasc=3.4e-04),
    "rnd1537": dict(envsc=2.6e-05, corr=1.7e-04, oasc=1.3e-04),
    "rnd2048": dict(envsc=4.8e-05, corr=4.0e-04, oasc=3.8e-04),
    "rnd2049": dict(envsc=7.0e-05, corr=1.1e-04, oasc=1.9e-04),
    "rnd3072": dict(envsc=2.3e-05, corr=1.4e-04, oasc=9.7e-05),
    "rnd3073": dict(envsc=5.0e-05, corr=2.9e-04, oasc=1.0e-04),
    "rnd4096": dict(envsc=3.0e-05, corr=3.0e-04, oasc=2.1e-04),
    "rnd4097": dict(envsc=1.3e-05, corr=1.2e-04, oasc=3.1e-04),
    "rnd6144": dict(envsc=4.0e-05, corr=2.2e-04, oasc=3.5e-04),
    "rnd6145": dict(envsc=5.8e-05, corr=3.3e-04, oasc=4.3e-04),
    "rnd8192": dict(envsc=2.8e-05, corr=2.0e-04, oasc=1.2e-04),
    "rnd8193": dict(envsc=6.5e-05, corr=2.9e-04, oasc=2.6e-04),
    "rnd12288": dict(envsc=5.5e-05, corr=2.5e-04, oasc=1.4e-04),
    "rnd300 edges": dict(envsc=5.6e-05, corr=7.5e-05, oasc=1.7e-04),
    "rnd1100 long": dict(envsc=1.6e-04, corr=2.2e-03, oasc=3.7e-04),
    # the queue labels (T.QUEUE_LABELS, profiles/r29_envelope_queue.md): 43-47 envelopes, 25-26 at M = 512 and 1025, 16-17 from 2049 on
    "rnd64 queue": dict(envsc=7.8e-06, corr=4.5e-05, oasc=4.8e-05),
    "rnd320 queue": dict(envsc=4.6e-05, corr=3.5e-04, oasc=3.5e-04),
    "rnd512 queue": dict(envsc=6.1e-05, corr=2.9e-04, oasc=1.7e-04),
    "rnd1025 queue": dict(envsc=5.4e-05, corr=3.8e-04, oasc=5.3e-04),
    "rnd2049 queue": dict(envsc=1.2e-05, corr=7.9e-05, oasc=6.2e-05),
    "rnd4097 queue": dict(envsc=7.4e-06, corr=1.1e-04, oasc=9.9e-05),
    "KR": dict(envsc=2.6e-06, corr=2.3e-04, oasc=3.3e-04),                 # 12 envelopes of 9 hits, 2 of them clustered
    "PF02826": dict(envsc=7.9e-06, corr=1.4e-04, oasc=1.0e-04),            # 38 envelopes of 22 hits, 8 of them clustered
    "Thioesterase": dict(envsc=2.3e-07, corr=2.7e-06, oasc=3.8e-06),       # its one hit
}
CPU_FACTOR = 2.0
DEVICE_FACTOR = 4.0               # another association of the same float32 terms: the device, and the host stage in its order
FIXTURES = ("KR", "PF02826", "Thioesterase")
MAX_FIXTURE_L = 1500
NULL2_SUM_TOL = 1e-5              # a few float32 roundings of the odds table
_T0 = []                          # when this module's first test began (the wall time in the report lines)


def floors(ref):
    """What float32 cannot do better, whatever the oracle measured: 1e-6 |envsc| for a score; Ld 2^-23 for domcorrection and
    oasc, each a float32 running sum of Ld addends of magnitude about 1, every addend rounded once."""
    return dict(envsc=1e-6 * abs(ref.envsc), corr=ref.Ld * 2.0 ** -23, oasc=ref.Ld * 2.0 ** -23)


def bounds(label, ref, factor):
    fl = floors(ref)
    return {what: max(factor * MEASURED_ENV[label][what], fl[what]) for what in ("envsc", "corr", "oasc")}


@pytest.fixture(autouse=True, scope="module")
def _clock():
    _T0.append(time.time())
    yield


@pytest.fixture
def report(capsys):
    def emit(line):
        with capsys.disabled():
            print(f"\n[envelope-reference] {line}  ({time.time() - _T0[0]:.0f} s)", end="", flush=True)
    return emit


@pytest.fixture
def device_order(libp7x):
    _lib.set_debug_option("host_order", 1)
    yield
    _lib.set_debug_option("host_order", -1)


def null2_sum(hmm, ref):
    f = plan7.Background(hmm.alphabet).residue_frequencies.astype(np.float64)
    return float(f @ ref.null2[:hmm.alphabet.K])


class Worst:
    """The largest distances of a set of envelopes from the reference, and the conditions on the set."""

    def __init__(self):
        self.d = dict(envsc=0.0, corr=0.0, oasc=0.0)
        self.n = self.full = 0
        self.null2 = 0.0

    def add(self, hmm, ref, envsc, corr, oasc, clustered):
        self.n += 1
        self.null2 = max(self.null2, abs(null2_sum(hmm, ref) - 1.0))
        got = dict(envsc=abs(envsc - ref.envsc), oasc=abs(oasc - ref.oasc))
        if not clustered:                          # a clustered envelope's correction is null2 by trace: not stated here
            got["corr"] = abs(corr - ref.domcorrection)
            self.full += 1
        for what, v in got.items():
            self.d[what] = max(self.d[what], v)
        return got

    def line(self):
        return (f"{self.n} envelopes ({self.full} in all three values): envsc {self.d['envsc']:.2e} corr {self.d['corr']:.2e} nats, "
                f"oasc {self.d['oasc']:.2e}; |sum f null2 - 1| <= {self.null2:.1e}")


# ------------------------------------------------------------------------------------------------ the reference by itself
def test_length_argument_is_the_default_at_the_targets_own_length(libp7x):
    hmm = random_hmm(40, seed=40)
    rm = R.RefModel.from_oprofile(plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400))
    seq = np.random.default_rng(3).integers(0, 20, 57)
    for multihit in (True, False):
        a = R.forward_backward(rm, seq, multihit, cells=True)
        b = R.forward_backward(rm, seq, multihit, cells=True, length=len(seq))
        assert (a.fwd, a.bck, a.loop, a.move) == (b.fwd, b.bck, b.loop, b.move)
        for name in ("fx", "bx", "fM", "fI", "bM", "bI"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        c = R.forward_backward(rm, seq, multihit, length=400)
        assert c.loop > a.loop and c.move < a.move and c.fwd != a.fwd
    hmm = random_hmm(2, seed=902)
    rm = R.RefModel.from_oprofile(plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400))
    for multihit in (True, False):
        assert R.enumerate_paths(rm, seq[:3], multihit) == R.enumerate_paths(rm, seq[:3], multihit, length=3)
        assert R.enumerate_paths(rm, seq[:3], multihit) != R.enumerate_paths(rm, seq[:3], multihit, length=30)


def test_null2_is_the_emitter_usage_of_the_enumerated_paths(libp7x, oracle, report):
    """Models of 1-3 nodes, targets of 1-5 residues, as envelopes of a target 0, 7 and 395 residues longer: occ[k] and rest
    from the walk over the state graph (every complete path's probability credited to the emitter of each residue) give the
    null2 of the posteriors, to 1e-12 -- and Forward under the longer target's length model is the paths' sum."""
    degen = oracle.degeneracy_sets(20)
    worst, n = 0.0, 0
    for M in (1, 2, 3):
        for seed in (0, 1):
            hmm = random_hmm(M, seed=900 + 10 * seed + M)
            rm = R.RefModel.from_oprofile(plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400))
            for Ld in range(1, 6):
                seq = np.random.default_rng([M, seed, Ld]).integers(0, 20, Ld)
                for extra in (0, 7, 395):
                    ref = R.forward_backward(rm, seq, False, cells=True, length=Ld + extra)
                    got = ER.null2_by_expectation(rm, ref, degen)
                    total, usage = R.enumerate_paths(rm, seq, False, length=Ld + extra, emitters=True)
                    assert abs(ref.fwd - total) <= 1e-12 * abs(total), (M, seed, Ld, extra)
                    occ, rest = np.zeros(M + 1), 0.0
                    for per_residue in usage:
                        assert abs(sum(per_residue.values()) / np.exp(total) - 1.0) <= 1e-12       # one emitter per residue
                        for (state, k), p in per_residue.items():
                            if state == "M":
                                occ[k] += p / np.exp(total) / Ld
                            else:
                                rest += p / np.exp(total) / Ld
                    want = np.ones(rm.Kp)
                    for x in range(20):
                        want[x] = sum(occ[k] * np.exp(rm.e[x, k]) for k in range(1, M + 1)) + rest
                    for x in range(20, rm.Kp):
                        if degen[x].any():
                            want[x] = np.mean([want[c] for c in range(20) if degen[x, c]])
                    err = float(np.abs(got / want - 1.0).max())
                    worst, n = max(worst, err), n + 1
                    assert err <= 1e-12, (M, seed, Ld, extra, got, want)
                    assert got[20] == got[27] == got[28] == 1.0                                # gap, '*', missing data
    report(f"self-check: null2 = emitter usage of the enumerated paths on {n} (model, envelope, target length) cases, worst relative {worst:.1e}")


def test_dombias_reach_covers_the_table_steps():
    """The bound on a reported bias: dombias moves by no more than dombias_reach when domcorrection moves by err."""
    rng = np.random.default_rng(1)
    for corr in np.concatenate([rng.uniform(-2.0, 12.0, 300), -ER.LOG_OMEGA + rng.uniform(-2e-3, 2e-3, 100)]):
        for err in (1e-6, 1e-4, 3e-3):
            reach = ER.dombias_reach(corr, err)
            moved = max(abs(ER.dombias(c) - ER.dombias(corr)) for c in np.linspace(corr - err, corr + err, 41))
            assert err <= reach <= err + 5.1e-4 * (2 + 2e3 * err) and moved <= reach + 1e-15, (corr, err, moved, reach)


# ------------------------------------------------------------------------------------------------ oracle against reference
def oracle_distances(oracle, key, hmm, named, planted=True):
    op = oracle.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400)
    w = Worst()
    for name, seq in named:
        envs, counts = oracle.domains(op, np.asarray(seq, dtype=np.uint8))
        if planted:
            assert len(envs) >= 1 and counts[2] == 0, (key, name, len(envs), counts, "not one region of single domains")
        for e in envs:
            ref = T.reference(key, hmm, name, seq, e[0], e[1])
            w.add(hmm, ref, e[6], e[7], e[8], clustered=e[12] != 0)
    return w


@pytest.mark.parametrize("label", T.LABELS + T.QUEUE_LABELS)
def test_oracle_envelopes_against_the_reference(libp7x, oracle, label, report):
    hmm = T.model(label)
    w = oracle_distances(oracle, label.split()[0], hmm, T.targets(label))
    report(f"oracle {label}: {w.line()}")
    assert w.null2 <= NULL2_SUM_TOL
    assert w.full >= len(T.targets(label))
    for what, got in w.d.items():
        assert got <= CPU_FACTOR * MEASURED_ENV[label][what], (label, what, got, MEASURED_ENV[label][what])


# ------------------------------------------------------------------------------------------------ host stage against reference
def derived_check(d, ref, E, clustered):
    """score, bias and accuracy of a domain against the reference's, the bounds E of the three kernel outputs carried through
    finish_one's formulas; 1e-6 relative for the float32 the record holds.  Returns the three distances."""
    e_acc = abs(d.accuracy - ref.accuracy)
    assert e_acc <= E["oasc"] / ref.Ld + 1e-6 * abs(ref.accuracy), (d.accuracy, ref.accuracy)
    if clustered:
        return None, None, e_acc
    reach = ER.dombias_reach(ref.domcorrection, E["corr"])
    e_bias, e_score = abs(d.bias - ref.dombias / ER.LN2), abs(d.score - ref.bitscore)
    assert e_bias <= reach / ER.LN2 + 1e-6 * abs(ref.dombias / ER.LN2), (d.bias, ref.dombias / ER.LN2, reach)
    assert e_score <= (E["envsc"] + reach) / ER.LN2 + 1e-6 * abs(ref.bitscore), (d.score, ref.bitscore, E, reach)
    return e_score, e_bias, e_acc


def host_distances(oracle, key, label, hmm, block, named, factor, planted=True):
    opts = T.pipeline_options(label)
    hits = host_pipeline.host_search(oracle, hmm, block, pipeline=plan7.Pipeline(hmm.alphabet, **opts),
                                     F=(opts.get("F1", 0.02), opts.get("F2", 1e-3), opts.get("F3", 1e-5)))
    by_name = {h.name: h for h in hits}
    w = Worst()
    for name, seq in named:
        if planted:
            assert name in by_name and by_name[name].nclustered == 0 and len(by_name[name].domains) >= 1, (label, name)
        h = by_name.get(name)
        for d in (h.domains if h is not None else ()):
            ref = T.reference(key, hmm, name, seq, d.env_from, d.env_to)
            clustered = h.nclustered > 0
            got = w.add(hmm, ref, d._rec.envsc, d._rec.domcorrection, d._rec.oasc, clustered)
            E = bounds(label, ref, factor)
            for what, v in got.items():
                assert v <= E[what], (label, name, what, v, E[what])
            derived_check(d, ref, E, clustered)
    return w


@pytest.mark.parametrize("label", T.LABELS + T.QUEUE_LABELS)
def test_host_stage_envelopes_against_the_reference(libp7x, oracle, label, report):
    """Upstream's order: the oracle's operations on the oracle's operands, so the oracle's bound (CPU_FACTOR).  score, bias and
    accuracy follow through finish_one's formulas."""
    hmm = T.model(label)
    named = T.targets(label)
    w = host_distances(oracle, label.split()[0], label, hmm, T.search_block(hmm, named), named, CPU_FACTOR)
    report(f"host stage {label}, upstream's order: {w.line()}")
    assert w.full >= len(named)


@pytest.mark.parametrize("label", T.LABELS + T.QUEUE_LABELS)
def test_host_stage_in_the_device_order_against_the_reference(libp7x, oracle, device_order, label, report):
    """host_order = 1, the lane-chunk association of the kernels: the device's bound (DEVICE_FACTOR, with the floors)."""
    hmm = T.model(label)
    named = T.targets(label)
    w = host_distances(oracle, label.split()[0], label, hmm, T.search_block(hmm, named), named, DEVICE_FACTOR)
    report(f"host stage {label}, device's order: {w.line()}")
    assert w.full >= len(named)


# ------------------------------------------------------------------------------------------------ fixture models
def fixture_hits(hits, proteome):
    """[(name, residues)] of the hits whose target is at most MAX_FIXTURE_L residues."""
    by_name = {s.name: s for s in proteome}
    return [(h.name, np.asarray(by_name[h.name].sequence, dtype=np.uint8)) for h in hits if len(by_name[h.name]) <= MAX_FIXTURE_L]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_envelopes_against_the_reference(libp7x, oracle, proteome, name, report):
    """Every domain of every hit of the default pipeline on the fixture proteome (targets of at most 1,500 residues): the
    oracle, then the host stage in both orders."""
    hmm = load_hmms(name)[0]
    named = fixture_hits(host_pipeline.host_search(oracle, hmm, proteome), proteome)
    assert len(named) >= 1
    w = oracle_distances(oracle, name, hmm, named, planted=False)
    report(f"oracle {name} x {len(named)} proteome hits: {w.line()}")
    assert w.null2 <= NULL2_SUM_TOL and w.full >= 1
    for what, got in w.d.items():
        assert got <= CPU_FACTOR * MEASURED_ENV[name][what], (name, what, got, MEASURED_ENV[name][what])
    for order, factor in ((-1, CPU_FACTOR), (1, DEVICE_FACTOR)):
        _lib.set_debug_option("host_order", order)
        try:
            wh = host_distances(oracle, name, name, hmm, proteome, named, factor, planted=False)
        finally:
            _lib.set_debug_option("host_order", -1)
        report(f"host stage {name}, {'device' if order == 1 else 'upstream'}'s order: {wh.line()}")
        assert wh.n >= w.full


# ------------------------------------------------------------------------------------------------ the queue labels' inputs
@pytest.mark.parametrize("label", T.QUEUE_LABELS)
def test_queue_targets_are_what_the_queue_tests_need(libp7x, oracle, label):
    """The block lists the fragments shortest first (the queue hands them out longest first: a real permutation), a window
    ends at node M and one lies across nodes 32 C and 32 C + 1, every target is a hit of single-domain regions, and the last
    target gives one envelope per planted fragment at least -- several envelopes of one item."""
    hmm = T.model(label)
    M = hmm.M
    wins = T.queue_windows(M)
    assert len(wins) == T.QUEUE_TARGETS[M]
    nodes = [last - first + 1 for _, first, last in wins]
    assert nodes == sorted(nodes) and nodes[0] == T.QUEUE_MIN_NODES and nodes[-1] == (min(M, T.FRAGMENT_NODES) if M <= 1025 else 120)
    mid = 32 * T.tier_of(M)
    assert any(last == M for _, _, last in wins) and any(first <= mid < last for _, first, last in wins)
    assert all(1 <= first <= last <= M for _, first, last in wins)
    named = T.targets(label)
    assert len(named) == len(wins) + 1 and len({n for n, _ in named}) == len(named)
    opts = T.pipeline_options(label)
    hits = host_pipeline.host_search(oracle, hmm, T.search_block(hmm, named), pipeline=plan7.Pipeline(hmm.alphabet, **opts),
                                     F=(opts.get("F1", 0.02), opts.get("F2", 1e-3), opts.get("F3", 1e-5)))
    by_name = {h.name: h for h in hits}
    for name, _ in named:
        assert name in by_name and by_name[name].nclustered == 0 and len(by_name[name].domains) >= 1, (label, name)
    assert len(by_name[named[-1][0]].domains) >= T.QUEUE_MULTI
    nenv = sum(len(by_name[name].domains) for name, _ in named)
    assert nenv >= 2 * (8 if M <= 448 else 4)                   # twice env_waves(C) of p7x_envkernel.hpp, at the least
