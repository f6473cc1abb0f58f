"""The stochastic-traceback ensembles of the host twin (p7x_domaindef.cpp: stochastic_trace, null2_by_trace, the choice
records of p7x_choice.hpp) against the float64 reference of tests/ensemble_reference.py, on the cases of
tests/ensemble_cases.py.  No GPU: tests/test_gpu_ensemble_reference.py holds the kernels to the same reference and to the
twin in their own summation order.

Two bounds, no others.  d_ref is what the upstream-order twin -- the oracle's bits -- is away from float64, measured here
over every choice point whose cell has a float64 posterior of at least 1e-9 (a condition: a walk meets a rarer cell less
than once in 5e6 sampled regions, and below it the scaled float32 matrix may hold denormals).  The device order is held
to max(4 d_ref, 2^-21) on the same cells: the project's factor of four, and its measured spread between the two float32
orders.  Measured figures: profiles/r26_ensemble_reference.md."""
import numpy as np
import pytest

import dp_reference as R
import ensemble_cases as EC
import ensemble_reference as ER
from conftest import random_hmm
from pyhmmer_amd import easel, plan7

NEAR_CAP = 0.01                 # at most this share of a case's samples may hold a step float64 would not have taken


@pytest.fixture
def report(capsys):
    def emit(line):
        with capsys.disabled():
            print("\n[ensemble-reference] " + line, end="", flush=True)
    return emit


# ------------------------------------------------------------------------------------------------ the reference pins itself
def _tiny(M, seed, seq):
    hmm = random_hmm(M, seed=seed)
    om = plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400)
    model = R.RefModel.from_oprofile(om)
    seq = np.asarray(seq, dtype=np.uint8)
    return om, model, seq, ER.RegionReference(model, om.rfv.shape[1] // 4, seq, 1, len(seq))


TINY = [(3, 5, (3, 7, 1, 12)), (2, 9, (0, 19, 4, 4, 11)), (4, 21, (8, 2, 15))]


def test_the_stream_is_the_fast_generator(libp7x):
    for seed in (1, 42, 123456789):
        rng = easel.Randomness(seed, fast=True)
        want = [int(rng.random() * ER.TWO32) for _ in range(70)]
        assert ER.lcg_stream(EC.seed_state(seed), 70).tolist() == want


@pytest.mark.parametrize("M,seed,seq", TINY)
def test_choice_probabilities_reproduce_every_enumerated_path(libp7x, M, seed, seq):
    """The product of the choice probabilities along a path is the path's posterior: the backward walk samples paths with
    exactly their probability under the model.  Every choice point sums to one (the E state's list is the only one that is
    not closed by construction)."""
    om, model, seq, reg = _tiny(M, seed, seq)
    paths = ER.enumerate_full_paths(model, seq)
    total = sum(p for _, p in paths)
    assert abs(np.log(total) - R.enumerate_paths(model, seq, True)) < 1e-12 and abs(np.log(total) - reg.ref.fwd) < 1e-12
    assert len(paths) > 100
    for path, p in paths:
        assert abs(reg.path_probability(path) - p / total) < 1e-12, path
    for row in range(1, reg.Lr + 1):
        assert abs(reg.e_cum(row)[-1] - 1.0) < 1e-12
    for q in (reg.qM[1:, 1:M + 1], reg.qI[1:, 1:M + 1], reg.qD[1:, 2:M + 1], reg.qC[1:], reg.qJ[1:], reg.qB):
        q = q[~np.isnan(q)]
        assert ((q >= 0.0) & (q <= 1.0 + 1e-15)).all()
    assert (np.diff(reg.qM[1:, 1:M + 1], axis=-1)[~np.isnan(reg.qM[1:, 1:M + 1, 0])] >= 0.0).all()


@pytest.mark.parametrize("M,seed,seq", TINY)
def test_marginals_equal_the_enumerated_usage(libp7x, M, seed, seq):
    om, model, seq, reg = _tiny(M, seed, seq)
    paths = ER.enumerate_full_paths(model, seq)
    total = sum(p for _, p in paths)
    marg = reg.marginals()
    want = {f: np.zeros(marg[f].shape) for f in marg}
    for path, p in paths:
        w = p / total
        bs = [z for z, (s, _, _) in enumerate(path) if s == ER.sB]
        es = [z for z, (s, _, _) in enumerate(path) if s == ER.sE]
        for s, k, row in path:
            if s in (ER.sM, ER.sI):
                want["M" if s == ER.sM else "I"][row, k] += w
                want["inside"][row] += w
            elif s == ER.sD:
                want["D"][row, k] += w
        for zb, ze in zip(bs, es):
            dm = [(k, row) for s, k, row in path[zb:ze] if s == ER.sM]
            want["start"][dm[0][1]] += w
            want["end"][dm[-1][1]] += w
        want["first"][path[bs[0] + 1][1]] += w
        want["last"][[k for s, k, _ in path[bs[-1]:es[-1]] if s == ER.sM][-1]] += w
    _, usage = R.enumerate_paths(model, seq, True, emitters=True)
    for r, u in enumerate(usage, start=1):                  # dp_reference's own enumeration says the same
        for (state, k), p in u.items():
            if state in ("M", "I"):
                assert abs(marg[state][r, k] - p / total) < 1e-12
    for f in marg:
        assert np.abs(marg[f] - want[f]).max() < 1e-12, f
    assert abs(marg["first"].sum() - 1.0) < 1e-12 and abs(marg["last"].sum() - 1.0) < 1e-12


def test_null2_by_trace_by_hand(libp7x, oracle):
    """One domain M1 I1 M2 M3 over four residues, the third a degenerate code: the insert's count lands in node 1's match
    slot, the domain's first residue counts as outside, the degenerate code takes the mean of its residues."""
    om, model, _, _ = _tiny(3, 5, (3, 7, 1, 12))
    degen = np.asarray(oracle.degeneracy_sets(20))
    x = next(c for c in range(20, degen.shape[0]) if degen[c].sum() == 2)
    a, b = np.nonzero(degen[x])[0]
    seq = np.array([5, 3, 7, x, 12, 9], dtype=np.uint8)            # residue 1 in N, 2..5 the domain, 6 in C
    reg = ER.RegionReference(model, om.rfv.shape[1] // 4, seq, 1, len(seq))
    S, N, B, M, I, E, C, T = ER.sS, ER.sN, ER.sB, ER.sM, ER.sI, ER.sE, ER.sC, ER.sT
    st = np.array([S, N, N, B, M, I, M, M, E, C, C, T])
    k = np.array([0, 0, 0, 0, 1, 1, 2, 3, 0, 0, 0, 0])
    i = np.array([0, 0, 1, 0, 2, 3, 4, 5, 0, 0, 6, 0])
    odds = lambda res: (2.0 * np.exp(model.e[res, 1]) + np.exp(model.e[res, 2]) + np.exp(model.e[res, 3])) / 4.0
    want = [1.0, 1.0, odds(7), 0.5 * (odds(a) + odds(b)), odds(12), 1.0]
    got = reg.null2_sums(st, k, i, np.array([0, len(st)]), degen)
    assert np.abs(got[1:] - want).max() < 1e-15


# ------------------------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("name", EC.NAMES)
def test_thresholds_of_every_cell(libp7x, name, report):
    """Every cell and row of the region, visited or not: the first node of a lane, the rows after a rescale, the C / J
    records.  The device-order twin within max(4 d_ref, 2^-21) of float64 wherever the posterior is at least 1e-9."""
    reg = EC.reference(name)
    d_ref, bound = EC.d_ref(name), EC.threshold_bound(name)
    dev = reg.threshold_distance(*EC.twin_records(name, EC.DEVICE))
    decades = lambda d: " ".join(f"{v:.2e}" for v in d.values())
    report(f"{name}: M {reg.M} Lr {reg.Lr} d_ref {d_ref:.3e} device order {dev[ER.FLOOR]:.3e} bound {bound:.3e}; by posterior floor "
           f"{ER.DECADES}: upstream {decades(EC._dref[name])}, device order {decades(dev)}")
    assert dev[ER.FLOOR] <= bound


# ------------------------------------------------------------------------------------------------ walks
def _walks(name, order):
    reg, bound = EC.reference(name), EC.threshold_bound(name)
    near, worst = 0, 0.0
    for seed in EC.EXACT_SEEDS:
        st, k, i, off, dom, n2 = EC.twin_traces(name, seed, order)
        w = reg.walk_check(st, k, i, off, EC.seed_state(seed))
        bad = ~w.ok
        assert not np.isnan(w.dist).any(), "a walk passed through a cell no float64 path reaches"
        assert (w.dist[bad] <= bound).all(), (name, order, seed, float(w.dist.max()), bound)
        near += len(np.unique(w.sample[bad]))
        worst = max(worst, float(w.dist.max()))
    return near, worst, ER.NSAMPLES * len(EC.EXACT_SEEDS)


@pytest.mark.parametrize("name", EC.NAMES)
def test_every_step_is_the_float64_pick_or_within_the_bound_of_it(libp7x, name, report):
    """Every deviate of every walk of the twin, both orders, four seeds: the step taken is the one float64 takes, or the
    deviate lies within the case's threshold bound of the boundary it crossed.  At most 1 % of the samples hold such a
    step (expected from the band: 300 steps x 3 thresholds x 2 x 2^-19, 0.3 %) -- the upstream order first."""
    near_u, worst_u, n = _walks(name, EC.UPSTREAM)
    assert near_u <= NEAR_CAP * n, (name, near_u, n)
    near_d, worst_d, n = _walks(name, EC.DEVICE)
    report(f"{name}: samples with a near-threshold step {near_u}/{n} upstream (farthest {worst_u:.2e}), {near_d}/{n} device order ({worst_d:.2e})")
    assert near_d <= NEAR_CAP * n, (name, near_d, n)


# ------------------------------------------------------------------------------------------------ distribution
@pytest.mark.parametrize("name", EC.NAMES)
def test_distribution(libp7x, name, report):
    """25 seeds x 200 samples of the twin: the count of every indicator -- residue r emitted by M_k, by I_k, D_k on row r, r
    inside a domain, a domain starting / ending at r, the first domain's entry node, the last domain's last match node --
    lies within 6 sqrt(S p (1 - p)) + 1 of S p, p the float64 marginal (the rule of test_host_emit.py::test_distribution).
    Cells with S p < 1 are pooled per family (ensemble_reference.Tally).  Over the 32 cases 43,151 cells are tested;
    a binomial count at S p >= 1 passes six sigma plus one with probability above 1 - 2e-6 (the Poisson tail at mean 1, the
    worst case), so under 0.09 false alarms are expected in all -- and the seeds are fixed."""
    reg, c = EC.reference(name), EC.case(name)
    tally = ER.Tally(reg.marginals(), ER.NSAMPLES * len(EC.DIST_SEEDS), ER.TRACE_FAMILIES + ER.DOM_FAMILIES)
    for seed in EC.DIST_SEEDS:
        st, k, i, off, dom, n2 = EC.twin_traces(name, seed, EC.UPSTREAM, keep=False)
        rows, t_of = reg.rows_of(st, i, off)
        tally.add_domains(dom)
        tally.add_traces(st, k, rows, t_of)
    bad, cells = tally.violations()
    report(f"{name}: {cells} cells, {len(bad)} outside six sigma")
    assert not bad, bad[:10]
    assert cells >= 10


# ------------------------------------------------------------------------------------------------ null2 by trace
@pytest.mark.parametrize("name", EC.NAMES)
def test_null2_sums_against_float64_over_the_same_paths(libp7x, oracle, name, report):
    """n2[pos] of the twin against null2 by trace in float64 summed over the twin's own 200 paths.  The upstream order's
    distance is the measurement; the device order is held to four times it, or to 200 x 2^-23 x n2 where that is more."""
    d_up = EC.null2_ref_distance(name)
    worst, top = 0.0, 0.0
    for seed in EC.EXACT_SEEDS:
        got, want = EC.twin_traces(name, seed, EC.DEVICE)[5], EC.null2_reference(name, seed, EC.DEVICE)
        d = np.abs(got[1:] - want[1:])
        worst, top = max(worst, float(d.max())), max(top, float(want.max()))
        assert (d <= EC.null2_bound(name, want)[1:]).all(), (name, seed, float(d.max()))
    report(f"{name}: null2 sums (largest {top:.1f}) upstream {d_up:.3e}, device order {worst:.3e}")
