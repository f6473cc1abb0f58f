"""The float32 Forward / Backward / decoding engines on the host -- the oracle (upstream's striped order) and the product's host
twin of hmmalign -- against the float64 log-space reference of tests/dp_reference.py, on the targets of
tests/tandem_targets.py: where Backward leaves Forward's scale factors behind (family a), where posterior decoding
overflows (family b), ragged lengths (family c), and a sample of the fixture proteome.

The reference is pinned by itself first (the sum over enumerated paths, Forward = Backward, posterior rows sum to 1).  The
bounds below are twice what these tests measured (profiles/r13_dp_reference.md; the engines are deterministic, the factor
leaves room for another libm); tests/test_gpu_dp_reference.py derives the device's bounds from them."""
import time

import numpy as np
import pytest

import dp_reference as R
import host_pipeline
import tandem_targets as T
from conftest import load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, plan7

# What these tests measured, per model on its own targets (families a, b, c) and per fixture model on the protein sample:
#   fwd, bck  nats, |oracle's score - reference| over multihit and unihit Forward / Backward
#   row       |oracle - reference| / max(|reference|, 1) of the log of a special-state cell (E N J B C, both directions)
#   pp        |host twin posterior - reference posterior| of the same cell, over every step of every trace
#   nexp      |nexpected - btot[L]| / max(btot[L], 1), the host stage on the oracle's rows
# The CPU bound of a figure is CPU_FACTOR times it; the device's bounds are in tests/test_gpu_dp_reference.py.
MEASURED = {
    "rnd40": dict(fwd=1.8e-5, bck=1.5e-5, row=6.4e-7, pp=1.1e-6, nexp=4.1e-7),
    "rnd45": dict(fwd=1.6e-5, bck=1.6e-5, row=3.1e-7, nexp=3.4e-7),                    # family b only
    "rnd100": dict(fwd=7.7e-5, bck=4.6e-5, row=4.8e-7, pp=1.1e-6, nexp=7.8e-7),
    "rnd300": dict(fwd=2.0e-4, bck=2.4e-4, row=8.3e-7, pp=1.2e-6, nexp=6.9e-6),
    "rnd1100": dict(fwd=1.1e-4, bck=1.1e-4, row=2.7e-6, pp=8.7e-7, nexp=2.3e-6),
    "rnd4200": dict(fwd=1.4e-4, bck=7.3e-5, row=4.8e-6, pp=9.8e-7, nexp=9.3e-7),
    "KR": dict(fwd=8.2e-5, bck=4.6e-5, row=8.2e-7, pp=1.1e-6, nexp=3.5e-6),
    "KR proteins": dict(fwd=1.1e-6, bck=1.9e-6, row=9.3e-7, pp=1.6e-6),
    "PF02826 proteins": dict(fwd=1.6e-6, bck=1.4e-6, row=1.1e-6, pp=2.2e-6),
    "Thioesterase proteins": dict(fwd=1.5e-6, bck=1.8e-6, row=9.3e-7, pp=1.7e-6),
    "KR 100 kb": dict(nexp=7.5e-6),
    "low complexity": dict(nexp=2.7e-5),
}
CPU_FACTOR = 2.0


def within(label, **figures):
    """Every measured figure within CPU_FACTOR times the recorded one."""
    for what, got in figures.items():
        assert got <= CPU_FACTOR * MEASURED[label][what], (label, what, got, MEASURED[label][what])


FIXTURES = ("KR", "PF02826", "Thioesterase")
SAMPLE = 30


@pytest.fixture
def report(capsys):
    """One line on the terminal whatever the capture mode: the measured figures belong to the run's output."""
    def emit(line):
        with capsys.disabled():
            print("\n[dp-reference] " + line, end="", flush=True)
    return emit


@pytest.fixture
def host_align(libp7x):
    _lib.set_debug_option("host_align", 1)
    yield
    _lib.set_debug_option("host_align", -1)


def _oracle_profile(oracle, key):
    hmm = T.model(key)
    return oracle.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400)


def sample_of(proteome, n=SAMPLE, max_len=T.MAX_L):
    """The first <n> proteins of every 40th of the fixture proteome that are no longer than the tandem targets."""
    picked = [s for s in proteome[::40] if 0 < len(s) <= max_len][:n]
    assert len(picked) == n
    return picked


def _fixture_model(name):
    return load_hmms(name)[0]


# ------------------------------------------------------------------------------------------------ the reference by itself
def test_tables_of_the_product_and_of_the_oracle_are_the_same(libp7x, oracle):
    """The reference reads the kernels' own float32 tables: the product's striped odds are the oracle's, float by float."""
    for key in T.MODEL_KEYS + ("rnd45",) + FIXTURES[1:]:
        hmm = T.model(key) if key in T.MODEL_KEYS + ("rnd45",) else _fixture_model(key)
        bg = plan7.Background(hmm.alphabet)
        om, op = plan7.OptimizedProfile(hmm, bg, 400), oracle.OracleProfile(hmm, bg, 400)
        assert np.array_equal(om.rfv.view(np.uint32), op.arr("rfv").view(np.uint32)), key
        assert np.array_equal(om.tfv.view(np.uint32), op.arr("tfv").view(np.uint32)), key
        a, b = R.RefModel.from_oprofile(om), R.RefModel.from_oracle(op)
        assert np.array_equal(a.tables(), b.tables()), key


def test_reference_forward_is_the_sum_over_all_paths(libp7x, report):
    """Every model of 1-3 nodes against every target of 1-5 residues of a sweep, both modes: Forward equals the sum of the
    probabilities of all enumerated paths (written as a walk over the state graph, not as the recursion) to 1e-12."""
    worst, n = 0.0, 0
    for M in (1, 2, 3):
        for seed in (0, 1):
            hmm = random_hmm(M, seed=900 + 10 * seed + M)
            rm = R.RefModel.from_oprofile(plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400))
            for L in range(1, 6):
                for rep in range(2):
                    seq = np.random.default_rng([M, seed, L, rep]).integers(0, 20, L)
                    for multihit in (True, False):
                        got = R.forward_backward(rm, seq, multihit).fwd
                        want = R.enumerate_paths(rm, seq, multihit)
                        rel = abs(got - want) / max(abs(want), 1e-300)
                        worst, n = max(worst, rel), n + 1
                        assert rel <= 1e-12, (M, seed, L, multihit, got, want)
    report(f"self-check: Forward = sum over enumerated paths on {n} (model, target, mode) cases, worst relative {worst:.1e}")


@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_reference_forward_is_backward_and_posteriors_sum_to_one(libp7x, key, report):
    worst_fb = worst_row = 0.0
    for name, seq in T.targets(key, "a") + T.targets(key, "c"):
        for multihit in (True, False):
            r = T.reference(key, name, seq, multihit, cells=True)
            worst_fb = max(worst_fb, abs(r.fwd - r.bck) / abs(r.fwd))
            ppM, ppI, pN, pJ, pC = r.posteriors()
            total = ppM.sum(axis=1) + ppI.sum(axis=1) + pN + pJ + pC
            worst_row = max(worst_row, float(np.abs(total[1:] - 1.0).max()))
    report(f"self-check {key}: |Forward - Backward| / |Forward| <= {worst_fb:.1e}, |sum of a row's posteriors - 1| <= {worst_row:.1e}")
    assert worst_fb <= 1e-10 and worst_row <= 1e-9


# ------------------------------------------------------------------------------------------------ the targets' conditions
@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_family_a_fragments_score_inside_the_window(libp7x, key, report):
    """[45, 80] nats: ln 1e16 + 8 and ln FLT_MAX - 8, so no summation order decides which branch a fragment takes."""
    sc = [R.forward_backward(T.ref_model(key), f, False).fwd for f in T.fragments(key)]
    report(f"family a {key}: {T.FRAGMENT_NODES[key]} nodes per fragment, unihit scores alone " + " ".join(f"{s:.1f}" for s in sc))
    assert all(45.0 <= s <= 80.0 for s in sc), sc


@pytest.mark.parametrize("key", T.OVERFLOW_KEYS)
def test_family_b_pieces_score_100_nats(libp7x, key, report):
    for copies in (2, 3):
        piece = T.overflow_piece(key, copies)
        sc = R.forward_backward(T.ref_model(key), piece, False).fwd
        report(f"family b {key}: {copies} copies of {len(piece)} nodes, unihit score of one alone {sc:.1f}")
        assert sc >= 100.0
    assert all(len(s) <= T.MAX_L for _, s in T.family_b(key))


# ------------------------------------------------------------------------------------------------ oracle against reference
def _oracle_multihit(op, seq, ref):
    st, fsc = op.fwd(seq)
    st2, bsc, fx, bx = op.bck(seq)
    assert st == 0 and st2 == 0
    own = bool((fx[:, 5] != bx[:, 5]).any())
    return abs(fsc - ref.fwd), abs(bsc - ref.bck), R.row_error(fx, bx, ref), own


def _oracle_unihit(oracle, op, seq, ref):
    status, fx, bx = oracle.dd_unihit_rows(op, seq)
    fsc, bsc = R.rows_scores(fx, bx, ref.move)
    own = bool((fx[:, 5] != bx[:, 5]).any())
    return abs(fsc - ref.fwd), abs(bsc - ref.bck), R.row_error(fx, bx, ref), own, status


@pytest.mark.parametrize("key", T.MODEL_KEYS + ("rnd45",))
def test_oracle_against_the_reference_on_the_tandem_targets(libp7x, oracle, key, report):
    """Multihit Forward, Backward and rows on families a, b, c; unihit (the export p7o_dd_unihit_rows) on a and c.  The
    families' conditions are stated from the oracle alone: every family-a target takes Backward's own scales in unihit mode
    and decodes; every family-b target overflows."""
    op = _oracle_profile(oracle, key)
    e = np.zeros(3)
    multi_own = 0
    families = ("ac" if key in T.FRAGMENT_NODES else "") + ("b" if key in T.OVERFLOW_KEYS else "")
    for fam in families:
        for name, seq in T.targets(key, fam):
            r = _oracle_multihit(op, seq, T.reference(key, name, seq, True))
            e = np.maximum(e, r[:3])
            multi_own += r[3]
    uni_own = {"a": 0, "c": 0}
    for fam in families.replace("b", ""):
        for name, seq in T.targets(key, fam):
            r = _oracle_unihit(oracle, op, seq, T.reference(key, name, seq, False, cells=True))
            e = np.maximum(e, r[:3])
            uni_own[fam] += r[3]
            assert r[4] == 0, (name, "decoding overflowed")
            if fam == "a":
                assert r[3], (name, "Backward stayed on Forward's scale factors")
    nb = 0
    if key in T.OVERFLOW_KEYS:
        for name, seq in T.targets(key, "b"):
            status, fx, bx = oracle.dd_unihit_rows(op, seq)
            assert status == 1 and (fx[:, 5] != bx[:, 5]).any(), (name, status)
            nb += 1
    na, nc = (len(T.targets(key, f)) if f in families else 0 for f in "ac")
    report(f"oracle {key}: E_fwd {e[0]:.3e} E_bck {e[1]:.3e} nats, E_row {e[2]:.3e}; unihit own scales on {uni_own['a']} of "
           f"{na} family-a and {uni_own['c']} of {nc} family-c targets, "
           f"{nb} family-b targets overflowed (all); multihit Backward left Forward's scales on {multi_own} targets")
    assert uni_own["a"] > 0 or "a" not in families
    within(key, fwd=e[0], bck=e[1], row=e[2])


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_against_the_reference_on_fixture_proteins(libp7x, oracle, proteome, name, report):
    hmm = _fixture_model(name)
    op = oracle.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400)
    rm = R.RefModel.from_oracle(op)
    e = np.zeros(3)
    own = 0
    for s in sample_of(proteome):
        seq = np.asarray(s.sequence, dtype=np.uint8)
        e = np.maximum(e, _oracle_multihit(op, seq, R.forward_backward(rm, seq, True))[:3])
        r = _oracle_unihit(oracle, op, seq, R.forward_backward(rm, seq, False))
        e = np.maximum(e, r[:3])
        own += r[3]
        assert r[4] == 0
    report(f"oracle {name} x {SAMPLE} proteins: E_fwd {e[0]:.3e} E_bck {e[1]:.3e} nats, E_row {e[2]:.3e}; unihit own scales on {own}")
    within(f"{name} proteins", fwd=e[0], bck=e[1], row=e[2])


# ------------------------------------------------------------------------------------------------ host twin against reference
def _posterior_error(trace, ref):
    got = np.asarray(trace.posterior_probabilities, dtype=np.float64)
    return float(np.abs(got - R.trace_posteriors(ref, trace)).max())


PP_GUARD = lambda M: 1.0e-5 + 2.5e-9 * M           # align_pp_guard (p7x_kernels.hpp)


def _near_a_digit_boundary(trace, M):
    """A posterior within the device's guard of a printed digit's boundary: the device hands such a sequence to the host twin."""
    pp = np.asarray(trace.posterior_probabilities, dtype=np.float64)
    v = (pp[np.isin(trace.st, (1, 3, 5, 8, 10)) & (trace.i > 0)] + 0.05) * 10.0
    return bool((np.abs(v - np.rint(v)) < 10.0 * PP_GUARD(M)).any())


@pytest.mark.parametrize("key", T.MODEL_KEYS)
def test_host_twin_posteriors_on_the_tandem_targets(libp7x, oracle, host_align, key, report):
    """Every posterior of every trace step against the reference's posterior of the same cell, families a and c; the
    sequences on which Backward takes its own scales (scaleproduct *= fS / bS row after row) are reported by themselves."""
    hmm = T.model(key)
    op = _oracle_profile(oracle, key)
    named = T.targets(key, "a") + T.targets(key, "c")
    traces = plan7.TraceAligner().compute_traces(hmm, T.block(hmm.alphabet, named))
    e_own = e_other = 0.0
    n_own = near = 0
    for (name, seq), tr in zip(named, traces):
        status, fx, bx = oracle.dd_unihit_rows(op, seq)
        err = _posterior_error(tr, T.reference(key, name, seq, False, cells=True))
        if (fx[:, 5] != bx[:, 5]).any():
            e_own, n_own = max(e_own, err), n_own + 1
        else:
            e_other = max(e_other, err)
        near += _near_a_digit_boundary(tr, hmm.M)
    report(f"host twin {key}: E_pp {e_own:.3e} on {n_own} sequences with own scales, {e_other:.3e} on the other {len(named) - n_own}; "
           f"{near} of {len(named)} have a posterior inside the device's digit-boundary guard")
    assert n_own >= len(T.targets(key, "a"))
    within(key, pp=max(e_own, e_other))
    assert 2 * near <= len(named)          # the device test's cap on flagged sequences can be met


@pytest.mark.parametrize("name", FIXTURES)
def test_host_twin_posteriors_on_fixture_proteins(libp7x, oracle, host_align, proteome, name, report):
    hmm = _fixture_model(name)
    op = oracle.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400)
    rm = R.RefModel.from_oracle(op)
    seqs = sample_of(proteome)
    traces = plan7.TraceAligner().compute_traces(hmm, easel.DigitalSequenceBlock(hmm.alphabet, seqs))
    e_own = e_other = 0.0
    n_own = 0
    for s, tr in zip(seqs, traces):
        seq = np.asarray(s.sequence, dtype=np.uint8)
        status, fx, bx = oracle.dd_unihit_rows(op, seq)
        err = _posterior_error(tr, R.forward_backward(rm, seq, False, cells=True))
        if (fx[:, 5] != bx[:, 5]).any():
            e_own, n_own = max(e_own, err), n_own + 1
        else:
            e_other = max(e_other, err)
    report(f"host twin {name} x {SAMPLE} proteins: E_pp {e_own:.3e} on {n_own} with own scales, {e_other:.3e} on the others")
    within(f"{name} proteins", pp=max(e_own, e_other))


@pytest.mark.parametrize("key", T.OVERFLOW_KEYS)
def test_host_twin_refuses_what_overflows_and_names_it(libp7x, host_align, key):
    """hmmalign on family b: OverflowError that names the overflowing sequence, also between two sequences that align; the
    block without it aligns."""
    hmm = T.model(key)
    fine = T.targets("rnd40", "a") if key == "rnd45" else T.targets(key, "a")
    aligner = plan7.TraceAligner()
    for name, seq in T.targets(key, "b"):
        named = [fine[0], (name, seq), fine[1]]
        with pytest.raises(OverflowError) as err:
            aligner.compute_traces(hmm, T.block(hmm.alphabet, named))
        assert repr(name) in str(err.value) and f"L = {len(seq)}" in str(err.value), str(err.value)
        assert fine[0][0] not in str(err.value) and fine[1][0] not in str(err.value)
    traces = aligner.compute_traces(hmm, T.block(hmm.alphabet, fine))
    assert len(traces) == 2 and all(len(t.st) for t in traces)
    # two that overflow, the shorter one first: the one named is the first of the input
    both = [T.targets(key, "b")[i] for i in np.argsort([len(s) for _, s in T.targets(key, "b")], kind="stable")]
    with pytest.raises(OverflowError) as err:
        aligner.compute_traces(hmm, T.block(hmm.alphabet, [fine[0]] + both))
    assert repr(both[0][0]) in str(err.value), str(err.value)


# ------------------------------------------------------------------------------------------------ the multihit parser
def region_scan(btot, etot, mocc, rt1=0.25, rt2=0.10):
    """p7_domaindef_ByPosteriorHeuristics' scan for regions over the domain-decoding sums (here: the reference's)."""
    regions, i, triggered = [], -1, False
    for j in range(1, len(btot)):
        if not triggered:
            if mocc[j] - (btot[j] - btot[j - 1]) < rt2:
                i = j
            elif i == -1:
                i = j
            if mocc[j] >= rt1:
                triggered = True
        elif mocc[j] - (etot[j] - etot[j - 1]) < rt2:
            regions.append((i, j))
            i, triggered = -1, False
    return regions


def low_complexity_model(M=60):
    """random_hmm(60) with two residues' match emissions raised: A to 0.9 at the even nodes, A and S to 0.45 each at the odd
    nodes, so that a homopolymer of A and the dipeptide repeat SA both match it along their whole length."""
    hmm = random_hmm(M, seed=M)
    abc = hmm.alphabet
    mat = np.array(hmm.match_emissions, dtype=np.float64)
    cons = []
    for k in range(1, M + 1):
        a, s = abc.symbols.index("A"), abc.symbols.index("S")
        rest = mat[k].copy()
        rest[[a, s]] = 0.0
        mat[k] = 0.1 * rest / rest.sum()
        mat[k, a], mat[k, s] = (0.9, 0.0) if k % 2 == 0 else (0.45, 0.45)
        cons.append("a" if k % 2 == 0 else "s")
    hmm.match_emissions[:] = mat
    hmm.composition = mat[1:].mean(axis=0).astype(np.float32)
    hmm.consensus = "".join(cons)
    return hmm


def _multihit_cases():
    cases = []
    for key in T.MODEL_KEYS + ("rnd45",):
        fams = ("a" if key in T.FRAGMENT_NODES else "") + ("b" if key in T.OVERFLOW_KEYS else "")
        cases.append((key, T.model(key), [t for f in fams for t in T.targets(key, f)]))
    kr = T.model("KR")
    cons = T.consensus(kr)
    cases.append(("KR 100 kb", kr, [("KR_100kb", np.tile(cons, 100_000 // len(cons) + 1))]))
    lc = low_complexity_model()
    a, s = lc.alphabet.symbols.index("A"), lc.alphabet.symbols.index("S")
    cases.append(("low complexity", lc, [("homopolymer", np.full(5000, a, dtype=np.uint8)),
                                         ("dipeptide", np.tile(np.array([s, a], dtype=np.uint8), 2500))]))
    return cases


def test_multihit_backward_never_leaves_forwards_scales(libp7x, oracle, report):
    """The region scan decodes with a constant scaleproduct = 1 / bx[N] (regions_kernel, domaindef_regions and the oracle's
    dd_domain_decoding): right only while the multihit Backward parser keeps Forward's scale factors.  On every input here
    -- families a and b of all models, 100 kb of KR consensus copies, a homopolymer and a dipeptide repeat of 5,000 residues
    against a low-complexity model -- it keeps them (DESIGN §3.5 rests on this test); and with that, nexpected and the
    regions of the host stage are those of the reference's btot / etot / mocc, which need no scale factors at all."""
    t0 = time.time()
    for label, hmm, named in _multihit_cases():
        bg = plan7.Background(hmm.alphabet)
        op = oracle.OracleProfile(hmm, bg, 400)
        rm = R.RefModel.from_oracle(op)
        left = 0
        for name, seq in named:
            st, bsc, fx, bx = op.bck(seq)
            assert st == 0
            left += bool((fx[:, 5] != bx[:, 5]).any())
        assert left == 0, (label, "the multihit Backward parser left Forward's scale factors")
        pli = plan7.Pipeline(hmm.alphabet, T=-1e4, domT=-1e4, bias_filter=False)
        hits = host_pipeline.host_search(oracle, hmm, T.block(hmm.alphabet, named), pipeline=pli, F=(1.0, 1.0, 1.0))
        by_name = {h.name: h for h in hits}
        worst = 0.0
        for name, seq in named:
            assert name in by_name, (label, name)
            ref = R.forward_backward(rm, seq, True)
            btot, etot, mocc = ref.domain_decoding()
            h = by_name[name]
            worst = max(worst, abs(h.nexpected - btot[-1]) / max(btot[-1], 1.0))
            assert h.nregions == len(region_scan(btot, etot, mocc)), (label, name, h.nregions)
        report(f"multihit parser {label}: Backward kept Forward's scales on all {len(named)} targets; "
               f"|nexpected - btot[L]| / max(btot[L], 1) <= {worst:.3e}  ({time.time() - t0:.0f} s)")
        within(label, nexp=worst)
