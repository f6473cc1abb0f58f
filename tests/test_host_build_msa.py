"""Builder.build_msa without a device (test seam "host_build" = 1: the host twin of the kernels of p7x_msabuild.hip counts
the same integers): the LuxC seed alignment against the model hmmbuild 3.3.2 made of it (tests/golden/hmms/LuxC.hmm), the
behaviour the fixture does not pin on small constructed alignments, the twin against a numpy float64 restatement of the
procedure (msa_cases.py), and the Stockholm reader."""
import io
import math

import numpy as np
import pytest

from conftest import GOLDEN
from pyhmmer_amd import _lib, easel, errors, plan7
import msa_cases as mc

LUXC_WEIGHTS = (1.1590, 1.3287, 1.3916, 1.3383, 0.7426, 0.7147, 0.6259, 0.6742, 0.6718, 1.0479, 0.9442, 0.9663, 1.3949)


@pytest.fixture(autouse=True)
def host_twin(libp7x):
    _lib.set_debug_option("host_build", 1)
    yield
    _lib.set_debug_option("host_build", -1)


def luxc_msa():
    with easel.MSAFile(GOLDEN / "msa" / "LuxC.sto", digital=True, alphabet=mc.AMINO) as f:
        return f.read()


def sampled_msa(hmm, n, seed):
    """emit_alignment of a model with its E-value parameters ignored, named after the model."""
    msa = hmm.emit_alignment(n, easel.Randomness(seed))
    msa.name = hmm.name
    return msa


def printed_luxc():
    """The numbers LuxC.hmm prints: COMPO, and per node the match, insert and transition lines (-ln p; inf for '*')."""
    lines = (GOLDEN / "hmms" / "LuxC.hmm").read_text().split("\n")
    body = lines[next(i for i, l in enumerate(lines) if l.startswith("HMM ")) + 2:]
    vals = lambda toks: np.array([np.inf if x == "*" else float(x) for x in toks])
    M = 400
    mat, ins, t = np.zeros((M + 1, 20)), np.zeros((M + 1, 20)), np.zeros((M + 1, 7))
    compo = vals(body[0].split()[1:21])
    ins[0], t[0] = vals(body[1].split()), vals(body[2].split())
    for k in range(1, M + 1):
        mat[k] = vals(body[3 * k].split()[1:21])
        ins[k], t[k] = vals(body[3 * k + 1].split()), vals(body[3 * k + 2].split())
    return compo, mat, ins, t


def check_luxc_model(hmm, bg, fixture):
    """Every assertion on the model of LuxC.sto (the host twin's here, the device's in test_gpu_build_msa.py)."""
    assert hmm.M == 400 and np.array_equal(hmm.map, fixture.map)
    assert hmm.checksum == 395769323 and hmm.nseq == 13
    assert abs(hmm.nseq_effective - 1.989990) < 1e-6
    assert (hmm.name, hmm.accession, hmm.description) == ("LuxC", "PF05893.5", "Acyl-CoA reductase (LuxC)")
    hmm.validate()
    compo, mat, ins, t = printed_luxc()
    nl = lambda p: -np.log(np.asarray(p, dtype=np.float64))
    with np.errstate(divide="ignore"):
        got_m, got_i, got_t, got_c = nl(hmm.match_emissions), nl(hmm.insert_emissions), nl(hmm.transition_probabilities), nl(hmm.composition)
    worst = {}
    for name, got, want in (("match", got_m[1:], mat[1:]), ("transitions", got_t, t), ("compo", got_c, compo)):
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), name
        fin = np.isfinite(want)
        worst[name] = float(np.abs(got[fin] - want[fin]).max())
    # the insert rows: one row at every node, the row the fixture prints at the 383 nodes after which no row inserts a residue
    assert np.array_equal(hmm.insert_emissions, np.tile(hmm.insert_emissions[0], (401, 1)))
    rows, n = np.unique(ins, axis=0, return_counts=True)
    common = rows[np.argmax(n)]
    assert int(n.max()) == 383
    worst["insert"] = float(np.abs(got_i[0] - common).max())
    print("largest |delta(-ln p)| against LuxC.hmm:", worst, "insert rows of the other 18 nodes:", float(np.abs(ins - common).max()))
    assert all(v <= 1e-5 for v in worst.values()), worst
    assert np.abs(ins - common).max() < 0.01
    assert hmm.consensus == fixture.consensus


@pytest.fixture(scope="module")
def luxc_model(libp7x):
    _lib.set_debug_option("host_build", 1)
    bg = plan7.Background(mc.AMINO)
    return plan7.Builder(mc.AMINO)._model_msa(luxc_msa(), bg), bg


def test_luxc_model(luxc_model, models):
    """M, MAP, CKSUM, EFFN, NSEQ; every finite -ln p of the match emissions, of the transitions of nodes 0..400 and of the
    COMPO line within 1e-5 of the printed value (half a unit of the file's last digit and as much for float32 storage;
    measured: match 5.2e-6, transitions 5.0e-6, COMPO 5.9e-6).  The insert rows: hmmbuild does not write the null model's
    frequencies there (with those, COMPO is off by 0.018) but the mean of its insert prior, which is the row the fixture
    prints at 383 of its 401 nodes; the model built here carries that row at every node, within the same 1e-5.  At the 18
    nodes after which some row inserts residues upstream adds those counts to a prior worth about 10,000 of them, which
    moves the fixture's rows by at most 0.005 there; that is not reproduced.  The consensus line equals the fixture's."""
    hmm, bg = luxc_model
    check_luxc_model(hmm, bg, models["LuxC"][0])
    assert hmm.evalue_parameters.m_mu is None or float(hmm._evparam[0]) == plan7.EVPARAM_UNSET       # not calibrated here
    assert hmm.command_line is not None and hmm.creation_time is not None and hmm.reference is None


def test_luxc_written_model_reads_back(luxc_model):
    hmm, bg = luxc_model
    text = io.StringIO()
    hmm.write(text)
    back = plan7.HMMFile(io.StringIO(text.getvalue())).read()
    again = io.StringIO()
    back.write(again)
    assert again.getvalue() == text.getvalue()
    for attr in ("M", "name", "accession", "description", "nseq", "checksum", "consensus", "creation_time", "command_line"):
        assert getattr(back, attr) == getattr(hmm, attr), attr
    assert np.array_equal(back.map, hmm.map) and abs(back.nseq_effective - hmm.nseq_effective) < 1e-6
    assert np.allclose(back.match_emissions, hmm.match_emissions, rtol=0, atol=1e-5)
    binary = io.BytesIO()
    hmm.write(binary, binary=True)
    assert plan7.HMMFile(io.BytesIO(binary.getvalue())).read() == hmm


def test_luxc_relative_weights():
    c = plan7.Builder(mc.AMINO)._msa_counts(luxc_msa())
    w = c.weights.astype(np.float64) * mc.UNIT
    assert c.weight_column_count == 397 and c.M == 400 and c.fragment_count == 0
    assert abs(w.sum() - 13.0) < 1e-9
    assert np.all(np.abs(w / np.array(LUXC_WEIGHTS) - 1.0) <= 2e-4), w


def aligned_sample(hmm, n, seed):
    """n emit_sequence draws of a model aligned to it by hmmalign's host twin (seam "host_align"): an alignment of a
    model that emit_alignment cannot give, because its paths pass through insert state 0."""
    from pyhmmer_amd import hmmer
    rng = easel.Randomness(seed)
    seqs = []
    for i in range(n):
        seq = hmm.emit_sequence(rng)
        seq.name = f"{hmm.name}-sample{i + 1}"
        seqs.append(seq)
    _lib.set_debug_option("host_align", 1)
    try:
        msa = hmmer.hmmalign(hmm, easel.DigitalSequenceBlock(hmm.alphabet, seqs), digitize=True)
    finally:
        _lib.set_debug_option("host_align", -1)
    msa.name = hmm.name
    return msa


@pytest.mark.parametrize("nodes", [83, 93])
def test_short_model_entropy_target(models, nodes):
    """Models of fewer than about 100 nodes are built to 45 + log2(M (M + 1) / 2) bits in total, not 0.59 per node: the
    built model's M x mean relative entropy lies within the entropy change across the last bisection bracket of it.
    Alignments of 40 rows sampled with seed 7 from the RREFam models of 83 and of 93 nodes.  The 93-node model enters
    insert state 0 with probability 0.31 and emit_alignment refuses a path through that state ("trace node out of
    range"), so its 40 sequences are drawn by emit_sequence and aligned by hmmalign (built model: 94 nodes)."""
    src = next(h for h in models["RREFam"] if h.M == nodes)
    msa = sampled_msa(src, 40, 7) if nodes == 83 else aligned_sample(src, 40, 7)
    bg = plan7.Background(mc.AMINO)
    builder = plan7.Builder(mc.AMINO)
    hmm = builder._model_msa(msa, bg)
    assert 76 <= hmm.M <= 96, hmm.M
    M = hmm.M
    target = 45.0 + math.log2(M * (M + 1) / 2.0)
    assert target / M > 0.59
    assert hmm.nseq == 40 and hmm.nseq_effective < 40
    counts = builder._msa_counts(msa).emissions
    bgf = bg.residue_frequencies.astype(np.float64)
    neff, (lo, hi) = mc.effective_number(counts, 40, bgf, target / M, want_bracket=True)
    assert abs(neff - hmm.nseq_effective) < 1e-6
    spread = M * abs(mc.relent(counts * (hi / 40), bgf) - mc.relent(counts * (lo / 40), bgf))
    got = M * hmm.mean_match_relative_entropy(bg)
    print("M", M, "target", target, "got", got, "bracket", spread)
    assert target - spread <= got <= target + spread


# ---------------------------------------------------------------- defined behaviour, small alignments

def build(rows, **kw):
    rf = kw.pop("rf", None)
    b = plan7.Builder(mc.AMINO, **kw)
    msa = mc.msa_of(rows, rf=rf)
    return b._msa_counts(msa), b._model_msa(msa, plan7.Background(mc.AMINO))


def test_fragment_adds_no_deletes_and_no_entry_or_exit():
    full = ["ACDEFGHIKL", "ACDEFGHIKL", "ACDEFGHIKL"]
    c0, _ = build(full, weighting="none", effective_number="none")
    c1, _ = build(full + ["---EFG----"], weighting="none", effective_number="none")
    assert c1.fragment_count == 1 and c1.fragments.tolist() == [0, 0, 0, 1] and c1.M == c0.M == 10
    t0, t1 = c0.transitions, c1.transitions
    assert np.array_equal(t1[:, 2], t0[:, 2]) and np.array_equal(t1[:, 5:], t0[:, 5:]) and not t1[:, [2, 5, 6]].any()
    assert t1[0, 0] == t0[0, 0] == 3 and t1[10, 0] == t0[10, 0] == 3            # B -> M1 and M10 -> E: the three full rows
    assert (t1[:, 0] - t0[:, 0]).tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0]      # E -> F -> G of the fragment
    assert (c1.emissions - c0.emissions).sum() == 3
    # the same row is no fragment under a lower threshold: it deletes seven nodes, enters at B and leaves at E
    c2, _ = build(full + ["---EFG----"], weighting="none", effective_number="none", fragthresh=0.2)
    assert c2.fragment_count == 0 and c2.transitions[0, 2] == 1 and c2.transitions[:, 6].sum() == 5


def test_hand_architecture_follows_the_reference_line():
    rows = ["ACDEFG", "ACDEFG", "A-DE-G", "ACD-FG"]
    c, hmm = build(rows, architecture="hand", rf="x.xx.x")
    assert c.map.tolist() == [0, 2, 3, 5] and hmm.M == 4 and hmm.reference == "xxxx" and hmm.map.tolist() == [0, 1, 3, 4, 6]
    assert c.weight_columns.tolist() == [1, 0, 1, 1, 0, 1]
    c, hmm = build(rows)
    assert c.map.tolist() == [0, 1, 2, 3, 4, 5] and hmm.reference is None
    with pytest.raises(ValueError, match="Could not build HMM"):
        build(rows, architecture="hand")


def test_alignments_that_cannot_be_built():
    bg = plan7.Background(mc.AMINO)
    b = plan7.Builder(mc.AMINO)
    with pytest.raises(ValueError, match="Could not build HMM"):
        b._model_msa(mc.msa_of(["----", "----", "----"]), bg)
    with pytest.raises(ValueError, match="Could not build HMM"):
        b._model_msa(mc.msa_of(["ACDE", "ACDE"], name=None), bg)
    with pytest.raises(ValueError, match="Could not build HMM"):
        b._model_msa(easel.DigitalMSA(mc.AMINO, name="empty"), bg)
    with pytest.raises(errors.AlphabetMismatch):
        b._model_msa(mc.msa_of(["ACDE"]), plan7.Background(easel.Alphabet.dna()))
    with pytest.raises(TypeError):
        b._model_msa(mc.msa_of(["ACDE"]).textize(), bg)
    _lib.set_debug_option("host_build", -1)
    if _lib.lib().p7x_device_count() == 0:
        with pytest.raises(errors.DeviceUnavailable):
            b._model_msa(mc.msa_of(["ACDE", "ACDE"]), bg)


def test_weighting_and_effective_number_options():
    rows = ["ACDEFGHI", "ACDEFGHI", "ACDEFGHI", "WCDYFGHI", "ACD-FGH-"]
    c, hmm = build(rows, weighting="none", effective_number="none")
    assert np.all(c.weights == 1 << 40) and hmm.nseq_effective == 5 and hmm.nseq == 5
    c, hmm = build(rows, effective_number=2.0)
    assert hmm.nseq_effective == 2.0
    w = c.weights * mc.UNIT
    assert abs(w.sum() - 5) < 1e-9 and w[3] > w[0] > w[4] and w[0] == w[1] == w[2]
    # by hand: the columns hold A A A W A / C x5 / D x5 / E E E Y - / F x5 / G x5 / H x5 / I I I I -
    full = (1 / 8 + 5 * (1 / 5) + 1 / 6 + 1 / 4) / 8
    odd = (1 / 2 + 5 * (1 / 5) + 1 / 2 + 1 / 4) / 8
    short = (1 / 8 + 5 * (1 / 5)) / 6
    want = np.array([full, full, full, odd, short])
    assert np.allclose(w, want * 5 / want.sum(), rtol=0, atol=1e-9)


def test_laplace_posterior_means():
    rows = ["AC", "AC", "A-", "WC"]
    c, hmm = build(rows, weighting="none", effective_number="none", prior_scheme="laplace")
    m = hmm.match_emissions.astype(np.float64)
    assert abs(m[1, 0] - 4 / 24) < 1e-7 and abs(m[1, 18] - 2 / 24) < 1e-7 and abs(m[1, 1] - 1 / 24) < 1e-7
    assert abs(m[2, 1] - 4 / 23) < 1e-7 and abs(m[2, 0] - 1 / 23) < 1e-7
    t = hmm.transition_probabilities.astype(np.float64)
    assert np.allclose(t[0, :3], [5 / 7, 1 / 7, 1 / 7]) and np.allclose(t[1, :3], [4 / 7, 1 / 7, 2 / 7])      # B -> M1 x4; M1 -> M2 x3, M1 -> D2 x1
    assert np.allclose(t[2], [4 / 5, 1 / 5, 0, 0.5, 0.5, 1, 0])              # node M: (4, 1, 1) / 6 of M -> E x3, then no M -> D; D -> E is 1
    assert np.allclose(t[1, 3:], [0.5, 0.5, 0.5, 0.5]) and np.allclose(t[0, 3:], [0.5, 0.5, 1, 0])


def test_degenerate_residue_spreads_its_count():
    c, _ = build(["AB", "AD", "AN"], weighting="none", effective_number="none")
    e = c.emissions
    assert e[2, 2] == 1.5 and e[2, 11] == 1.5 and e[2].sum() == 3 and c.node_counts[2, 21] == 1 << 40
    c, _ = build(["AX", "AD"], weighting="none", effective_number="none")
    assert np.allclose(c.emissions[2], np.full(20, 0.05) + np.eye(20)[2])


def test_delete_next_to_inserted_residues_becomes_a_match():
    """Plan 7 has neither D->I nor I->D: the delete takes the inserted residue before it, else the one after it."""
    rows = ["AC.DE", "AC.DE", "AC.DE", "A-w-E", "A-wyE".replace("y", "-")]
    c, _ = build(rows, weighting="none", effective_number="none")
    assert c.map.tolist() == [0, 1, 3, 4]
    t, e = c.transitions, c.emissions
    assert e[2, 18] == 2 and e[2, 1] == 3                    # node 2 took the W of both gapped rows
    assert t[1].tolist() == [5, 0, 0, 0, 0, 0, 0] and t[2].tolist() == [3, 0, 2, 0, 0, 0, 0] and t[3, 5] == 2
    ref = mc.build(mc.msa_of(rows)._codes(), plan7.Background(mc.AMINO).residue_frequencies, weighting="none", effective="none")
    assert np.array_equal(ref["t"], t) and np.array_equal(ref["mat"], e)


def test_builder_options():
    abc = mc.AMINO
    b = plan7.Builder(abc)
    assert (b.architecture, b.weighting, b.effective_number, b.prior_scheme, b.symfrac, b.fragthresh, b.ere, b.esigma) == \
        ("fast", "pb", "entropy", "alphabet", 0.5, 0.5, None, 45.0)
    b = plan7.Builder(abc, architecture="hand", weighting="none", effective_number=3.5, prior_scheme="laplace", symfrac=0.6,
                      fragthresh=0.3, ere=0.7, esigma=40.0, popen=0.05, seed=9)
    c = b.copy()
    for attr in ("architecture", "weighting", "effective_number", "prior_scheme", "symfrac", "fragthresh", "ere", "esigma", "popen",
                 "pextend", "score_matrix", "seed"):
        assert getattr(c, attr) == getattr(b, attr), attr
    for kw in (dict(architecture="slow"), dict(weighting="gsc"), dict(weighting="blosum"), dict(effective_number="clust"),
               dict(effective_number=-1.0), dict(prior_scheme="bogus"), dict(symfrac=1.5), dict(fragthresh=-0.1), dict(ere=0.0)):
        with pytest.raises(errors.InvalidParameter):
            plan7.Builder(abc, **kw)
    with pytest.raises(errors.InvalidParameter, match="pb"):
        plan7.Builder(abc, weighting="gsc")


# ---------------------------------------------------------------- the twin against the float64 restatement

def against_restatement(msa):
    """The twin's fixed-point weights and counts against the float64 sums, and its probabilities, as the library holds
    them in double before it stores them as float32, within 1e-9 of the restatement's.
    Weights and counts: within 300 x 2^-40 of the float64 sums (the terms of a weight and the weight itself are rounded
    to the unit 2^-40, and the scaling to sum N multiplies that by up to N = 300).  A count is sum_i w_i m_i with m_i = 1,
    except the I->I count of a node, where m_i is the row's inserted residues there less one: that count gets the same
    bound times the largest m_i of its node (measured on the sampled alignment: 441 units at the worst node, 21 units per
    unit of its multiplier; LuxC: 5 units).
    Beside that bound, the restatement run with the twin's own weights must give the twin's counts to the rounding of
    float64 sums (1e-12 relative): a wrong I->I count cannot hide in the room the multiplier needs."""
    bg = plan7.Background(mc.AMINO)
    b = plan7.Builder(mc.AMINO)
    c = b._msa_counts(msa)
    hmm = plan7.HMM(mc.AMINO, c.M, msa.name)
    neff, t64, mat64 = b._msa_parameters(c, bg, hmm)
    ax = msa._codes()
    ref = mc.build(ax, bg.residue_frequencies)
    assert np.array_equal(ref["consensus"], c.map) and np.array_equal(ref["frag"], c.fragments.astype(bool))
    marked, frag = mc.mark_fragments(ax, 0.5)
    w = c.weights * mc.UNIT                                  # exact: 64-bit integers below 2^53 here
    assert int(c.weights.max()) < 2 ** 53
    d = np.abs(w - ref["weights"]) / mc.UNIT
    mult = np.maximum(mc.insert_lengths(marked, frag, c.map).max(axis=0) - 1, 1)
    dt = np.abs(c.transitions - ref["t"]) / mc.UNIT
    worst = {"weights": d.max(), "emissions": np.abs(c.emissions - ref["mat"]).max() / mc.UNIT,
             "transitions but I->I": np.delete(dt, 4, axis=1).max(), "I->I over its multiplier": (dt[:, 4] / mult).max(),
             "I->I": dt[:, 4].max(), "largest multiplier": int(mult.max()),
             "match probabilities": np.abs(mat64 - ref["pm"]).max(), "transition probabilities": np.abs(t64 - ref["pt"]).max()}
    print(msa.name, "against the restatement (counts in units of 2^-40):", {k: float(v) for k, v in worst.items()})
    assert c.N <= 300 and worst["weights"] <= 300
    assert worst["emissions"] <= 300 and worst["transitions but I->I"] <= 300 and worst["I->I over its multiplier"] <= 300
    own_mat, own_t = mc.counts(marked, frag, w, c.map)
    assert np.allclose(c.emissions, own_mat, rtol=1e-12, atol=1e-12) and np.allclose(c.transitions, own_t, rtol=1e-12, atol=1e-12)
    assert neff == ref["neff"]
    assert worst["match probabilities"] <= 1e-9 and worst["transition probabilities"] <= 1e-9
    assert np.array_equal(hmm.match_emissions, mat64.astype(np.float32))
    assert np.array_equal(hmm.transition_probabilities, t64.astype(np.float32))


def test_twin_against_restatement_luxc():
    against_restatement(luxc_msa())


def test_twin_against_restatement_sampled(models):
    against_restatement(sampled_msa(models["PF02826"][0], 300, 5))


def test_insert_counts_beyond_64_bits():
    """The I->I count of a node sums (inserted residues - 1) x weight over the rows: 4,096 rows of unit weight (2^40) with
    4,198 residues between two consensus columns make 4,096 x 4,197 x 2^40 > 2^64.  The count is kept in two sums
    (transition_counts slots 4 and 7) and comes out exact."""
    n, alen = 4096, 4200
    row = "A" + "C" * (alen - 2) + "D"
    b = plan7.Builder(mc.AMINO, architecture="hand", weighting="none", effective_number="none")
    c = b._msa_counts(mc.msa_of([row] * n, rf="x" + "." * (alen - 2) + "x", names=[f"r{i}" for i in range(n)]))
    assert c.M == 2 and n * (alen - 3) * 2 ** 40 > 2 ** 64
    q = c.transition_counts
    assert int(q[1, 4]) + (int(q[1, 7]) << 20) == n * (alen - 3) << 40
    t = c.transitions
    assert t[1].tolist() == [0, n, 0, n, n * (alen - 3), 0, 0] and t[0].tolist() == [n, 0, 0, 0, 0, 0, 0]
    hmm = b._model_msa(mc.msa_of([row] * n, rf="x" + "." * (alen - 2) + "x", names=[f"r{i}" for i in range(n)]), plan7.Background(mc.AMINO))
    assert abs(float(hmm.transition_probabilities[1, 4]) - (n * (alen - 3) + 0.1331) / (n * (alen - 2) + 0.2882)) < 1e-7


def test_twin_on_several_threads():
    """From 1,024 rows on the twin splits the rows over threads and adds their integer sums: eight copies of 256 rows
    count eight times what the 256 rows count (unit weights), fragments and taken residues included."""
    rows = mc.random_rows(256, 90, seed=3)
    rows[5] = "-" * 40 + rows[5][40:60] + "-" * 30
    b = plan7.Builder(mc.AMINO, weighting="none")
    one, many = b._msa_counts(mc.msa_of(rows)), b._msa_counts(mc.msa_of(rows * 8, names=[f"r{i}" for i in range(2048)]))
    assert one.fragment_count == 1 and many.fragment_count == 8 and np.array_equal(one.map, many.map)
    for name in ("column_counts", "weighted_counts", "node_counts", "transition_counts"):
        assert np.array_equal(getattr(one, name) * 8, getattr(many, name)), name
    assert one.transition_counts[:, [1, 3, 4]].all(axis=0).any() or one.transition_counts[:, 1].any()


# ---------------------------------------------------------------- MSAFile

def test_msafile_reads_luxc():
    with easel.MSAFile(GOLDEN / "msa" / "LuxC.sto") as f:
        msa = f.read()
        assert f.read() is None
    assert isinstance(msa, easel.TextMSA) and len(msa.names) == 13 and len(msa) == 445
    assert (msa.name, msa.accession, msa.description) == ("LuxC", "PF05893.5", "Acyl-CoA reductase (LuxC)")
    assert msa.names[0] == "Q9KV99_VIBCH/423-818" and msa._accs[0] == "Q9KV99.1"
    d = luxc_msa()
    assert isinstance(d, easel.DigitalMSA) and d.name == "LuxC" and d._codes().shape == (13, 445)
    assert mc.checksum(d._codes()) == 395769323 == _lib.lib().p7x_msa_checksum(d._codes().ctypes.data, 13 * 445)
    with pytest.raises(ValueError):
        easel.MSAFile(GOLDEN / "msa" / "LuxC.sto", format="clustal")
    with pytest.raises(ValueError):
        easel.MSAFile(io.StringIO(">seq\nACDE\n")).read()
    assert "MSAFile" in easel.__all__


@pytest.mark.parametrize("name", ["KR-1.sto", "LuxC.hmmalign.sto"])
def test_msafile_reads_what_the_writer_wrote(name):
    """The alignments hmmsearch -A and hmmalign wrote: rows, per-row annotation and the #=GC lines read back; written again
    they give their own bytes where the writer knows all their annotation (KR-1.sto carries a #=GF AU line it does not)."""
    whole = (GOLDEN / "msa" / name).read_text()
    text = whole[:whole.index("//\n") + 3]                  # the first alignment of the file
    with easel.MSAFile(io.StringIO(whole)) as f:
        msa = f.read()
        assert 1 + len(list(f)) == whole.count("//\n")
    out = io.StringIO()
    msa.write(out)
    if "#=GF AU" not in text:
        assert out.getvalue() == text
    again = easel.MSAFile(io.StringIO(out.getvalue())).read()
    assert again == msa and again.name == msa.name
    assert len(msa.names) > 0 and all(len(r) == len(msa) for r in msa.alignment)
    assert msa.reference is None or len(msa.reference) == len(msa)
    if "#=GC RF" in text:
        assert msa.reference is not None and msa.reference == "".join(l.split()[2] for l in text.split("\n") if l.startswith("#=GC RF"))
    if "#=GR" in text:
        assert msa.posterior_probabilities is not None and len(msa.posterior_probabilities) == len(msa.names)


def test_msafile_iterates_over_several_alignments():
    one = (GOLDEN / "msa" / "LuxC.sto").read_text()
    two = "# STOCKHOLM 1.0\n#=GF ID tiny\n\nr1 AC-E\nr2 ACDE\n#=GC RF xx.x\n\nr1 FG\nr2 F-\n#=GC RF xx\n//\n"
    with easel.MSAFile(io.StringIO(one + two), digital=True, alphabet=mc.AMINO) as f:
        msas = list(f)
    assert [m.name for m in msas] == ["LuxC", "tiny"] and [len(m) for m in msas] == [445, 6]
    assert msas[1].alignment == ("AC-EFG", "ACDEF-") and msas[1].reference == "xx.xxx"
    with pytest.raises(ValueError):
        list(easel.MSAFile(io.StringIO(one.replace("//", ""))))
