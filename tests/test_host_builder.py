"""Sequence queries (phmmer) without a device: the single-sequence model of p7x_builder.cpp, the calibration stream and
the fits, driven with the oracle's scores, against HMMER's own `phmmer --domtblout` of the last sequence of PKSI.faa
against that file (tests/golden/tables/A0A089QRB9.domtbl; the reference reads it the same way, test_hmmer.py:464-493)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GOLDEN, golden_table
from pyhmmer_amd import _lib, easel, errors, plan7

N, LENGTHS = 200, (200, 200, 100)
OFFSETS = (0, 40000, 80000)


def stream_of(bg, seed=42, generator=1, abc_type=3):
    out = np.zeros(100000, dtype=np.uint8)
    bgf = np.ascontiguousarray(bg.residue_frequencies, dtype=np.float32)
    assert _lib.lib().p7x_calibration_stream(abc_type, bgf.ctypes.data, seed, generator, out.ctypes.data) == 0
    return out


def sample(stream, stage, i):
    o = OFFSETS[stage] + i * LENGTHS[stage]
    return stream[o:o + LENGTHS[stage]]


def oracle_scores(op, stream):
    """The oracle's filters over the 600 samples: scores in nats [3][200], overflow marks [2][200], raw xJ / xC."""
    sc = np.zeros((3, N), dtype=np.float32)
    ovf = np.zeros((2, N), dtype=np.uint8)
    raw = np.zeros((2, N), dtype=np.int32)
    for i in range(N):
        st, sc[0, i], raw[0, i] = op.msv(sample(stream, 0, i))
        ovf[0, i] = st != 0
        st, sc[1, i], raw[1, i] = op.vit(sample(stream, 1, i))
        ovf[1, i] = st != 0
        st, sc[2, i] = op.fwd(sample(stream, 2, i))
    return sc, ovf, raw


def fit(sc, ovf, mh):
    ev = np.zeros(6, dtype=np.float32)
    sc = np.ascontiguousarray(sc, dtype=np.float32)
    st = _lib.lib().p7x_calibration_fit(sc.ctypes.data, None if ovf is None else np.ascontiguousarray(ovf, dtype=np.uint8).ctypes.data,
                                        float(mh), ev.ctypes.data)
    return st, ev


@pytest.fixture(scope="module")
def pksi():
    abc = easel.Alphabet.amino()
    with easel.SequenceFile(GOLDEN / "seqs" / "PKSI.faa", digital=True, alphabet=abc) as sf:
        return sf.read_block()


@pytest.fixture(scope="module")
def query_model(libp7x, pksi):
    bg = plan7.Background(pksi.alphabet)
    return plan7.Builder(pksi.alphabet)._model(pksi[len(pksi) - 1], bg), bg


PLACEHOLDER = (-9.0, 0.69, -10.0, 0.69, -4.0, 0.69)       # E-value parameters that no calibration produced


@pytest.fixture(scope="module")
def searched(oracle, pksi, query_model):
    """Every target of PKSI.faa through the oracle's domain definition (all filters open: every target is scored), the model
    carrying placeholder E-value parameters: {name: (envelopes, sequence scores)}.  Nothing here depends on the calibration."""
    hmm, bg = query_model
    hmm = hmm.copy()
    hmm._evparam[:] = PLACEHOLDER
    op = oracle.OracleProfile(hmm, bg, 400)
    out = {}
    for s in pksi:
        envs, counts, sq = oracle.domains(op, np.asarray(s.sequence, dtype=np.uint8), want_sequence=True)
        out[s.name] = (envs, sq)
    return hmm, out


@pytest.fixture(scope="module")
def calibrated(oracle, query_model):
    """The six parameters of the query's model: the oracle's msv / vit / fwd over the stream, through the fit seam."""
    hmm, bg = query_model
    op = oracle.OracleProfile(hmm, bg, 100)
    om = plan7.OptimizedProfile(hmm, bg, 100)
    sc, ovf, raw = oracle_scores(op, stream_of(bg))
    st, ev = fit(sc, ovf, _lib.lib().p7x_oprofile_match_relent(om._handle))
    assert st == 0
    return ev


def test_model_of_the_query(query_model, pksi):
    hmm, bg = query_model
    q = pksi[len(pksi) - 1]
    assert hmm.M == 2085 == len(q)
    hmm.validate()
    t = hmm.transition_probabilities
    popen, pextend = np.float32(0.02), np.float32(0.4)
    assert np.all(t[:hmm.M, 0] == np.float32(1 - 2 * 0.02)) and np.all(t[:, 1] == popen) and np.all(t[:hmm.M, 2] == popen)
    assert np.all(t[:, 3] == np.float32(1 - 0.4)) and np.all(t[:, 4] == pextend)
    assert np.all(t[:hmm.M, 5] == np.float32(1 - 0.4)) and np.all(t[:hmm.M, 6] == pextend)
    assert tuple(t[hmm.M]) == (np.float32(1 - 0.02), popen, 0.0, np.float32(0.6), pextend, 1.0, 0.0)
    assert np.all(np.abs(t[:, 0:3].sum(axis=1) - 1) <= 1e-4) and np.all(np.abs(hmm.match_emissions[1:].sum(axis=1) - 1) <= 1e-4)
    assert np.array_equal(hmm.insert_emissions, np.tile(bg.residue_frequencies, (hmm.M + 1, 1)))
    assert (hmm.name, hmm.description, hmm.accession) == (q.name, q.description, q.accession or None)
    assert hmm.nseq == 1 and hmm.max_length is None
    assert hmm.consensus.upper() == "".join(q.alphabet.symbols[int(x)] for x in q.sequence)
    dsq = np.asarray(q.sequence)
    for k in (1, 2, 1000, 2085):               # the match row of a node is the conditional row of its residue: the same for equal residues
        same = np.nonzero(dsq == dsq[k - 1])[0] + 1
        assert np.array_equal(hmm.match_emissions[same], np.tile(hmm.match_emissions[k], (len(same), 1)))
        assert int(np.argmax(hmm.match_emissions[k] / bg.residue_frequencies)) == int(dsq[k - 1])      # BLOSUM62's diagonal is every row's maximum
    assert abs(float(hmm.composition.sum()) - 1.0) <= 1e-4


def test_builder_parameters_and_errors(libp7x, pksi):
    abc = easel.Alphabet.amino()
    b = plan7.Builder(abc, popen=0.05, pextend=0.5, seed=7)
    c = b.copy()
    assert (c.alphabet, c.popen, c.pextend, c.score_matrix, c.seed) == (abc, 0.05, 0.5, "BLOSUM62", 7)
    with pytest.raises(errors.InvalidParameter):
        plan7.Builder(easel.Alphabet.dna())
    with pytest.raises(errors.InvalidParameter):
        plan7.Builder(abc, score_matrix="BLOSUM90")
    with pytest.raises(errors.InvalidParameter):
        b.score_matrix = "PAM30"
    with pytest.raises(errors.InvalidParameter):
        plan7.Builder(abc, popen=0.5)
    with pytest.raises(errors.AlphabetMismatch):
        b._model(pksi[0], plan7.Background(easel.Alphabet.dna()))
    with pytest.raises(errors.AlphabetMismatch):
        b._model(easel.DigitalSequence(easel.Alphabet.dna(), name="d", sequence=np.zeros(5, np.uint8)), plan7.Background(abc))
    with pytest.raises(TypeError):
        b._model("MKV", plan7.Background(abc))
    # a degenerate residue (B = D or N): the normalised sum of its residues' joint rows, between the two rows
    bg = plan7.Background(abc)
    hmm = b._model(easel.DigitalSequence(abc, name="x", sequence=np.array([2, 11, 21], np.uint8)), bg)
    lo, hi = np.minimum(hmm.match_emissions[1], hmm.match_emissions[2]), np.maximum(hmm.match_emissions[1], hmm.match_emissions[2])
    assert np.all(hmm.match_emissions[3] >= lo - 1e-7) and np.all(hmm.match_emissions[3] <= hi + 1e-7)
    assert abs(float(hmm.match_emissions[3].sum()) - 1) <= 1e-6
    with pytest.raises(ValueError):
        b._model(easel.DigitalSequence(abc, name="gap", sequence=np.array([2, 20, 3], np.uint8)), bg)
    with pytest.raises(NotImplementedError):
        plan7.LongTargetsPipeline(easel.Alphabet.dna()).search_seq(None, None)


def test_scores_and_coordinates_reproduce_the_phmmer_table(searched):
    """The 20 rows of A0A089QRB9.domtbl: same targets in the same order, sequence score, bias and domain score within 0.1
    (the reference test's delta, the table's printed precision), hmm / ali / env coordinates equal."""
    hmm, res = searched
    rows = golden_table("A0A089QRB9.domtbl", kind="domtbl")
    assert len(rows) == 20
    order = []
    for r in rows:
        if r[0] not in order:
            order.append(r[0])
    by_score = sorted(res, key=lambda n: -res[n][1]["score"])
    assert by_score[:len(order)] == order
    for r in rows:
        envs, sq = res[r[0]]
        assert abs(sq["score"] - float(r[7])) <= 0.1 and abs((sq["pre_score"] - sq["score"]) - float(r[8])) <= 0.1, (r[0], sq)
        e = {(int(e[0]), int(e[1])): e for e in envs}.get((int(r[19]), int(r[20])))
        assert e is not None, (r[0], r[19], r[20])
        assert (int(e[4]), int(e[5]), int(e[2]), int(e[3])) == (int(r[15]), int(r[16]), int(r[17]), int(r[18])), (r[0], r[15:21])
        assert abs(e[9] - float(r[13])) <= 0.1 and abs(e[10] - float(r[14])) <= 0.1, (r[0], r[13], r[14], e[9], e[10])


def test_calibration_reproduces_the_table_evalues(searched, calibrated, pksi):
    """|ln E - ln E(table)| <= 0.06 for every non-zero E-value, c-Evalue and i-Evalue: the table prints two significant
    digits (at most 5 % relative error: ln 1.05 = 0.049, plus float formatting slack).  P-values from the calibrated
    parameters as the pipeline forms them: the exponential tail exp(-lambda (score - tau)) of a bit score above tau."""
    hmm, res = searched
    tau, lam = float(calibrated[4]), float(calibrated[5])
    lnP = lambda bits: min(0.0, -lam * (bits - tau))
    rows = golden_table("A0A089QRB9.domtbl", kind="domtbl")
    Z, domZ = len(pksi), len({r[0] for r in rows})
    checked = 0
    for r in rows:
        envs, sq = res[r[0]]
        e = {(int(e[0]), int(e[1])): e for e in envs}[(int(r[19]), int(r[20]))]
        for want, lnE in ((float(r[6]), lnP(sq["score"]) + math.log(Z)), (float(r[11]), lnP(e[9]) + math.log(domZ)),
                          (float(r[12]), lnP(e[9]) + math.log(Z))):
            if want > 0:
                assert abs(lnE - math.log(want)) <= 0.06, (r[0], r[9], want, math.exp(lnE))
                checked += 1
    assert checked >= 40


def test_stream(libp7x):
    """600 sequences of the stated lengths from one stream, a constant of (alphabet, background, seed, generator); residue
    counts over the 100,000 residues within 4 sigma of the background (binomial: sigma = sqrt(n f (1 - f)))."""
    abc = easel.Alphabet.amino()
    bg = plan7.Background(abc)
    for gen in (0, 1):
        a = stream_of(bg, generator=gen)
        assert a.shape[0] == N * sum(LENGTHS) and int(a.max()) < abc.K
        plan7.Builder(abc)._model(easel.DigitalSequence(abc, name="other", sequence=a[:50].copy()), bg)
        assert np.array_equal(a, stream_of(bg, generator=gen))
        assert not np.array_equal(a, stream_of(bg, seed=43, generator=gen))
        f = bg.residue_frequencies.astype(np.float64)
        f /= f.sum()
        n = a.shape[0]
        counts = np.bincount(a, minlength=abc.K).astype(np.float64)
        assert np.all(np.abs(counts - n * f) <= 4.0 * np.sqrt(n * f * (1.0 - f))), (gen, counts - n * f)
    assert not np.array_equal(stream_of(bg, generator=0), stream_of(bg, generator=1))
    # MT19937 with Easel's seeding (mt[z] = 69069 mt[z-1], then one generation): its first outputs for seed 42 give these residues
    uni = plan7.Background(abc, uniform=True)
    mt = [42]
    for z in range(1, 624):
        mt.append((69069 * mt[-1]) & 0xffffffff)
    for z in range(624):
        y = (mt[z] & 0x80000000) | (mt[(z + 1) % 624] & 0x7fffffff)
        mt[z] = mt[(z + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
    def temper(y):
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680; y ^= (y << 15) & 0xefc60000; y ^= y >> 18
        return y & 0xffffffff
    want = [min(19, int(temper(mt[i]) / 4294967296.0 * 20)) for i in range(600)]
    got = stream_of(uni, generator=0)[:600]
    assert sum(int(g) != w for g, w in zip(got, want)) <= 2          # a deviate on a cumulative boundary of the float sums may fall either way
    # the fast generator (esl_randomness_CreateFast): the seed dispersed by Jenkins' mix3, then x <- 69069 x + 1, restated here
    m32 = 0xffffffff
    def mix3(a, b, c):
        for s1, s2, s3 in ((13, 8, 13), (12, 16, 5), (3, 10, 15)):
            a = (a - b - c) & m32; a ^= c >> s1
            b = (b - c - a) & m32; b ^= (a << s2) & m32
            c = (c - a - b) & m32; c ^= b >> s3
        return c
    x = mix3(42, 87654321, 12345678) or 42
    want = []
    for i in range(600):
        x = (x * 69069 + 1) & m32
        want.append(min(19, int(x / 4294967296.0 * 20)))
    got = stream_of(uni, generator=1)[:600]
    assert sum(int(g) != w for g, w in zip(got, want)) <= 2


def test_fit_seam_recovers_a_gumbel_and_reports_an_overflow(libp7x):
    """Scores drawn from a Gumbel of known location and slope come back within four standard errors of the maximum-likelihood
    estimates (location at known lambda: 1 / (lambda sqrt(n)); lambda: 0.78 lambda / sqrt(n)), and agree with the Python
    fits the benchmark's library is calibrated with; an overflowed sample is refused with the range status."""
    import bench_workloads
    rng = np.random.default_rng(5)
    mh = 1.44 / 0.01                                     # lambda = ln 2 + 0.01
    lam = math.log(2.0) + 0.01
    mu = (-9.5, -11.0, -3.0)
    null1 = [L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0)) for L in LENGTHS]
    x = np.stack([m - np.log(-np.log(rng.random(N))) / lam for m in mu])
    sc = np.stack([x[s] * math.log(2.0) + null1[s] for s in range(3)]).astype(np.float32)
    st, ev = fit(sc, np.zeros((2, N), np.uint8), mh)
    assert st == 0
    assert abs(ev[1] - lam) <= 1e-6 and ev[1] == ev[3] == ev[5]
    se = 1.0 / (lam * math.sqrt(N))
    assert abs(ev[0] - mu[0]) <= 4 * se and abs(ev[2] - mu[1]) <= 4 * se
    bits = [(sc[s].astype(np.float64) - np.float32(null1[s])) / math.log(2.0) for s in range(3)]
    assert abs(ev[0] - bench_workloads._gumbel_fit_loc(bits[0], lam)) <= 1e-5
    gmu, glam = bench_workloads._gumbel_fit_complete(bits[2])
    assert abs(glam - lam) <= 4 * 0.78 * lam / math.sqrt(N)
    tau = gmu - math.log(-math.log(1.0 - 0.04)) / glam + math.log(0.04) / lam
    assert abs(ev[4] - tau) <= 1e-3
    ovf = np.zeros((2, N), np.uint8)
    ovf[1, 17] = 1
    st, _ = fit(sc, ovf, mh)
    assert st == 16 and "217" in _lib.last_error()
    assert fit(sc, None, mh)[0] == 0


def test_overflow_rule_moves_the_rest_of_the_stream(libp7x):
    """Upstream draws an overflowed sample again: the model's own stream is the common one with that draw thrown away --
    equal before it, moved by one sample behind it, across the stage boundaries."""
    bg = plan7.Background(easel.Alphabet.amino())
    bgf = np.ascontiguousarray(bg.residue_frequencies, dtype=np.float32)
    a = stream_of(bg)
    def redraw(skipped):
        out = np.zeros(100000, dtype=np.uint8)
        sk = np.asarray(skipped, dtype=np.int32)
        st = _lib.lib().p7x_calibration_redraw(3, bgf.ctypes.data, 42, 1, sk.ctypes.data, len(sk), out.ctypes.data)
        return st, out
    st, same = redraw([])
    assert st == 0 and np.array_equal(same, a)
    st, b = redraw([5])
    assert st == 0
    assert np.array_equal(b[:5 * 200], a[:5 * 200])
    assert np.array_equal(b[5 * 200:399 * 200], a[6 * 200:400 * 200])             # MSV 5..199 and Viterbi 0..198: the next draw
    assert np.array_equal(sample(b, 1, 199), np.concatenate([sample(a, 2, 0), sample(a, 2, 1)]))    # 200 residues of what were Forward samples
    assert np.array_equal(sample(b, 2, 0), sample(a, 2, 2))
    assert redraw([450])[0] == 11 and redraw([7, 3])[0] == 11                     # a Forward sample cannot overflow; increasing order
    # what the device path does when a kept sample overflows in its turn: the sample's draw joins the list (p7x_calibration_draw_of)
    def draw_of(kept, skipped):
        sk = np.asarray(skipped, dtype=np.int32)
        return _lib.lib().p7x_calibration_draw_of(kept, sk.ctypes.data, len(sk))
    assert [draw_of(k, []) for k in (0, 7, 599)] == [0, 7, 599]
    assert [draw_of(k, [5]) for k in (4, 5, 6, 398)] == [4, 6, 7, 399]
    assert [draw_of(k, [5, 6, 300]) for k in (4, 5, 297, 298)] == [4, 7, 299, 301]
    skipped = [5]
    for kept in (5, 5, 250):                      # kept sample 5 overflows twice more, then Viterbi sample 50
        skipped.append(draw_of(kept, skipped))
        assert skipped == sorted(set(skipped))
        st, c = redraw(skipped)
        assert st == 0
        keep = [d for d in range(400 + len(skipped)) if d not in skipped][:400]      # 200-residue draws of the common stream
        flat = np.concatenate([a, np.zeros(0, np.uint8)])
        for k in (0, 4, 5, 6, 199, 200, 250, 390):
            d = keep[k]
            if (d + 1) * 200 <= 80000:
                assert np.array_equal(c[k * 200:(k + 1) * 200], flat[d * 200:(d + 1) * 200]), (skipped, k, d)
    assert skipped == [5, 6, 7, 253]
