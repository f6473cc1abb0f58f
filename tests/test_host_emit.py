"""Sampling on the host: easel.Randomness, HMM.emit_sequence / emit_alignment / sample, Profile.emit_sequence, and the host
twin of the device emitter (HMM.emit_block under the test seam "host_emit" = 1; tests/test_gpu_emit.py compares the kernel
with it byte for byte).  What is checked is the distribution, the generators and determinism -- no fixture pins
upstream's draw-for-draw stream, and none is claimed."""
import ctypes as C
import pickle

import numpy as np
import pytest

import gap_models
from conftest import load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, errors, plan7
from test_host_builder import stream_of

MM, MI, MD, IM, II, DM, DD = range(7)
ST_M, ST_I = 1, 3


@pytest.fixture
def host_emit(libp7x):
    _lib.set_debug_option("host_emit", 1)
    yield
    _lib.set_debug_option("host_emit", -1)
    _lib.set_debug_option("emit_cap", -1)


# ---------------------------------------------------------------------------------------------------- the test models
def all_delete_hmm():
    """gap_models.gappy_hmm with EVERY M->D at 0.9 and every D->D at 0.97: about one path in six deletes all 60 nodes."""
    hmm = gap_models.gappy_hmm(60, 5)
    t = np.array(hmm.transition_probabilities, dtype=np.float64)
    M = hmm.M
    t[0:M, MM], t[0:M, MI], t[0:M, MD] = 0.08, 0.02, 0.9
    t[1:M, DM], t[1:M, DD] = 0.03, 0.97
    hmm.transition_probabilities[:] = t
    return hmm


def long_insert_hmm():
    """One node whose insert state is entered by every other path and left with probability 0.01."""
    hmm = random_hmm(30, 11)
    t = np.array(hmm.transition_probabilities, dtype=np.float64)
    t[10, MM], t[10, MI], t[10, MD] = 0.45, 0.5, 0.05
    t[10, IM], t[10, II] = 0.01, 0.99
    hmm.transition_probabilities[:] = t
    return hmm


def sampled(M, seed, abc=None):
    return plan7.HMM.sample(abc or easel.Alphabet.amino(), M, seed)


def check_paths(hmm, db):
    """Every residue a canonical one; every path a legal core path: nodes never fall, a match state is at a later node than
    whatever came before, an insert state follows a match or insert state of its own node (so never a delete state)."""
    K, M = hmm.alphabet.K, hmm.M
    assert (db.lengths > 0).all()
    for i in range(len(db)):
        o, L = int(db.offsets[i]), int(db.lengths[i])
        dsq, st, node = db.block.packed().dsq[o:o + L], db.states[o:o + L], db.nodes[o:o + L]
        assert dsq.max() < K and set(st.tolist()) <= {ST_M, ST_I}
        assert node.min() >= 0 and node.max() <= M and (node[st == ST_M] >= 1).all()
        prev = np.concatenate([[0], node[:-1]])
        assert (node[st == ST_M] > prev[st == ST_M]).all()
        assert (node[st == ST_I] == prev[st == ST_I]).all()
        assert db.block.packed().dsq[o - 1] == 255 and db.block.packed().dsq[o + L] == 255


# ---------------------------------------------------------------------------------------------------- Randomness
@pytest.mark.parametrize("fast", [False, True])
def test_randomness_streams(libp7x, fast):
    a, b = easel.Randomness(42, fast=fast), easel.Randomness(42, fast=fast)
    xs = [a.random() for _ in range(700)]                     # past one refill of the twister's 624 words
    assert xs == [b.random() for _ in range(700)]
    assert xs != [easel.Randomness(43, fast=fast).random() for _ in range(700)]
    assert a.fast is fast and repr(a) == f"Randomness(42, fast={fast})"
    c = a.copy()
    state = a.getstate()
    nxt = [a.random() for _ in range(10)]
    assert [c.random() for _ in range(10)] == nxt
    d = easel.Randomness(7, fast=not fast)
    d.setstate(state)
    assert d.fast is fast and [d.random() for _ in range(10)] == nxt
    e = pickle.loads(pickle.dumps(a))
    assert [e.random() for _ in range(5)] == [a.random() for _ in range(5)]
    a.seed(42)
    assert [a.random() for _ in range(3)] == xs[:3]
    u = easel.Randomness(3, fast=fast)._draw(100000)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert easel.Randomness(0, fast=fast).getstate()[1] != 0          # an arbitrary seed was taken
    g = [easel.Randomness(5, fast=fast).normalvariate(2.0, 0.5) for _ in range(3)]
    assert g[0] == g[1] == g[2] and np.isfinite(g[0])


@pytest.mark.parametrize("generator", [0, 1])
def test_randomness_is_the_calibration_streams_generator(libp7x, generator):
    """The calibration stream (pinned by the phmmer E-value tests) is esl_rsq_xfIID over the generator's deviates: drawing
    the same deviates from Randomness and choosing as esl_rnd_FChoose does gives its first residues -- one generator, not two."""
    bg = plan7.Background(easel.Alphabet.amino())
    want = stream_of(bg, 42, generator)[:2000]
    p = np.ascontiguousarray(bg.residue_frequencies, dtype=np.float32)
    fs = c = np.float32(0.0)
    for x in p:                                               # the Kahan sum of the norm, in float
        y = np.float32(x - c); t = np.float32(fs + y); c = np.float32(np.float32(t - fs) - y); fs = t
    cum = np.cumsum(p.astype(np.float64)) / float(fs)
    u = easel.Randomness(42, fast=bool(generator))._draw(2000)
    got = np.array([int(np.argmax(x < cum)) if (x < cum).any() else len(p) - 1 for x in u], dtype=np.uint8)
    assert np.array_equal(got, want)


def test_philox_known_answers(libp7x):
    """Philox-4x32-10 against the known-answer vectors of the Random123 distribution (key, counter -> output)."""
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 2, (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:
        k, c, o = np.array(key, np.uint32), np.array(ctr, np.uint32), np.zeros(4, np.uint32)
        assert libp7x.p7x_debug_philox(k.ctypes.data, c.ctypes.data, o.ctypes.data) == 0
        assert tuple(int(x) for x in o) == want


# ---------------------------------------------------------------------------------------------------- core emitter
def test_edge_models(host_emit):
    one = sampled(1, 3)
    db = one.emit_block(500, seed=9, traces=True)             # M1, I0, I1, D1: the all-delete path B D1 E is drawn again
    check_paths(one, db)
    assert set(db.nodes[db.states == ST_M].tolist()) == {1} and set(db.nodes[db.states == ST_I].tolist()) <= {0, 1}
    assert (db.attempts > 0).any()
    check_paths(sampled(2, 4), sampled(2, 4).emit_block(500, seed=9, traces=True))
    dna = random_hmm(50, 3, alphabet=easel.Alphabet.dna())
    check_paths(dna, dna.emit_block(300, seed=1, traces=True))
    gaps = all_delete_hmm()
    db = gaps.emit_block(2000, seed=2, traces=True)
    check_paths(gaps, db)
    assert (db.lengths > 0).all() and 150 < int((db.attempts > 0).sum()) < 600       # P(empty path) = 0.9 x 0.97^58 = 0.154


def test_overflow_redraw_is_identical(host_emit):
    hmm = long_insert_hmm()
    whole = hmm.emit_block(400, seed=5, traces=True)
    assert whole.redrawn < 200 and int(whole.lengths.max()) > 300
    _lib.set_debug_option("emit_cap", 8)
    small = hmm.emit_block(400, seed=5, traces=True)
    assert small.cap == 8 and small.redrawn == int((small.lengths > 8).sum()) > 300
    for a, b in ((whole.lengths, small.lengths), (whole.block.packed().dsq, small.block.packed().dsq), (whole.states, small.states),
                 (whole.nodes, small.nodes), (whole.attempts, small.attempts)):
        assert np.array_equal(a, b)
    check_paths(hmm, small)


def test_stream_independence_and_names(host_emit):
    hmm = load_hmms("PF02826")[0]
    few, many = hmm.emit_block(65, seed=7), hmm.emit_block(1000, seed=7)
    assert all(np.array_equal(few[i].sequence, many[i].sequence) for i in range(65))
    assert not np.array_equal(hmm.emit_block(65, seed=8)[0].sequence, few[0].sequence)
    assert few[3].name == "2-Hacid_dh_C-sample3" and len(few) == 65 and isinstance(few.block, easel.DigitalSequenceBlock)
    assert few.states is None and not few.on_device
    empty = hmm.emit_block(0)
    assert len(empty) == 0 and len(empty.block) == 0 and empty.block.packed().dsq.tolist() == [255]


def test_errors(libp7x):
    hmm = sampled(5, 1)
    with pytest.raises(ValueError):
        hmm.emit_block(-1)
    if libp7x.p7x_device_count() == 0:
        with pytest.raises(errors.DeviceUnavailable):
            hmm.emit_block(4)
    stuck = sampled(5, 1)
    stuck.transition_probabilities[2, IM], stuck.transition_probabilities[2, II] = 0.0, 1.0
    with pytest.raises(ValueError):
        stuck.emit_sequence(1)
    # the size computation behind P7X_EMEM: slots and packed copy of n sequences, six times as much with traces
    need = C.c_int64()
    assert libp7x.p7x_debug_emit_bytes(1000000, 400, 0, -1, C.byref(need)) == 0 and need.value >= 2 * 400 * 1000000
    plain = need.value
    assert libp7x.p7x_debug_emit_bytes(1000000, 400, 1, -1, C.byref(need)) == 0 and need.value > 5 * plain
    assert libp7x.p7x_debug_emit_bytes(1000000, 400, 0, plain - 1, C.byref(need)) == 5
    assert libp7x.p7x_debug_emit_bytes(1000000, 400, 0, plain, C.byref(need)) == 0
    assert libp7x.p7x_debug_emit_bytes(1 << 60, 400, 0, -1, C.byref(need)) == 5
    assert libp7x.p7x_debug_emit_bytes(10, 6, 0, -1, C.byref(need)) == 11


def cumulative(row):
    row = np.asarray(row, dtype=np.float64)
    return row / row.sum()


def within(count, v, p):
    return abs(count - v * p) <= 6.0 * np.sqrt(v * p * (1.0 - p)) + 1.0


def test_distribution(host_emit):
    """20,000 paths through a 12-node sampled model: every transition count out of a state visited v times lies within
    6 sqrt(v p (1 - p)) + 1 of v p, and so does every emission count.  Paths that emitted nothing (attempts) are counted
    too, so the counts are of the unconditioned chain.  About 650 cells at six sigma: under 1e-5 false alarms expected."""
    hmm = sampled(12, 2024)
    M, K = hmm.M, hmm.alphabet.K
    n = 20000
    db = hmm.emit_block(n, seed=12345, traces=True)
    tc = np.zeros((M + 1, 7), dtype=np.int64)
    mc, ic = np.zeros((M + 1, K), dtype=np.int64), np.zeros((M + 1, K), dtype=np.int64)
    dsq = db.block.packed().dsq

    def deletes(k, to):                        # M_k -> D_k+1 .. D_to-1 -> (M_to | E when to = M + 1)
        tc[k, MD] += 1
        for d in range(k + 1, to - 1):
            tc[d, DD] += 1
        tc[to - 1, DM] += 1
    for i in range(n):
        o, L = int(db.offsets[i]), int(db.lengths[i])
        for _ in range(int(db.attempts[i])):
            deletes(0, M + 1)
        s, k = ST_M, 0
        for r in range(o, o + L):
            s2, k2 = int(db.states[r]), int(db.nodes[r])
            if s2 == ST_I:
                tc[k, MI if s == ST_M else II] += 1
                ic[k2, dsq[r]] += 1
            else:
                if k2 == k + 1:
                    tc[k, MM if s == ST_M else IM] += 1
                else:
                    assert s == ST_M
                    deletes(k, k2)
                mc[k2, dsq[r]] += 1
            s, k = s2, k2
        if k == M:
            tc[k, MM if s == ST_M else IM] += 1
        else:
            assert s == ST_M
            deletes(k, M + 1)
    t = np.asarray(hmm.transition_probabilities, dtype=np.float64)
    cells = 0
    for k in range(M + 1):
        for cols in ((MM, MI, MD), (IM, II), (DM, DD)):
            v, p = tc[k, list(cols)].sum(), cumulative(t[k, list(cols)])
            for c, pc in zip(cols, p):
                assert within(tc[k, c], v, pc), (k, c, tc[k, c], v, pc)
                cells += 1
        for counts, probs in ((mc, hmm.match_emissions), (ic, hmm.insert_emissions)):
            if k == 0 and counts is mc:
                assert counts[0].sum() == 0
                continue
            v, p = counts[k].sum(), cumulative(probs[k])
            for x in range(K):
                assert within(counts[k, x], v, p[x]), (k, x, counts[k, x], v, p[x])
                cells += 1
    assert cells > 500 and tc.sum() > 12 * n


# ---------------------------------------------------------------------------------------------------- the reference's calls
def test_emit_sequence(libp7x):
    hmm = load_hmms("PF02826")[0]
    a, b = hmm.emit_sequence(42), hmm.emit_sequence(easel.Randomness(42, fast=True))
    assert np.array_equal(a.sequence, b.sequence) and a.name == "" and 100 < len(a) < 300 and a.sequence.max() < 20
    rng = easel.Randomness(123)
    assert not np.array_equal(hmm.emit_sequence(rng).sequence, hmm.emit_sequence(rng).sequence)
    one = sampled(1, 3)
    rng = easel.Randomness(1)
    assert all(len(one.emit_sequence(rng)) >= 1 for _ in range(200))
    tiny = long_insert_hmm()                                  # longer than the first buffer: drawn again from the same state
    lens = [len(tiny.emit_sequence(easel.Randomness(s))) for s in range(1, 40)]
    assert max(lens) > 200


def test_emit_alignment(libp7x):
    hmm = load_hmms("PF02826")[0]
    msa = hmm.emit_alignment(5, 17)
    assert isinstance(msa, easel.DigitalMSA) and len(msa.sequences) == 5
    assert msa.names == tuple(f"2-Hacid_dh_C-sample{i}" for i in range(1, 6))
    rows = msa.alignment
    consensus = [j for j in range(len(rows[0])) if all(r[j] == "-" or r[j].isupper() for r in rows)]
    inserts = [j for j in range(len(rows[0])) if all(r[j] == "." or r[j].islower() for r in rows)]
    assert len(consensus) == hmm.M and len(consensus) + len(inserts) == len(rows[0])
    seqs, traces = hmm._emit_traces(5, easel.Randomness(17, fast=True))       # the same stream: the same five paths
    for row, s in zip(rows, seqs):
        assert row.replace("-", "").replace(".", "").upper() == hmm.alphabet.decode(s.sequence)
    again = plan7.TraceAligner().align_traces(hmm, seqs, traces, digitize=True, all_consensus_cols=True)
    assert again.alignment == rows
    assert len(hmm.emit_alignment(0, 1).sequences) == 0


def test_profile_emit_sequence(libp7x):
    hmm = load_hmms("PF02826")[0]
    profile = hmm.to_profile(L=200)
    with pytest.raises(errors.AlphabetMismatch):
        profile.emit_sequence(random_hmm(20, 1, alphabet=easel.Alphabet.dna()))
    with pytest.raises(errors.AlphabetMismatch):
        profile.emit_sequence(hmm, plan7.Background(easel.Alphabet.dna()))
    a, b = profile.emit_sequence(hmm, None, 9), profile.emit_sequence(hmm, plan7.Background(hmm.alphabet), easel.Randomness(9, fast=True))
    assert np.array_equal(a.sequence, b.sequence) and a.sequence.max() < 20
    # The mean length against the configured profile's own special-state probabilities (OptimizedProfile.xf, rows E, N, J,
    # C; columns move, loop): a state that loops with p emits p / (1 - p) residues; the core is passed 1 / P(E -> C) times
    # on average and J once less.  The mean length of a pass is taken from THESE draws (fragments are local, so the mean of
    # the full-length core emitter does not apply): that term cancels against the lengths it is part of and checks
    # nothing by itself.  What this assertion checks is the N / J / C loops; the next one checks the number of passes.
    xf = profile.to_optimized().xf.astype(np.float64)
    (e_move, e_loop), n_loop, j_loop, c_loop = xf[0], xf[1, 1], xf[2, 1], xf[3, 1]
    assert abs(n_loop - 200.0 / 203.0) < 1e-6 and n_loop == j_loop == c_loop and e_loop == e_move == 0.5
    passes = 1.0 / e_move
    rng = easel.Randomness(31)
    draws = [profile._emit(hmm, None, rng) for _ in range(2000)]
    lens = np.array([len(d[0]) for d in draws], dtype=np.float64)
    core, hits = sum(d[1] for d in draws), sum(d[2] for d in draws)
    expected = n_loop / (1.0 - n_loop) + c_loop / (1.0 - c_loop) + (passes - 1.0) * j_loop / (1.0 - j_loop) + passes * core / hits
    assert abs(lens.mean() - expected) <= 6.0 * lens.std(ddof=1) / np.sqrt(len(lens)), (lens.mean(), expected)
    assert abs(hits / 2000.0 - passes) <= 6.0 * np.sqrt(e_loop / e_move ** 2 / 2000.0)      # geometric: variance (1 - p) / p^2
    assert 1 <= core / hits < hmm.M


@pytest.mark.parametrize("M", [1, 2, 65])
def test_hmm_sample(libp7x, M):
    for abc in (easel.Alphabet.amino(), easel.Alphabet.dna()):
        hmm = plan7.HMM.sample(abc, M, 42)
        hmm.validate()
        assert hmm.M == M and hmm.name == "sampled-hmm" and len(hmm.consensus) == M
        assert hmm == plan7.HMM.sample(abc, M, easel.Randomness(42))
        assert hmm != plan7.HMM.sample(abc, M, 43)
        assert hmm.max_length is None                           # as p7_hmm_Sample: a long-target search computes its own
        t = hmm.transition_probabilities
        assert t[M, MD] == 0.0 and t[M, DD] == 0.0 and t[M, DM] == 1.0 and t[0, DM] == 1.0
