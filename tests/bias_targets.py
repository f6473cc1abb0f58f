"""Targets and models for the bias filter's float64 reference (test input only), each as small as the edge it aims at.

Models (MODEL_KEYS): random_hmm at M = 1, 7, 8, 9 (L1 = M / 8 below, at and above 1), 262, 2,048 and 8,192; the KR fixture
(its file has no COMPO line: the composition is all zero and the composition state dead on every residue) and the LuxC
fixture (with one); a DNA model; "zero", an amino model whose composition is exactly 0 for two residues (one state of the filter HMM dead on
them); "bg", a model scored against a non-uniform, non-default Background.

Families, per model:
(a) lengths: 1, 2, 3 and every length around the kernel's 16-residue blocks and their prefetch (15-18, 31-34, 47-50, 63-66,
    127-130), 1,000 and one of 20,000 background residues; two empty targets stand between scored ones.
(b) composition: background residues; residues drawn from the model's composition; homopolymers of the residue with the
    largest and with the smallest compo / bgf and two-letter repeats (largest + smallest, the two largest) at L = 17, 300
    and 5,000 -- on the repeats of the largest the composition state wins every residue and the running sum of logs grows
    by about a nat per residue; half background then half biased and the reverse, so the state switches once.
(c) codes: every degenerate and special code of the alphabet (gap, '*', '~' included) at positions 1, 2, 16, 17 and L of a
    40-residue background target, and a target made only of the any-residue code.
(d) many targets: 70,000 targets of 1-40 residues (more than one grid stride of 64 x 4 x 256 lanes), one in eight residues
    of every eighth target a degenerate code; its first 1, 63, 64 and 65 targets are the small blocks."""
import functools
import math

import numpy as np

from conftest import load_hmms, random_hmm
from pyhmmer_amd import easel, plan7

RANDOM_M = (1, 7, 8, 9, 262, 2048, 8192)
MODEL_KEYS = tuple(f"rnd{M}" for M in RANDOM_M) + ("KR", "LuxC", "dna", "zero", "bg")
LENGTHS = (1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 50, 63, 64, 65, 66, 127, 128, 129, 130, 1000, 20000)
REPEAT_L = (17, 300, 5000)
CODE_POSITIONS = (1, 2, 16, 17)           # and L
CODE_L = 40
MANY = 70_000
SMALL_BLOCKS = (1, 63, 64, 65)
ZEROED = "WC"                             # the two residues the "zero" model never emits


def _zero_composition_model():
    hmm = random_hmm(60, seed=60)
    idx = [hmm.alphabet.symbols.index(c) for c in ZEROED]
    hmm.match_emissions[1:, idx] = 0.0           # row 0 of the match emissions is a convention, not a distribution
    hmm.insert_emissions[:, idx] = 0.0
    hmm.renormalize()
    hmm.set_composition()
    assert all(hmm.composition[i] == 0.0 for i in idx)
    return hmm


@functools.lru_cache(maxsize=None)
def model(key):
    """(hmm, background) of a key."""
    if key in ("KR", "LuxC"):
        hmm = load_hmms(key)[0]
    elif key == "dna":
        hmm = random_hmm(150, seed=77, alphabet=easel.Alphabet.dna())
    elif key == "zero":
        hmm = _zero_composition_model()
    elif key == "bg":
        hmm = random_hmm(120, seed=121)
    else:
        hmm = random_hmm(int(key[3:]), seed=int(key[3:]))
    bg = plan7.Background(hmm.alphabet)
    if key == "bg":            # frequencies between a third and three times the default's, renormalised in float32
        f = bg.residue_frequencies.astype(np.float64) * np.exp(np.random.default_rng(5).uniform(-1.1, 1.1, hmm.alphabet.K))
        bg.residue_frequencies = (f / f.sum()).astype(np.float32)
    return hmm, bg


def _rng(key, salt):
    return np.random.default_rng([sum(key.encode()), salt])


def _draw(rng, p, n):
    p = np.asarray(p, dtype=np.float64)
    return rng.choice(p.shape[0], size=n, p=p / p.sum()).astype(np.uint8)


def composition(key):
    """The profile's float32 composition (a model file without a COMPO line leaves it to the profile)."""
    return np.asarray(profile(key).compositions, dtype=np.float32)[:model(key)[0].alphabet.K]


def _odds(key):
    return composition(key).astype(np.float64) / model(key)[1].residue_frequencies.astype(np.float64)


@functools.lru_cache(maxsize=None)
def family_a(key):
    hmm, bg = model(key)
    rng = _rng(key, 1)
    out = [(f"len{L}", _draw(rng, bg.residue_frequencies, L)) for L in LENGTHS]
    empty = np.zeros(0, dtype=np.uint8)
    return out[:3] + [("empty1", empty)] + out[3:7] + [("empty2", empty)] + out[7:]


@functools.lru_cache(maxsize=None)
def family_b(key):
    hmm, bg = model(key)
    rng = _rng(key, 2)
    odds = _odds(key)
    order = np.argsort(odds, kind="stable")
    lo, hi, hi2 = int(order[0]), int(order[-1]), int(order[-2])
    out = [("background", _draw(rng, bg.residue_frequencies, 300)), ("composition", _draw(rng, composition(key) if composition(key).sum() > 0 else hmm.match_emissions[1:].mean(axis=0), 300))]
    for L in REPEAT_L:
        out += [(f"homopolymer_hi{L}", np.full(L, hi, dtype=np.uint8)), (f"homopolymer_lo{L}", np.full(L, lo, dtype=np.uint8)),
                (f"repeat_hi_lo{L}", np.resize(np.array([hi, lo], dtype=np.uint8), L)),
                (f"repeat_hi_hi2_{L}", np.resize(np.array([hi, hi2], dtype=np.uint8), L))]
    plain, biased = _draw(rng, bg.residue_frequencies, 300), np.resize(np.array([hi, hi2], dtype=np.uint8), 300)
    out += [("background_then_biased", np.concatenate([plain, biased])), ("biased_then_background", np.concatenate([biased, plain]))]
    return out


@functools.lru_cache(maxsize=None)
def family_c(key):
    hmm, bg = model(key)
    abc = hmm.alphabet
    rng = _rng(key, 3)
    out = []
    for x in range(abc.K, abc.Kp):
        seq = _draw(rng, bg.residue_frequencies, CODE_L)
        seq[[p - 1 for p in CODE_POSITIONS] + [CODE_L - 1]] = x
        out.append((f"code{x}", seq))
    out.append(("all_any", np.full(CODE_L, abc.Kp - 3, dtype=np.uint8)))
    return out


def targets(key, family):
    return {"a": family_a, "b": family_b, "c": family_c}[family](key)


FAMILIES = ("a", "b17", "b300", "b5000", "c", "d")      # what the measured figures are recorded by
HOST_D = 4096                                            # targets of family d the host engines are measured on


def label(family, seq):
    """Family b by length: a figure measured on the 5,000-residue repeats says nothing about a 17-residue one."""
    return family if family != "b" else "b17" if len(seq) <= 17 else "b5000" if len(seq) >= 5000 else "b300"


def scored(named):
    """Without the empty targets (nothing scores an empty sequence)."""
    return [(name, seq) for name, seq in named if len(seq)]


@functools.lru_cache(maxsize=None)
def family_d(key):
    """Packed block (dsq with Easel's sentinels, offsets, lengths) of MANY targets of 1-40 residues."""
    hmm, bg = model(key)
    abc = hmm.alphabet
    rng = _rng(key, 4)
    lengths = rng.integers(1, 41, size=MANY).astype(np.int32)
    offsets = (np.concatenate([[0], np.cumsum(lengths[:-1].astype(np.int64) + 1)]) + 1).astype(np.int64)
    dsq = np.full(int(lengths.sum()) + MANY + 1, 255, dtype=np.uint8)
    member = np.ones(dsq.shape[0], dtype=bool)
    member[offsets - 1] = False
    member[-1] = False
    res = _draw(rng, bg.residue_frequencies, int(lengths.sum()))
    owner = np.repeat(np.arange(MANY), lengths)
    swap = (owner % 8 == 0) & (rng.random(res.shape[0]) < 0.125)
    res[swap] = rng.integers(abc.K + 1, abc.Kp - 2, size=int(swap.sum())).astype(np.uint8)
    dsq[member] = res
    return dsq, offsets, lengths


@functools.lru_cache(maxsize=None)
def profile(key):
    hmm, bg = model(key)
    return plan7.OptimizedProfile(hmm, bg, 400)


@functools.lru_cache(maxsize=None)
def ref_model(key):
    import bias_reference as R
    return R.FilterModel.from_profile(profile(key), model(key)[1])


@functools.lru_cache(maxsize=None)
def reference(key, family):
    """The float64 reference of the scored targets of a family, computed once per session: [(name, seq, result)]."""
    import bias_reference as R
    return [(name, seq, R.filter_score(ref_model(key), seq)) for name, seq in scored(targets(key, family))]


@functools.lru_cache(maxsize=None)
def reference_d(key):
    """(filtersc[MANY], S[MANY]) of family d, vectorised by length."""
    import bias_reference as R
    return R.filter_scores_by_length(ref_model(key), *family_d(key))


def block(alphabet, named):
    return easel.DigitalSequenceBlock(alphabet, [easel.DigitalSequence(alphabet, name=name, sequence=np.asarray(seq, dtype=np.uint8))
                                                 for name, seq in named])


# ------------------------------------------------------------------------------------------------ the decision block
DECISION_N = 20_000
DECISION_SEED = 1
DECISION_KEYS = ("LuxC", "rnd262", "zero")
DECISION_PLANTS = ("LuxC", "LuxC", "rnd262", "zero")      # whose composition the planted stretches take, in turn


@functools.lru_cache(maxsize=None)
def decision_block(seed=DECISION_SEED):
    """Packed block of DECISION_N amino targets of 50-400 background residues; every third carries a stretch drawn from the
    composition of one of the DECISION_PLANTS models (in turn), 30-100 % of its length, so that the bias filter has MSV
    survivors to decide on both sides of F1."""
    rng = np.random.default_rng([77, seed])
    bgf = plan7.Background(easel.Alphabet.amino()).residue_frequencies
    lengths = rng.integers(50, 401, size=DECISION_N).astype(np.int32)
    offsets = (np.concatenate([[0], np.cumsum(lengths[:-1].astype(np.int64) + 1)]) + 1).astype(np.int64)
    dsq = np.full(int(lengths.sum()) + DECISION_N + 1, 255, dtype=np.uint8)
    for t in range(DECISION_N):
        L = int(lengths[t])
        seq = _draw(rng, bgf, L)
        if t % 3 == 0:
            compo = composition(DECISION_PLANTS[(t // 3) % len(DECISION_PLANTS)])
            n = int(rng.integers(3 * L // 10, L + 1))
            a = int(rng.integers(0, L - n + 1))
            seq[a:a + n] = _draw(rng, compo, n)
        dsq[offsets[t]:offsets[t] + L] = seq
    return dsq, offsets, lengths


def check_decisions(key, passed, usc, nullsc, who, E, F1):
    """passed[t] (the target went past the filter) against ln P <= ln F1, P in float64 from usc[t] and nullsc[i], for the
    targets who[i] outside the margin |ln P - ln F1| <= lambda E[i] / ln 2 (|d ln P / d score| <= lambda for the Gumbel
    tail; the score is in bits, E in nats).  Asserts every decision; returns (left out, went past, stopped)."""
    import bias_reference as R
    hmm = model(key)[0]
    mu, lam = float(hmm._evparam[0]), float(hmm._evparam[1])
    lnF1 = math.log(F1)
    left = npass = nfail = 0
    wrong = []
    for i, t in enumerate(who):
        lnp = R.ln_pvalue(usc[t], nullsc[i], mu, lam)
        if abs(lnp - lnF1) <= lam * E[i] / R.LN2:
            left += 1
            continue
        want = lnp <= lnF1
        npass, nfail = npass + want, nfail + (not want)
        if bool(passed[t]) != want:
            wrong.append((key, int(t), bool(passed[t]), lnp, lnF1))
    assert not wrong, wrong[:10]
    return left, npass, nfail
