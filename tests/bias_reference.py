"""Float64 reference of the bias filter's null score (test infrastructure only): p7_bg_SetFilter + p7_bg_SetLength +
esl_hmm_Forward + p7_bg_FilterScore, written from upstream's definition in plain numpy / Python floats.  It shares no code
with bias_kernel (p7x_pipeline.hip), bias_filter_score (p7x_domaindef.cpp) or oracle/p7_oracle.c.

The filter model is a two-state HMM over the target's residues:

    state 0  the background: emits x with odds 1, stays with p1 = L / (L + 1), moves to state 1 with 1 - p1
    state 1  the model's composition: emits x with odds compo[x] / bgf[x], stays with L1 / (L1 + 1), L1 = M / 8, goes back
             to state 0 with 1 / (L1 + 1)
    start    0.999 in state 0, 0.001 in state 1;  either state ends with probability 1 (the length is scored outside)

    filtersc = ln Forward(x_1 .. x_L) + L ln p1 + ln(1 - p1)

The parameters and the table of emission odds are the float32 values upstream stores (p1, 1 - p1, the two transitions of
state 1, 0.999f / 0.001f, and the quotients compo / bgf of the profile's float32 composition and the background's float32
frequencies; for a degenerate code the quotient of the two float32 sums over the residues it stands for; 1 for the gap,
'*' and missing-data codes).  Everything after these inputs is float64: the recurrence, normalised at every residue, the
logarithms, and the two length terms."""
import itertools
import math
from types import SimpleNamespace

import numpy as np

LN2 = math.log(2.0)
# the canonical residues a degenerate code stands for (Easel's standard alphabets)
DEGENERATE = {
    "amino": {"B": "ND", "J": "IL", "Z": "QE", "O": "K", "U": "C", "X": "ACDEFGHIKLMNPQRSTVWY"},
    "nucleic": {"R": "AG", "Y": "CT", "M": "AC", "K": "GT", "S": "CG", "W": "AT", "H": "ACT", "B": "CGT", "V": "ACG", "D": "AGT",
                "N": "ACGT"},
}


class FilterModel:
    """The parameters of the filter HMM of one profile: M nodes, composition compo[K], background bgf[K] (both float32)."""

    def __init__(self, alphabet, M, compo, bgf):
        f32 = np.float32
        compo, bgf = np.asarray(compo, dtype=f32), np.asarray(bgf, dtype=f32)
        K, Kp = alphabet.K, alphabet.Kp
        assert compo.shape == (K,) and bgf.shape == (K,)
        self.alphabet, self.M, self.K, self.Kp = alphabet, int(M), K, Kp
        odds = np.ones(Kp, dtype=f32)                                # gap, '*', '~': 1
        odds[:K] = compo / bgf
        sets = DEGENERATE["amino" if K == 20 else "nucleic"]
        canon = alphabet.symbols[:K].replace("U", "T")
        for x in range(K + 1, Kp - 2):
            members = [canon.index(c) for c in sets[alphabet.symbols[x]]]
            num = den = f32(0.0)
            for y in sorted(members):
                num, den = f32(num + compo[y]), f32(den + bgf[y])
            odds[x] = f32(num / den)
        self.odds = odds.astype(np.float64)
        L1 = f32(f32(M) / f32(8.0))                                  # M / 8 is exact in float32 for every M < 2^24
        self.t10 = float(f32(1.0) / f32(L1 + f32(1.0)))
        self.t11 = float(L1 / f32(L1 + f32(1.0)))
        self.pi = (float(f32(0.999)), float(f32(0.001)))

    @classmethod
    def from_profile(cls, om, background):
        """From an OptimizedProfile (its float32 compositions) and the Background it was built with."""
        return cls(om.alphabet, om.M, np.asarray(om.compositions, dtype=np.float32)[:om.alphabet.K], background.residue_frequencies)

    def length(self, L):
        """(p1, 1 - p1) of a target of L residues, as float32 forms them."""
        p1 = np.float32(L) / np.float32(L + 1)
        return float(p1), float(np.float32(1.0) - p1)


def filter_score(model, seq):
    """One target: filtersc (nats), forward (ln Forward alone) and S, the largest absolute partial sum of the log terms in
    the order a running sum takes them (one term per residue, the end term, then the two length terms)."""
    L = len(seq)
    assert L >= 1, "the filter HMM scores no empty sequence"
    odds = model.odds
    t00, t01 = model.length(L)
    t10, t11 = model.t10, model.t11
    x = int(seq[0])
    f0, f1 = model.pi[0], model.pi[1] * odds[x]
    total = S = 0.0
    for i in range(L):
        if i:
            e = odds[int(seq[i])]
            f0, f1 = f0 * t00 + f1 * t10, (f0 * t01 + f1 * t11) * e
        top = f0 if f0 >= f1 else f1
        f0, f1 = f0 / top, f1 / top
        total += math.log(top)
        S = max(S, abs(total))
    total += math.log(f0 + f1)
    S = max(S, abs(total))
    forward = total
    total += L * math.log(t00)
    S = max(S, abs(total))
    total += math.log(1.0 - t00)
    S = max(S, abs(total))
    return SimpleNamespace(filtersc=total, forward=forward, S=S, L=L)


def filter_scores_by_length(model, dsq, offsets, lengths):
    """A packed block (dsq[offsets[t] : offsets[t] + lengths[t]] the residues of target t, every length >= 1): the same
    recurrence for all targets of one length at a time, vectorised over the targets.  Returns (filtersc[n], S[n])."""
    dsq, offsets, lengths = np.asarray(dsq), np.asarray(offsets, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    n = lengths.shape[0]
    out, outS = np.empty(n), np.empty(n)
    for L in np.unique(lengths):
        L = int(L)
        assert L >= 1
        who = np.nonzero(lengths == L)[0]
        res = dsq[offsets[who][:, None] + np.arange(L)[None, :]]
        e = model.odds[res]
        t00, t01 = model.length(L)
        f0 = np.full(who.shape[0], model.pi[0])
        f1 = model.pi[1] * e[:, 0]
        total, S = np.zeros(who.shape[0]), np.zeros(who.shape[0])
        for i in range(L):
            if i:
                f0, f1 = f0 * t00 + f1 * model.t10, (f0 * t01 + f1 * model.t11) * e[:, i]
            top = np.maximum(f0, f1)
            f0, f1 = f0 / top, f1 / top
            total = total + np.log(top)
            S = np.maximum(S, np.abs(total))
        for term in (np.log(f0 + f1), np.full_like(total, L * math.log(t00)), np.full_like(total, math.log(1.0 - t00))):
            total = total + term
            S = np.maximum(S, np.abs(total))
        out[who], outS[who] = total, S
    return out, outS


def enumerate_paths(model, seq):
    """ln of the sum over all 2^L state paths of the path's probability x odds (written as a walk over the paths, not as the
    recursion): what filter_score calls forward."""
    L = len(seq)
    assert 1 <= L <= 16
    t00, t01 = model.length(L)
    t = ((t00, t01), (model.t10, model.t11))
    terms = []
    for path in itertools.product((0, 1), repeat=L):
        p = model.pi[path[0]]
        for i, s in enumerate(path):
            if i:
                p *= t[path[i - 1]][s]
            if s == 1:
                p *= model.odds[int(seq[i])]
        terms.append(p)                         # the end transition of either state is 1
    return math.log(math.fsum(terms))


def gumbel_ln_survival(x, mu, lam):
    """ln P(S > x) of a Gumbel(mu, lambda): P = 1 - exp(-exp(-lambda (x - mu))), through expm1 (no cancellation in the tail)."""
    return math.log(-math.expm1(-math.exp(-lam * (x - mu))))


def ln_pvalue(usc, filtersc, mu, lam):
    """ln of the P-value the pipeline compares with F1: the Gumbel survival of (usc - filtersc) / ln 2 bits, in float64."""
    if math.isinf(usc):
        return -math.inf                        # the MSV score overflowed: P = 0, the target passes
    return gumbel_ln_survival((float(usc) - float(filtersc)) / LN2, float(mu), float(lam))
