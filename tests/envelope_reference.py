"""Float64 reference of what a search reports for one domain envelope (test infrastructure only): the unihit Forward score
of the envelope's residues under the whole target's length model, the null2 odds by expectation and their correction, the
optimal-accuracy score, and the domain's bit score, bias and accuracy as p7x_tophits.cpp::finish_one derives them.

Built on tests/dp_reference.py (Forward / Backward / posteriors in log space on the kernels' own float32 odds tables) and
tests/oa_reference.py.  null2 by expectation (p7_Null2_ByExpectation) in plain terms: over the envelope's Ld residues,

    occ[k]   = sum_i ppM[i, k] / Ld                      how often match state k emits a residue of the envelope
    rest     = sum_i (ppI[i, .] + ppN[i] + ppJ[i] + ppC[i]) / Ld   every other emitter; all of them emit with odds 1
    null2[x] = sum_k occ[k] odds(x | M_k) + rest         K canonical residues
    null2[d] = mean of null2 over the residues a degenerate code d stands for; gap, '*' and missing data: 1

Every residue of the envelope is emitted by exactly one state, so sum_k occ[k] + rest = 1 and, the match odds being
emission probability over background frequency, sum_x f(x) null2[x] = 1 (f the background) up to the float32 rounding of the
tables."""
import math
from types import SimpleNamespace

import numpy as np

import dp_reference as R
import oa_reference

LOG_OMEGA = math.log(1.0 / 256.0)                   # the prior of the null2 model (p7_pipeline.c: omega)
LN2 = math.log(2.0)


def null2_by_expectation(model, ref, degeneracy):
    """null2[Kp] from the posteriors of <ref> (unihit, cells=True) over its rows 1..Ld.  degeneracy: [Kp][K], the residues
    each code stands for (oracle_lib.degeneracy_sets)."""
    M, Ld = model.M, ref.L
    degeneracy = np.asarray(degeneracy, dtype=np.float64)
    K = degeneracy.shape[1]
    ppM, ppI, pN, pJ, pC = ref.posteriors()
    occ = ppM[1:, 1:M + 1].sum(axis=0) / Ld
    rest = (ppI[1:, 1:M + 1].sum() + pN[1:].sum() + pJ[1:].sum() + pC[1:].sum()) / Ld
    null2 = np.ones(model.Kp)
    null2[:K] = np.exp(model.e[:K, 1:M + 1]) @ occ + rest
    return finish_null2(null2, degeneracy)


def finish_null2(null2, degeneracy):
    """The degenerate codes of a null2 vector whose K canonical entries are set: the mean over the residues a code stands
    for; gap, '*' and missing data stay 1 (tests/ensemble_reference.py's null2 by trace ends the same way)."""
    degeneracy = np.asarray(degeneracy, dtype=np.float64)
    K = degeneracy.shape[1]
    for x in range(K, len(null2)):
        members = degeneracy[x] > 0
        null2[x] = null2[:K][members].mean() if members.any() else 1.0
    return null2


def null1(L):
    """p7_bg_SetLength + p7_bg_NullOne: p1 = L / (L + 1) is a float32, the logarithms are C's double log()."""
    p1 = float(np.float32(L) / np.float32(L + 1))
    return L * math.log(p1) + math.log(1.0 - p1)


FLOGSUM_STEPS = 1000.0          # p7_FLogsum: log(1 + exp(-d)) read from a table of 16,000 entries, d truncated to 1 / 1000 nat


def flogsum_index(a, b):
    d = abs(a - b)
    return None if d >= 15.7 else int(d * FLOGSUM_STEPS)


def flogsum(a, b):
    """p7_FLogsum(a, b) in float64: the table lookup is part of what a reported bias is."""
    idx = flogsum_index(a, b)
    return max(a, b) if idx is None or min(a, b) == -np.inf else max(a, b) + math.log(1.0 + math.exp(-idx / FLOGSUM_STEPS))


def dombias(domcorrection):
    return flogsum(0.0, LOG_OMEGA + domcorrection)


def dombias_reach(domcorrection, err):
    """How far dombias can move when domcorrection moves by at most <err> nats: the function rises with slope 0 or 1 between
    the table's steps (<err>), and jumps by the difference of two neighbouring table entries where log(1 / 256) +
    domcorrection crosses a multiple of 1 / 1000 nat -- the jumps inside the interval are added.  The interval is widened
    by a float32 ulp of the argument, which finish_one hands to p7_FLogsum as a float."""
    b = LOG_OMEGA + domcorrection
    w = err + 2.0 ** -22 * max(abs(b), 1.0)
    table = lambda i: math.log(1.0 + math.exp(-i / FLOGSUM_STEPS)) if i < 15700 else 0.0
    lo, hi = abs(b - w), abs(b + w)
    if (b - w) * (b + w) < 0.0:
        lo, hi = 0.0, max(lo, hi)
    i0, i1 = int(min(lo, hi) * FLOGSUM_STEPS), int(max(lo, hi) * FLOGSUM_STEPS)
    return err + (table(i0) - table(i1))


def envelope(model, seq, ienv, jenv, degeneracy):
    """The envelope ienv..jenv (1-based, inclusive) of the target <seq>.  Returns a namespace: envsc, domcorrection (nats),
    oasc, null2[Kp], and dombias (nats), bitscore (bits), accuracy as finish_one forms them."""
    seq = np.asarray(seq)
    L = len(seq)
    sub = seq[ienv - 1:jenv]
    Ld = len(sub)
    assert 1 <= ienv <= jenv <= L and Ld == jenv - ienv + 1
    ref = R.forward_backward(model, sub, False, cells=True, length=L)
    pp = ref.posteriors()
    ref.posteriors = lambda: pp                       # (the optimal-accuracy reference asks for them again)
    null2 = null2_by_expectation(model, ref, degeneracy)
    corr = math.fsum(math.log(null2[x]) for x in sub)
    oasc = oa_reference.optimal_accuracy(model, ref)
    bias = dombias(corr)
    length_term = (L - Ld) * math.log(float(np.float32(L) / np.float32(L + 3)))
    return SimpleNamespace(L=L, Ld=Ld, envsc=ref.fwd, bck=ref.bck, null2=null2, domcorrection=corr, oasc=oasc, dombias=bias,
                           bitscore=(ref.fwd + length_term - null1(L) - bias) / LN2, accuracy=oasc / Ld)
