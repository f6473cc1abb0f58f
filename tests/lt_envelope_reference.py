"""Float64 reference of what a long-target (nhmmer) search reports for one envelope (test infrastructure only): upstream
rescore_isolated_domain(long_target = TRUE) in plain terms, on tests/dp_reference.py (Forward / Backward / posteriors in log
space) and tests/oa_reference.py.

Over the envelope's Ld residues, unihit, under the length model of Ld itself:

    orig          = Forward with the profile's own odds (the kernels' float32 tables, as RefModel reads them)
    adj           = Forward with the odds of the adjusted background (below)
    domcorrection = max(0, orig - adj)                      the score lost to the envelope's own composition
    oasc          = optimal accuracy on the posteriors of the adjusted-odds Forward / Backward

The adjusted background and odds (p7x_domaindef.cpp::reparameterize, upstream reparameterize_model): with cnt[x] the number
of residues x in the envelope -- a degenerate code counting 1 / n for each of the n residues it stands for; gap, '*' and
missing data not at all --

    bgn[x]    = (1 - s) cnt[x] / sum(cnt) + s bg[x],        s = 25 / min(100, max(50, window length))
    e'[x, k]  = log(match_prob[k][x] / bgn[x])              x < K
    e'[d, k]  = sum_{x in d} bgn[x] e'[x, k] / sum_{x in d} bgn[x]      a degenerate code d: the expected score under bgn
    e'[gap], e'['*'], e'[missing] = -inf

all of it in float64 from the model's float32 match probabilities and background frequencies: the float32 rounding of the
product's table (the product of odds and background that stands for the match probability, logf, expf) is part of the distance
that gets measured, not of the reference.

The reported numbers follow p7x_longtarget_host.cpp::lt_window_hits in float64 (reported()): what the envelope's own length
model charged for entering, leaving and the flanks is taken out, the score re-expressed for a window of max_length, the null
model is that of the same span, and the bias is domcorrection itself (no omega prior)."""
import copy
import math
from types import SimpleNamespace

import numpy as np

import dp_reference as R
import oa_reference

LN2 = math.log(2.0)
NEG = -np.inf


def smoothing(window_length):
    return 25.0 / min(100, max(50, int(window_length)))


def composition_counts(sub, degeneracy):
    """cnt[K] over the residues <sub>: canonical residues 1, degenerate codes 1 / n to each member, the rest nothing."""
    degeneracy = np.asarray(degeneracy, dtype=np.float64)
    Kp, K = degeneracy.shape
    cnt = np.zeros(K)
    for x in np.asarray(sub, dtype=np.int64):
        if x < K:
            cnt[x] += 1.0
        elif K < x <= Kp - 3:
            cnt += degeneracy[x] / degeneracy[x].sum()
    return cnt


def adjusted_background(sub, bg, degeneracy, s):
    bg = np.asarray(bg, dtype=np.float64)
    cnt = composition_counts(sub, degeneracy)
    tot = cnt.sum()
    return (1.0 - s) * (cnt / tot if tot > 0 else bg) + s * bg


def adjusted_emissions(match_prob, bgn, degeneracy):
    """e'[Kp, M + 2] (natural logs; columns 0 and M + 1 are -inf) from match_prob[M + 1, K] (row 0 unused) and bgn[K]."""
    degeneracy = np.asarray(degeneracy, dtype=np.float64)
    Kp, K = degeneracy.shape
    mp = np.asarray(match_prob, dtype=np.float64)
    M = mp.shape[0] - 1
    e = np.full((Kp, M + 2), NEG)
    with np.errstate(divide="ignore"):
        e[:K, 1:M + 1] = np.log(mp[1:, :] / bgn[None, :]).T
    for x in range(K + 1, Kp - 2):
        w = degeneracy[x] * bgn
        with np.errstate(invalid="ignore"):                     # (a zero match probability: 0 * -inf; none of the models here)
            e[x, 1:M + 1] = (w[:, None] * e[:K, 1:M + 1]).sum(axis=0) / w.sum()
    return e


def with_emissions(model, e):
    """The RefModel <model> with its match odds replaced by the logs e[Kp, M + 2]."""
    m = copy.copy(model)
    m.e = np.asarray(e, dtype=np.float64)
    assert m.e.shape == model.e.shape
    return m


def reported(orig, domcorrection, env_len, ali_len, max_length):
    """(bit score, bias in bits) of lt_window_hits from the envelope's score and correction in nats.  The two loop
    probabilities are the float32 quotients the product forms; everything else float64."""
    span = max(max_length, env_len)
    loop_env = float(np.float32(env_len) / np.float32(env_len + 2))
    loop_max = float(np.float32(max_length) / np.float32(max_length + 2))
    sc = orig - (2.0 * math.log(2.0 / (env_len + 2)) + (env_len - ali_len) * math.log(loop_env))
    sc += 2.0 * math.log(2.0 / (max_length + 2)) + (span - ali_len) * math.log(loop_max)
    p1 = float(np.float32(span) / np.float32(span + 1))                     # p7_bg_SetLength + p7_bg_NullOne
    nullsc = span * math.log(p1) + math.log(1.0 - p1)
    return (sc - (nullsc + domcorrection)) / LN2, domcorrection / LN2


def envelope(model, match_prob, bg, sub, degeneracy, s=0.25):
    """The envelope whose residues are <sub> (on its own strand).  model: the RefModel of the profile; match_prob[M + 1, K],
    bg[K]: the model's float32 match probabilities and background.  Returns a namespace: Ld, orig, adj, domcorrection (nats),
    oasc, bgn[K]."""
    sub = np.asarray(sub)
    Ld = len(sub)
    assert Ld >= 1
    orig = R.forward_backward(model, sub, False, backward=False).fwd
    bgn = adjusted_background(sub, bg, degeneracy, s)
    madj = with_emissions(model, adjusted_emissions(match_prob, bgn, degeneracy))
    ref = R.forward_backward(madj, sub, False, cells=True)
    pp = ref.posteriors()
    ref.posteriors = lambda: pp                       # (the optimal-accuracy reference asks for them again)
    oasc = oa_reference.optimal_accuracy(madj, ref)
    return SimpleNamespace(Ld=Ld, orig=orig, adj=ref.fwd, bck=ref.bck, domcorrection=max(0.0, orig - ref.fwd), oasc=oasc, bgn=bgn,
                           accuracy=oasc / Ld)
