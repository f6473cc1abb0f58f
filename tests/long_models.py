"""Models beyond 8,192 nodes (sequence queries of phmmer: one node per residue) -- lengths, models and targets shared by
tests/test_gpu_long_models.py and tests/test_host_long_models.py (test input only).

The wave-per-target kernels give lane z the nodes zC+1 .. zC+C; beyond C = 128 there is one more tier, 192 nodes per
lane (P7X_NODE_TIERS).  Targets stay short -- a test is about the layout, not about the size of a matrix: background
sequences of 1 ... 419 residues and FRAGMENTS of at most 400 residues cut from one emission of the model, placed on the
first lane, the last lane that holds nodes and the lane boundaries in between."""
import functools

import numpy as np

from conftest import random_hmm, synthetic_block
from pyhmmer_amd import _lib, easel, plan7

OLD_LIMIT = 8192
NEW_TIERS = (192,)                   # nodes per lane beyond 128, as P7X_NODE_TIERS lists them
FRAGMENT = 400                       # residues of a fragment, at most
SPACER = 30                          # residues between the two copies of the two-domain target


def limit() -> int:
    return int(_lib.lib().p7x_max_model_length())


def long_lengths():
    """The first model beyond the old limit, the last model of every new tier and the first of the next, and the limit."""
    lim = limit()
    out = {OLD_LIMIT + 1, lim}
    for c in NEW_TIERS:
        if 64 * c < lim:
            out |= {64 * c, 64 * c + 1}
    return sorted(m for m in out if OLD_LIMIT < m <= lim)


def nodes_per_lane(M: int) -> int:
    return next(c for c in (128,) + NEW_TIERS if 64 * c >= M)


def emit_with_nodes(hmm, rng):
    """One pass through the core model, node 1 -> M: the residues and the node that emitted each (match or insert)."""
    t = np.asarray(hmm.transition_probabilities, dtype=np.float64)
    mat = np.asarray(hmm.match_emissions, dtype=np.float64)
    ins = np.asarray(hmm.insert_emissions, dtype=np.float64)
    cmat = np.cumsum(mat / np.maximum(mat.sum(axis=1, keepdims=True), 1e-30), axis=1)
    cins = np.cumsum(ins / np.maximum(ins.sum(axis=1, keepdims=True), 1e-30), axis=1)
    M, K = hmm.M, hmm.alphabet.K
    u, v = rng.random(4 * M + 64), rng.random(4 * M + 64)
    res, node = [], []
    state, k, n = 0, 1, 0            # 0 = M, 1 = I, 2 = D
    while k <= M and n < len(u):
        if state == 0:
            res.append(min(int(np.searchsorted(cmat[k], v[n])), K - 1)); node.append(k)
            if k == M:
                break
            s3 = t[k, 0] + t[k, 1] + t[k, 2]
            state = 0 if u[n] * s3 < t[k, 0] else (1 if u[n] * s3 < t[k, 0] + t[k, 1] else 2)
            if state != 1:
                k += 1
        elif state == 1:
            res.append(min(int(np.searchsorted(cins[k], v[n])), K - 1)); node.append(k)
            if u[n] * (t[k, 3] + t[k, 4]) < t[k, 3]:
                state, k = 0, k + 1
        else:
            if k == M:
                break
            state = 0 if u[n] * (t[k, 5] + t[k, 6]) < t[k, 5] else 2
            k += 1
        n += 1
    return np.array(res, dtype=np.uint8), np.array(node, dtype=np.int32)


def fragment_windows(M: int):
    """(first node, last node) of six fragments: the first lane, the last lane that holds nodes, and windows that straddle
    the first, a middle and the last boundary between two lanes that hold nodes (and one more in the second lane)."""
    C = nodes_per_lane(M)
    nl = (M + C - 1) // C                           # lanes that hold nodes
    span = FRAGMENT - 40                            # nodes: inserts make a fragment a little longer than its window
    out = [(1, span), (M - span + 1, M)]
    for z in sorted({1, nl // 2, nl - 1}):
        lo = max(1, z * C - span // 2 + 1)          # nodes zC and zC + 1 are neighbours in different lanes
        out.append((lo, min(M, lo + span - 1)))
    out.append((C + 7, C + 7 + span - 1))
    return out[:6] if len(out) >= 6 else out + [(2 * C + 3, 2 * C + 3 + span - 1)] * (6 - len(out))


@functools.lru_cache(maxsize=None)
def case(M: int):
    """(hmm, background, emission, its nodes, [six fragments]) of the model of M nodes; computed once per session."""
    hmm = random_hmm(M, seed=12000 + M)
    bg = plan7.Background(hmm.alphabet)
    rng = np.random.default_rng([12, M])
    res, node = emit_with_nodes(hmm, rng)
    frags = []
    for lo, hi in fragment_windows(M):
        f = res[(node >= lo) & (node <= hi)][:FRAGMENT]
        assert 200 <= len(f) <= FRAGMENT, (M, lo, hi, len(f))
        f.setflags(write=False)
        frags.append(f)
    res.setflags(write=False)
    return hmm, bg, res, node, frags


def _seq(abc, name, arr):
    return easel.DigitalSequence(abc, name=name, sequence=np.ascontiguousarray(arr, dtype=np.uint8))


def filter_block(M: int, nrand: int = 90):
    """<nrand> background targets of 1 ... 419 residues and the six fragments (the block shape of
    test_gpu_filters.test_every_wavefront_kernel_instantiation_vs_oracle)."""
    hmm, bg, res, node, frags = case(M)
    abc = hmm.alphabet
    rng = np.random.default_rng([13, M])
    seqs = list(synthetic_block(nrand, 0, seed=M, alphabet=abc, lengths=rng.integers(1, 420, size=nrand)))
    seqs += [_seq(abc, f"frag{i}", f) for i, f in enumerate(frags)]
    return easel.DigitalSequenceBlock(abc, seqs)


TWO_WINDOWS = (170, 150, 90)         # the copies start this many nodes before the first lane boundary


def two_domain_targets(M: int):
    """Three targets "two0" .. "two2", each two copies of one fragment joined by a SPACER-residue spacer.  A fragment is
    the emission of 180 nodes across the first lane boundary; a repeat cannot be explained by one pass through the model, so
    the copies are two domains.  The spacer is what the SPACER nodes after the fragment emitted: with background residues
    there the posterior of being in the model falls below the region threshold and the target is two regions of one domain
    each.  Even so a region ends wherever one residue takes nearly all of a domain's end probability, which depends on the
    residues at the junction: of these three windows at least one keeps both copies in ONE region, which is then resolved
    by a traceback ensemble, at every length of long_lengths() (measured with tests/host_pipeline.py: one or two of three)."""
    hmm, bg, res, node, frags = case(M)
    out = []
    for j, back in enumerate(TWO_WINDOWS):
        lo = nodes_per_lane(M) - back
        a = res[(node >= lo) & (node < lo + 180)]
        spacer = res[(node >= lo + 180) & (node < lo + 180 + SPACER + 10)][:SPACER]
        assert len(spacer) == SPACER and 2 * len(a) + SPACER <= FRAGMENT + 60
        out.append(_seq(hmm.alphabet, f"two{j}", np.concatenate([a, spacer, a])))
    return out


def domain_block(M: int, nrand: int = 30):
    """The targets of the envelope tests: background, the six fragments with flanks, and the two-domain targets."""
    hmm, bg, res, node, frags = case(M)
    abc = hmm.alphabet
    rng = np.random.default_rng([15, M])
    seqs = list(synthetic_block(nrand, 0, seed=M + 1, alphabet=abc, lengths=rng.integers(20, 420, size=nrand)))
    for i, f in enumerate(frags):
        fl = rng.integers(0, abc.K, size=int(rng.integers(0, 20))).astype(np.uint8)
        seqs.append(_seq(abc, f"frag{i}", np.concatenate([fl, f[:FRAGMENT - 2 * len(fl)], fl])))
    seqs += two_domain_targets(M)
    return easel.DigitalSequenceBlock(abc, seqs)


def records(hits):
    """What tests/test_gpu_envelopes.py compares of a hit list: exact fields and float fields, hit by hit."""
    out = []
    for h in hits:
        doms = []
        for d in h.domains:
            a = d.alignment
            doms.append(((d.env_from, d.env_to, a.target_from, a.target_to, a.hmm_from, a.hmm_to, a.target_sequence,
                          a.hmm_sequence, a.identity_sequence, a.posterior_probabilities),
                         (d.score, d.bias, d.accuracy * 10.0)))
        out.append((h.name, (h.score, h.bias), doms))
    return out
