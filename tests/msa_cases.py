"""Helpers of the build_msa tests: small constructed alignments and a numpy float64 restatement of the builder's
procedure (relative weights, consensus columns, weighted counts, priors, effective sequence number, parameters), written
from the procedure alone -- it shares no code with the library, works row by row in plain loops, and sums in float64
where the library sums fixed-point integers."""
import math

import numpy as np

from pyhmmer_amd import easel

K, GAP, MISSING = 20, 20, 28
UNIT = 2.0 ** -40                    # the library's fixed-point unit

DEGEN = {21: (2, 11), 22: (7, 9), 23: (3, 13), 24: (8,), 25: (1,), 26: tuple(range(20))}      # B J Z O U X

T_PRIOR = np.array([0.7939, 0.0278, 0.0135, 0.1551, 0.1331, 0.9002, 0.5630])
MIX_Q = np.array([0.178091, 0.056591, 0.0960191, 0.0781233, 0.0834977, 0.0904123, 0.114468, 0.0682132, 0.234585])
MIX_ALPHA = np.array([float(x) for x in """
0.270671 0.039848 0.017576 0.016415 0.014268 0.131916 0.012391 0.022599 0.020358 0.030727 0.015315 0.048298 0.053803 0.020662 0.023612 0.216147 0.147226 0.065438 0.003758 0.009621
0.021465 0.010300 0.011741 0.010883 0.385651 0.016416 0.076196 0.035329 0.013921 0.093517 0.022034 0.028593 0.013086 0.023011 0.018866 0.029156 0.018153 0.036100 0.071770 0.419641
0.561459 0.045448 0.438366 0.764167 0.087364 0.259114 0.214940 0.145928 0.762204 0.247320 0.118662 0.441564 0.174822 0.530840 0.465529 0.583402 0.445586 0.227050 0.029510 0.121090
0.070143 0.011140 0.019479 0.094657 0.013162 0.048038 0.077000 0.032939 0.576639 0.072293 0.028240 0.080372 0.037661 0.185037 0.506783 0.073732 0.071587 0.042532 0.011254 0.028723
0.041103 0.014794 0.005610 0.010216 0.153602 0.007797 0.007175 0.299635 0.010849 0.999446 0.210189 0.006127 0.013021 0.019798 0.014509 0.012049 0.035799 0.180085 0.012744 0.026466
0.115607 0.037381 0.012414 0.018179 0.051778 0.017255 0.004911 0.796882 0.017074 0.285858 0.075811 0.014548 0.015092 0.011382 0.012696 0.027535 0.088333 0.944340 0.004373 0.016741
0.093461 0.004737 0.387252 0.347841 0.010822 0.105877 0.049776 0.014963 0.094276 0.027761 0.010040 0.187869 0.050018 0.110039 0.038668 0.119471 0.065802 0.025430 0.003215 0.018742
0.452171 0.114613 0.062460 0.115702 0.284246 0.140204 0.100358 0.550230 0.143995 0.700649 0.276580 0.118569 0.097470 0.126673 0.143634 0.278983 0.358482 0.661750 0.061533 0.199373
0.005193 0.004039 0.006722 0.006121 0.003468 0.016931 0.003647 0.002184 0.005019 0.005990 0.001473 0.004158 0.009055 0.003630 0.006583 0.003172 0.003690 0.002967 0.002772 0.002686
""".split()]).reshape(9, 20)

AMINO = easel.Alphabet.amino()


def msa_of(rows, name="case", rf=None, names=None):
    """A DigitalMSA of text rows (``-`` / ``.`` gaps)."""
    names = names or [f"s{i}" for i in range(len(rows))]
    msa = easel.DigitalMSA._from_rows(names, rows, [""] * len(rows), [""] * len(rows), rf=rf, alphabet=AMINO)
    msa.name = name
    return msa


def random_rows(n, alen, seed, gap=0.25, ends_consensus=True):
    """n text rows of alen columns: residues with a share of gaps, some gap-rich columns, a few degenerate residues."""
    rng = np.random.default_rng(seed)
    colgap = np.where(rng.random(alen) < 0.3, 0.8, gap * rng.random(alen))
    for c in (0, alen - 1):
        colgap[c] = 0.0 if ends_consensus else 0.95
    sym = np.array(list("ACDEFGHIKLMNPQRSTVWY"))
    res = sym[rng.integers(0, 6, size=(n, alen)) * 3 % 20]
    odd = rng.random((n, alen)) < 0.02
    res[odd] = np.array(list("BXZ"))[rng.integers(0, 3, size=int(odd.sum()))]
    gaps = rng.random((n, alen)) < colgap
    res[gaps] = "-"
    if not ends_consensus:                       # only the first row has a residue in the first and the last column
        res[:, 0] = res[:, alen - 1] = "-"
        res[0, 0] = res[0, alen - 1] = "A"
    if not (res[0] != "-").any():
        res[0, alen // 2] = "A"
    return ["".join(r) for r in res]


def is_res(a):
    return (a < K) | ((a > K) & (a <= 26))


def mark_fragments(ax, fragthresh):
    """Step 2: the cells outside a fragment's span become MISSING; returns the copy and the fragment flags."""
    ax = ax.copy()
    n, alen = ax.shape
    frag = np.zeros(n, dtype=bool)
    for i in range(n):
        cols = np.nonzero(is_res(ax[i]))[0]
        if cols.size == 0:
            continue
        first, last = int(cols[0]), int(cols[-1])
        if (last - first + 1) / alen < fragthresh:
            frag[i] = True
            ax[i, :first] = MISSING
            ax[i, last + 1:] = MISSING
    return ax, frag


def pb_weights(ax, symfrac, rf_cols=None, weighting="pb"):
    """Step 3: relative weights, sum N; also the weighting columns."""
    n, alen = ax.shape
    if weighting == "none":
        return np.ones(n), np.arange(alen)
    if rf_cols is not None:
        cols = np.asarray(rf_cols)
    else:
        nres = is_res(ax).sum(axis=0)
        ngap = (ax == GAP).sum(axis=0)
        cols = np.nonzero((nres + ngap > 0) & (nres >= symfrac * (nres + ngap)))[0]
    if cols.size == 0:
        cols = np.arange(alen)
    w = np.zeros(n)
    rlen = np.zeros(n)
    for c in cols:
        col = ax[:, c]
        cnt = np.bincount(col[col < K], minlength=K)
        r = int((cnt > 0).sum())
        for i in range(n):
            if col[i] < K:
                w[i] += 1.0 / (r * cnt[col[i]])
        rlen += is_res(col)
    w = np.where(rlen > 0, w / np.maximum(rlen, 1), 0.0)
    if w.sum() <= 0:
        return np.ones(n), cols
    return w * n / w.sum(), cols


def consensus_columns(ax, w, symfrac):
    """Step 4 ("fast"): weighted residue occupancy of at least symfrac."""
    r = (is_res(ax) * w[:, None]).sum(axis=0)
    g = ((ax == GAP) * w[:, None]).sum(axis=0)
    return np.nonzero((r > 0) & (r >= symfrac * (r + g)))[0]


def row_path(row, frag, cons):
    """One row as a path through the consensus columns: a list of (node, state, residue codes) where the states are "M",
    "D", "I" and "X" (missing); B and E are nodes 0 and M + 1, state "M" (or "X" for a fragment).  A delete next to an
    insert takes the neighbouring inserted residue and becomes a match: the one before it if there is one, else the one
    after it (Plan 7 has no D->I or I->D transition)."""
    M = len(cons)
    bounds = [-1] + [int(c) for c in cons] + [len(row)]
    path = [[0, "X" if frag else "M", None]]
    for k in range(M + 1):
        for c in range(bounds[k] + 1, bounds[k + 1]):
            if is_res(row[c]):
                path.append([k, "I", int(row[c])])
        if k < M:
            a = row[bounds[k + 1]]
            path.append([k + 1, "M" if is_res(a) else ("D" if a == GAP else "X"), int(a) if is_res(a) else None])
    path.append([M + 1, "X" if frag else "M", None])
    out = []
    i = 0
    while i < len(path):
        cur = path[i]
        nxt = path[i + 1] if i + 1 < len(path) else None
        if cur[1] == "D" and nxt is not None and nxt[1] == "I":
            out.append([cur[0], "M", nxt[2]])
            i += 2
        elif cur[1] == "I" and nxt is not None and nxt[1] == "D":
            out.append([nxt[0], "M", cur[2]])
            i += 2
        else:
            out.append(cur)
            i += 1
    return out


def counts(ax, frag, w, cons):
    """Step 5: weighted emission counts mat[M+1][20] and transition counts t[M+1][7] (MM MI MD IM II DM DD)."""
    M = len(cons)
    mat = np.zeros((M + 1, K))
    t = np.zeros((M + 1, 7))
    slot = {("M", "M"): 0, ("M", "I"): 1, ("M", "D"): 2, ("I", "M"): 3, ("I", "I"): 4, ("D", "M"): 5, ("D", "D"): 6}
    for i in range(ax.shape[0]):
        path = row_path(ax[i], bool(frag[i]), cons)
        for node, st, a in path:
            if st == "M" and a is not None:
                if a < K:
                    mat[node, a] += w[i]
                else:
                    for b in DEGEN[a]:
                        mat[node, b] += w[i] / len(DEGEN[a])
        # the steps between consecutive nodes, with the inserted residues between them; nothing is counted for a step
        # either end of which is missing
        main = [j for j, p in enumerate(path) if p[1] != "I"]
        for j1, j2 in zip(main[:-1], main[1:]):
            (k1, s1, _), (_, s2, _) = path[j1], path[j2]
            nins = j2 - j1 - 1
            if s1 == "X" or s2 == "X":
                continue
            if nins == 0:
                t[k1, slot[(s1, s2)]] += w[i]
            else:
                t[k1, slot[(s1, "I")]] += w[i]
                t[k1, 4] += (nins - 1) * w[i]
                t[k1, slot[("I", s2)]] += w[i]
    return mat, t


def insert_lengths(ax, frag, cons):
    """[N][M+1]: the inserted residues of every row after every node (after a delete has taken its neighbour's)."""
    out = np.zeros((ax.shape[0], len(cons) + 1), dtype=np.int64)
    for i in range(ax.shape[0]):
        for node, st, _ in row_path(ax[i], bool(frag[i]), cons):
            if st == "I":
                out[i, node] += 1
    return out


def emission_posterior(c, prior="alphabet"):
    """Step 6: the posterior mean emission distribution of one count vector."""
    if prior == "laplace":
        return (c + 1.0) / (c.sum() + K)
    logp = np.empty(9)
    for q in range(9):
        a = MIX_ALPHA[q]
        logp[q] = (math.log(MIX_Q[q]) + math.lgamma(a.sum()) - math.lgamma(c.sum() + a.sum())
                   + sum(math.lgamma(c[x] + a[x]) - math.lgamma(a[x]) for x in range(K)))
    p = np.exp(logp - logp.max())
    p /= p.sum()
    return sum(p[q] * (c + MIX_ALPHA[q]) / (c.sum() + MIX_ALPHA[q].sum()) for q in range(9))


def relent(mat, bgf, prior="alphabet"):
    """Mean match relative entropy (bits) of the emissions parameterised from the counts mat[1..M]."""
    tot = 0.0
    for k in range(1, mat.shape[0]):
        p = emission_posterior(mat[k], prior)
        tot += float((p * np.log2(p / bgf)).sum())
    return tot / (mat.shape[0] - 1)


def entropy_target(M, ere=0.59, esigma=45.0):
    return max(ere, (esigma + math.log2(M * (M + 1) / 2.0)) / M)


def effective_number(mat, n, bgf, target, prior="alphabet", want_bracket=False):
    """Step 7: N when the model at N holds no more than the target; else the k-th bisection midpoint on [0, N]."""
    if relent(mat, bgf, prior) <= target:
        return (float(n), (float(n), float(n))) if want_bracket else float(n)
    lo, hi, mid = 0.0, float(n), 0.0
    k = 1
    while n / 2.0 ** k >= 0.005:
        k += 1
    for _ in range(k):
        mid = 0.5 * (lo + hi)
        if relent(mat * (mid / n), bgf, prior) > target:
            hi = mid
        else:
            lo = mid
    return (mid, (lo, hi)) if want_bracket else mid


def parameterize(mat, t, neff, n, bgf, prior="alphabet"):
    """Step 8: probabilities (float64) t[M+1][7], mat[M+1][20], ins[M+1][20]."""
    M = mat.shape[0] - 1
    s = neff / n
    pm = np.zeros((M + 1, K))
    pm[0, 0] = 1.0
    for k in range(1, M + 1):
        pm[k] = emission_posterior(mat[k] * s, prior)
    alpha = T_PRIOR if prior == "alphabet" else np.ones(7)
    pt = t * s + alpha
    for lo, hi in ((0, 3), (3, 5), (5, 7)):
        pt[:, lo:hi] /= pt[:, lo:hi].sum(axis=1, keepdims=True)
    pt[M, 2] = 0.0
    pt[M, 0:2] /= pt[M, 0:2].sum()
    pt[M, 5:7] = (1.0, 0.0)
    pt[0, 5:7] = (1.0, 0.0)
    return pt, pm, np.tile(bgf, (M + 1, 1))


def build(ax, bgf, symfrac=0.5, fragthresh=0.5, weighting="pb", rf_cols=None, prior="alphabet", effective="entropy",
          ere=0.59, esigma=45.0):
    """The whole restatement: a dict of every intermediate."""
    bgf = np.asarray(bgf, dtype=np.float64)
    n = ax.shape[0]
    marked, frag = mark_fragments(ax, fragthresh)
    w, wcols = pb_weights(marked, symfrac, rf_cols, weighting)
    cons = np.asarray(rf_cols) if rf_cols is not None else consensus_columns(marked, w, symfrac)
    mat, t = counts(marked, frag, w, cons)
    M = len(cons)
    if effective == "entropy":
        neff = effective_number(mat, n, bgf, entropy_target(M, ere, esigma), prior)
    elif effective == "none":
        neff = float(n)
    else:
        neff = float(effective)
    pt, pm, pi = parameterize(mat, t, neff, n, bgf, prior)
    return dict(weights=w, weight_columns=wcols, consensus=cons, mat=mat, t=t, neff=neff, pt=pt, pm=pm, pi=pi, frag=frag)


def checksum(ax):
    """Step 1: Jenkins one-at-a-time over the digital codes, row after row."""
    v = 0
    for x in ax.reshape(-1).tolist():
        v = (v + x) & 0xffffffff
        v = (v + (v << 10)) & 0xffffffff
        v ^= v >> 6
    v = (v + (v << 3)) & 0xffffffff
    v ^= v >> 11
    v = (v + (v << 15)) & 0xffffffff
    return v
