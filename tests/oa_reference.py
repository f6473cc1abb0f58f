"""Float64 optimal accuracy of a unihit local alignment (test infrastructure only): the best expected accuracy any trace of
the whole sequence can have, from the posteriors of tests/dp_reference.py.

The recurrence is p7_OptimalAccuracy's, with delta = 0 where a transition has probability > 0 and -inf elsewhere:

    M(i,k) = max(B(i-1) dBM, M(i-1,k-1) dMM, I(i-1,k-1) dIM, D(i-1,k-1) dDM) + ppM(i,k)
    I(i,k) = max(M(i-1,k) dMI, I(i-1,k) dII) + ppI(i,k)
    D(i,k) = max(M(i,k-1) dMD, D(i,k-1) dDD)
    E(i)   = max_k(M(i,k), D(i,k))
    C(i)   = max(C(i-1) + ppC(i), E(i))
    N(i)   = N(i-1) + ppN(i),  B(i) = N(i);  the result is C(L).

A trace's expected accuracy (the sum of its steps' posteriors) can reach this value and cannot exceed it."""
import numpy as np

NEG = -np.inf


def _gate(logt):
    """0 where the transition exists (its log is finite), -inf where it does not."""
    return np.where(np.isfinite(logt), 0.0, NEG)


def optimal_accuracy(model, ref):
    """C(L) for the RefModel <model> and the RefResult <ref> (computed with cells=True, unihit)."""
    m, M, L = model, model.M, ref.L
    ppM, ppI, ppN, _, ppC = ref.posteriors()
    g = {n: _gate(getattr(m, n)) for n in ("bm", "mm", "im", "dm", "md", "mi", "ii", "dd")}
    k = slice(1, M + 1)
    km1 = slice(0, M)
    Mp, Ip, Dp = (np.full(M + 2, NEG) for _ in range(3))
    N, C = 0.0, NEG
    for i in range(1, L + 1):
        Mc, Ic, Dc = (np.full(M + 2, NEG) for _ in range(3))
        best = np.maximum(np.maximum(N + g["bm"][k], Mp[km1] + g["mm"][k]), np.maximum(Ip[km1] + g["im"][k], Dp[km1] + g["dm"][k]))
        Mc[k] = best + ppM[i, k]
        Ic[k] = np.maximum(Mp[k] + g["mi"][k], Ip[k] + g["ii"][k]) + ppI[i, k]
        if m.dd_closed:                    # every D -> D is open: the chain is a running maximum
            Dc[2:M + 1] = np.maximum.accumulate(Mc[1:M] + g["md"][1:M])
        else:
            for kk in range(2, M + 1):
                Dc[kk] = max(Mc[kk - 1] + g["md"][kk - 1], Dc[kk - 1] + g["dd"][kk - 1])
        E = max(Mc[k].max(), Dc[k].max())
        C = max(C + ppC[i], E)
        N = N + ppN[i]
        Mp, Ip, Dp = Mc, Ic, Dc
    return float(C)
