"""Float64, log-space reference of local Plan-7 Forward / Backward / posterior decoding (test infrastructure only).

It reads the optimized profile's own float32 odds tables (the product's `OptimizedProfile.rfv` / `.tfv` or the oracle's
`arr("rfv")` / `arr("tfv")`: striped, node k = z Q + q + 1 at vector q, lane z), turns them once into float64 logarithms (a
zero odds ratio becomes -inf) and evaluates the recursions with `np.logaddexp`.  Nothing is rescaled, so there are no scale
factors to leave behind and nothing can overflow: what the float32 engines get from their scaled rows is compared with this.

The N / J / C loop and move probabilities are the float32 constants the engines form from the target length
(pmove = (2 + nj) / (L + 2 + nj), ploop = 1 - pmove, nj = 1 multihit, 0 unihit); E -> C / E -> J are 0.5 / 0.5 or 1 / 0.

The D -> D chain of a row has no loop over nodes: with P[k] = sum of log tDD below node k, D_k = P[k] + the running
logaddexp of (M_j + tMD_j - P[j + 1]), j < k (and its mirror image in Backward).  A model with a zero D -> D (none of the
models here; node M has no D -> D, which the chain never uses) takes a plain loop."""
import numpy as np

NEG = -np.inf
lae = np.logaddexp


def _log(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.log(a)


class RefModel:
    """Un-striped float64 logs of the tables.  e[x, k], k = 1..M (column 0 is -inf); bm mm im dm enter node k, md mi ii dd
    leave node k (index 0 and M + 1 are -inf padding)."""

    def __init__(self, M, rfv, tfv):
        rfv = np.asarray(rfv, dtype=np.float32)
        tfv = np.asarray(tfv, dtype=np.float32).reshape(-1, 4)
        Q = rfv.shape[1] // 4
        assert tfv.shape[0] == 8 * Q and Q * 4 >= M
        k = np.arange(1, M + 1)
        q, z = (k - 1) % Q, (k - 1) // Q
        self.M, self.Kp = M, rfv.shape[0]
        self.e = np.full((self.Kp, M + 2), NEG)
        self.e[:, 1:M + 1] = _log(rfv.reshape(self.Kp, Q, 4)[:, q, z])
        names = ("bm", "mm", "im", "dm", "md", "mi", "ii")
        for s, name in enumerate(names):
            t = np.full(M + 2, NEG)
            t[1:M + 1] = _log(tfv[7 * q + s, z])
            setattr(self, name, t)
        self.dd = np.full(M + 2, NEG)
        self.dd[1:M + 1] = _log(tfv[7 * Q + q, z])
        # D -> D prefix sums: P[k] = sum_{l < k} log dd[l], k = 1..M
        chain = self.dd[1:M]
        self.dd_closed = bool(np.isfinite(chain).all())
        self.P = np.zeros(M + 2)
        if self.dd_closed:
            self.P[2:M + 1] = np.cumsum(chain)

    @classmethod
    def from_oprofile(cls, om):
        return cls(om.M, om.rfv, om.tfv)

    @classmethod
    def from_oracle(cls, op):
        return cls(op.p.M, op.arr("rfv"), op.arr("tfv"))

    def tables(self):
        return np.concatenate([self.e.ravel()] + [getattr(self, n) for n in ("bm", "mm", "im", "dm", "md", "mi", "ii", "dd")])


def length_model(L, multihit):
    """(log ploop, log pmove, log E->C, log E->J) from the engines' float32 constants."""
    nj = np.float32(1.0 if multihit else 0.0)
    pmove = (np.float32(2.0) + nj) / (np.float32(L) + np.float32(2.0) + nj)
    ploop = np.float32(1.0) - pmove
    assert pmove.dtype == np.float32 and ploop.dtype == np.float32
    emove, eloop = (0.5, 0.5) if multihit else (1.0, 0.0)
    return tuple(float(v) for v in _log([ploop, pmove, emove, eloop]))


class RefResult:
    """fwd / bck: totals in nats.  fx / bx: (L + 1) x 5 logs of E N J B C per row (the oracle's column order).  With
    cells: fM fI fD bM bI bD (L + 1) x (M + 2) logs, from which the posteriors come (fD / bD: the delete cells, which emit nothing
    and have no part in posteriors(); tests/ensemble_reference.py states the traceback choices from them)."""

    def posteriors(self):
        """ppM, ppI: (L + 1) x (M + 2); ppN, ppJ, ppC: (L + 1), the probability that residue i is emitted there."""
        tot = self.fwd
        ppM = np.exp(self.fM + self.bM - tot)
        ppI = np.exp(self.fI + self.bI - tot)
        L = self.L
        pn = np.zeros((3, L + 1))
        for c, col in enumerate((1, 2, 4)):
            pn[c, 1:] = np.exp(self.fx[:-1, col] + self.loop + self.bx[1:, col] - tot)
        return ppM, ppI, pn[0], pn[1], pn[2]

    def domain_decoding(self):
        """btot, etot, mocc of p7_DomainDecoding (rows 0..L)."""
        tot, L = self.fwd, self.L
        btot, etot, mocc = np.zeros(L + 1), np.zeros(L + 1), np.zeros(L + 1)
        btot[1:] = np.cumsum(np.exp(self.fx[:-1, 3] + self.bx[:-1, 3] - tot))
        etot[1:] = np.cumsum(np.exp(self.fx[1:, 0] + self.bx[1:, 0] - tot))
        njc = sum(np.exp(self.fx[:-1, col] + self.loop + self.bx[1:, col] - tot) for col in (1, 2, 4))
        mocc[1:] = 1.0 - njc
        return btot, etot, mocc


def forward_backward(model, seq, multihit, cells=False, length=None, backward=True):
    """length: the target length the N / J / C length model is formed from, where it is not len(seq) -- a domain envelope is
    scored over its own residues under the length model of the whole target.  backward=False: Forward only (fwd and fx)."""
    m = model
    M = m.M
    seq = np.asarray(seq, dtype=np.int64)
    L = len(seq)
    loop, move, emove, eloop = length_model(L if length is None else length, multihit)
    k = slice(1, M + 1)
    km1 = slice(0, M)
    kp1 = slice(2, M + 2)
    r = RefResult()
    r.L, r.loop, r.move = L, loop, move
    fx = np.full((L + 1, 5), NEG)
    bx = np.full((L + 1, 5), NEG)
    E, N, J, B, C = range(5)
    if cells:
        r.fM, r.fI = np.full((L + 1, M + 2), NEG), np.full((L + 1, M + 2), NEG)
        r.bM, r.bI = np.full((L + 1, M + 2), NEG), np.full((L + 1, M + 2), NEG)
        r.fD, r.bD = np.full((L + 1, M + 2), NEG), np.full((L + 1, M + 2), NEG)

    # ---- Forward
    fx[0, N], fx[0, B] = 0.0, move
    Mp, Ip, Dp = (np.full(M + 2, NEG) for _ in range(3))
    for i in range(1, L + 1):
        e = m.e[seq[i - 1]]
        Mc, Ic, Dc = (np.full(M + 2, NEG) for _ in range(3))
        Mc[k] = e[k] + lae(lae(fx[i - 1, B] + m.bm[k], Mp[km1] + m.mm[k]), lae(Ip[km1] + m.im[k], Dp[km1] + m.dm[k]))
        Ic[k] = lae(Mp[k] + m.mi[k], Ip[k] + m.ii[k])
        if M > 1:
            if m.dd_closed:
                # D_k = P[k] + logsum_{j < k} (M_j + md_j - P[j + 1]), k = 2..M
                Dc[2:M + 1] = m.P[2:M + 1] + lae.accumulate(Mc[1:M] + m.md[1:M] - m.P[2:M + 1])
            else:
                for kk in range(2, M + 1):
                    Dc[kk] = lae(Mc[kk - 1] + m.md[kk - 1], Dc[kk - 1] + m.dd[kk - 1])
        xE = lae.reduce(lae(Mc[k], Dc[k]))
        fx[i, E] = xE
        fx[i, N] = fx[i - 1, N] + loop
        fx[i, C] = lae(fx[i - 1, C] + loop, xE + emove)
        fx[i, J] = lae(fx[i - 1, J] + loop, xE + eloop)
        fx[i, B] = lae(fx[i, J] + move, fx[i, N] + move)
        if cells:
            r.fM[i], r.fI[i], r.fD[i] = Mc, Ic, Dc
        Mp, Ip, Dp = Mc, Ic, Dc
    r.fwd = float(fx[L, C] + move)
    if not backward:
        r.fx = fx
        return r

    # ---- Backward
    def close_row(xE, a_m, a_d):
        """M and D of a row from its E and the parts that come from the row below (a_m, a_d: nodes 1..M in [k])."""
        Dc = np.full(M + 2, NEG)
        a = lae(xE, a_d)                       # D_k = a_k (+) dd_k + D_{k+1}
        if m.dd_closed:
            Dc[k] = -m.P[k] + lae.accumulate((a[k] + m.P[k])[::-1])[::-1]
        else:
            for kk in range(M, 0, -1):
                Dc[kk] = lae(a[kk], m.dd[kk] + Dc[kk + 1])
        Mc = np.full(M + 2, NEG)
        Mc[k] = lae(lae(xE, a_m[k]), m.md[k] + Dc[kp1])
        return Mc, Dc

    none = np.full(M + 2, NEG)
    if L >= 1:
        bx[L, C] = move
        bx[L, E] = bx[L, C] + emove
        Mn, Dn = close_row(bx[L, E], none, none)
        In = none.copy()
        if cells:
            r.bM[L], r.bI[L], r.bD[L] = Mn, In, Dn
        for i in range(L - 1, -1, -1):
            e = m.e[seq[i]]                    # residue i + 1
            em = np.full(M + 2, NEG)
            em[k] = e[k] + Mn[k]               # emission times M of the row below
            xB = lae.reduce(m.bm[k] + em[k])
            bx[i, B] = xB
            if i == 0:
                bx[0, N] = lae(xB + move, bx[1, N] + loop)
                break
            bx[i, C] = bx[i + 1, C] + loop
            bx[i, J] = lae(xB + move, bx[i + 1, J] + loop)
            bx[i, N] = lae(xB + move, bx[i + 1, N] + loop)
            bx[i, E] = lae(bx[i, C] + emove, bx[i, J] + eloop)
            a_m, a_d, Ic = none.copy(), none.copy(), none.copy()
            a_m[k] = lae(m.mm[kp1] + em[kp1], m.mi[k] + In[k])
            a_d[k] = m.dm[kp1] + em[kp1]
            Ic[k] = lae(m.im[kp1] + em[kp1], m.ii[k] + In[k])
            Mn, Dn = close_row(bx[i, E], a_m, a_d)
            In = Ic
            if cells:
                r.bM[i], r.bI[i], r.bD[i] = Mn, In, Dn
        r.bck = float(bx[0, N])
    else:
        r.bck = r.fwd
    r.fx, r.bx = fx, bx
    return r


# ---- an independent statement of Forward: the sum over every path, enumerated (tiny models and targets only)
def enumerate_paths(model, seq, multihit, length=None, emitters=False):
    """log of the summed probability of every complete path S N.. B .. E (J .. B .. E)* C.. T that emits exactly <seq>.
    length: as in forward_backward.  emitters: return (that log, usage) instead, usage[i - 1] = {state: probability} of
    residue i's emitter over the paths, not normalised -- states ("M", k), ("I", k), ("N", 0), ("J", 0), ("C", 0)."""
    m, M, L = model, model.M, len(seq)
    loop, move, emove, eloop = (float(np.exp(v)) for v in length_model(L if length is None else length, multihit))
    ex = lambda a: float(np.exp(a))
    total = []
    who = []                                   # the emitter of each residue emitted so far on the path being walked
    usage = [{} for _ in range(L)]

    def emits(fn):
        """<fn> visits a state that has just emitted residue i: it is on the path for as long as the visit lasts."""
        def inner(state, kk, i, p):
            if p == 0.0:
                return
            who.append((state, kk))
            fn(state, kk, i, p)
            who.pop()
        return inner

    def em(kk, i):
        return ex(m.e[seq[i], kk])

    def visit(state, kk, i, p):
        """<i> residues emitted so far; <p> the probability of the path up to and including <state>."""
        if p == 0.0:
            return
        if state == "N":
            if i < L:
                emit("N", 0, i + 1, p * loop)
            visit("B", 0, i, p * move)
        elif state == "B":
            if i < L:
                for k2 in range(1, M + 1):
                    emit("M", k2, i + 1, p * ex(m.bm[k2]) * em(k2, i))
        elif state == "M":
            visit("E", 0, i, p)
            if i < L:
                emit("I", kk, i + 1, p * ex(m.mi[kk]))
                if kk < M:
                    emit("M", kk + 1, i + 1, p * ex(m.mm[kk + 1]) * em(kk + 1, i))
            if kk < M:
                visit("D", kk + 1, i, p * ex(m.md[kk]))
        elif state == "I":
            if i < L:
                emit("I", kk, i + 1, p * ex(m.ii[kk]))
                if kk < M:
                    emit("M", kk + 1, i + 1, p * ex(m.im[kk + 1]) * em(kk + 1, i))
        elif state == "D":
            visit("E", 0, i, p)
            if kk < M:
                visit("D", kk + 1, i, p * ex(m.dd[kk]))
                if i < L:
                    emit("M", kk + 1, i + 1, p * ex(m.dm[kk + 1]) * em(kk + 1, i))
        elif state == "E":
            visit("C", 0, i, p * emove)
            visit("J", 0, i, p * eloop)
        elif state == "J":
            if i < L:
                emit("J", 0, i + 1, p * loop)
                visit("B", 0, i, p * move)
        elif state == "C":
            if i < L:
                emit("C", 0, i + 1, p * loop)
            else:
                total.append(p * move)
                if emitters:
                    for pos, state in enumerate(who):
                        usage[pos].setdefault(state, []).append(p * move)

    emit = emits(visit)
    visit("N", 0, 0, 1.0)
    import math
    s = math.fsum(total)
    logsum = math.log(s) if s > 0 else NEG
    if emitters:
        return logsum, [{state: math.fsum(ps) for state, ps in u.items()} for u in usage]
    return logsum


# ---- the float32 engines' outputs in the reference's terms
def scaled_rows_to_logs(fx, bx):
    """The engines' special-state rows ((L+1) x [E N J B C SCALE], each row divided by its scale factor) as natural logs of the
    unscaled values: a Forward row carries the factors of rows 1..i, a Backward row those of rows i..L (row 0: of 1..L).
    Returns (flog, blog), (L+1) x 5; a zero is -inf."""
    fx, bx = np.asarray(fx, dtype=np.float64), np.asarray(bx, dtype=np.float64)
    fcum = np.cumsum(np.log(fx[:, 5]))
    blogs = np.log(bx[:, 5])
    bcum = np.cumsum(blogs[::-1])[::-1]
    if len(bcum) > 1:
        bcum[0] = bcum[1]
    return _log(fx[:, :5]) + fcum[:, None], _log(bx[:, :5]) + bcum[:, None]


def rows_scores(fx, bx, move):
    """Forward and Backward totals (nats) from the rows: C(L) + log pmove, and N(0)."""
    flog, blog = scaled_rows_to_logs(fx, bx)
    return float(flog[-1, 4] + move), float(blog[0, 1])


def row_error(fx, bx, ref):
    """Largest |engine - reference| / max(|reference|, 1) over the special-state logs, where the engine's scaled value is a
    normal float32 (cells far below their row's scale are denormal or zero in the engine; the reference has no scale)."""
    flog, blog = scaled_rows_to_logs(fx, bx)
    tiny = np.finfo(np.float32).tiny
    worst = 0.0
    for got, want, raw in ((flog, ref.fx, fx), (blog, ref.bx, bx)):
        ok = (np.asarray(raw)[:, :5] >= tiny) & np.isfinite(want)
        if ok.any():
            worst = max(worst, float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)).max()))
    return worst


_T_M, _T_I, _T_N, _T_C, _T_J = 1, 3, 5, 8, 10           # p7T_* codes of Trace.st


def trace_posteriors(ref, trace):
    """The reference's posterior of every step of a trace (what Trace.posterior_probabilities holds: the emitting state's
    posterior for M / I and for N / C / J steps that emit, 0 elsewhere)."""
    ppM, ppI, pN, pJ, pC = ref.posteriors()
    st, k, i = np.asarray(trace.st), np.asarray(trace.k), np.asarray(trace.i)
    want = np.zeros(len(st))
    for code, table in ((_T_M, ppM), (_T_I, ppI)):
        sel = st == code
        want[sel] = table[i[sel], k[sel]]
    for code, table in ((_T_N, pN), (_T_C, pC), (_T_J, pJ)):
        sel = (st == code) & (i > 0)
        want[sel] = table[i[sel]]
    return want
