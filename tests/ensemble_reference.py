"""Float64 reference of the stochastic-traceback ensembles of a multi-domain region (test infrastructure only): the choice
probabilities of every cell and row (what the kernels and the host twin store as integer thresholds, p7x_choice.hpp), a check
of sampled paths against them deviate by deviate, the posterior marginals a sampled ensemble must reproduce, and null2 by
trace (p7_Null2_ByTrace) from a path.

Built on tests/dp_reference.py: the region is scored as the product scores it -- multihit Forward / Backward over the
region's residues only, under the length model of the whole target.  A traceback runs from C(Lr) back to S and at every
state but N draws one deviate u = x / 2^32 from the LCG x <- 69069 x + 1 and takes the first alternative whose cumulative
probability exceeds u.  The alternatives and their order, stated here from the recursion and not from the float32 code:

    M(i, k)   B(i-1) bm_k | M(i-1, k-1) mm_k | I(i-1, k-1) im_k | D(i-1, k-1) dm_k        three cumulative values
    I(i, k)   M(i-1, k) mi_k | I(i-1, k) ii_k
    D(i, k)   M(i, k-1) md_{k-1} | D(i, k-1) dd_{k-1}
    C(i)      C(i-1) loop | E(i) E->C          J(i)   J(i-1) loop | E(i) E->J          B(i)   N(i) move | J(i) move
    E(i)      M(i, k) then D(i, k) in upstream's striped visiting order: q = 0 .. Q-1 outer; inside, the four match cells
              k = z Q + q + 1, z = 0 .. 3, then the four delete cells of the same nodes

A state's row is the number of residues emitted up to and including it."""
from types import SimpleNamespace

import numpy as np

import dp_reference as R
from envelope_reference import finish_null2

NEG = -np.inf
lae = np.logaddexp
TWO32 = 4294967296.0
sM, sD, sI, sS, sN, sB, sE, sC, sT, sJ = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10          # p7T_* codes of a trace
DRAWS = (sM, sD, sI, sC, sJ, sB, sE)                                             # the states that draw a deviate
FLOOR = 1e-9                    # a choice point counts where its cell's posterior is at least this
DECADES = (1e-3, 1e-6, 1e-9, 1e-12, 0.0)
NSAMPLES = 200


def lcg_stream(x0, n):
    """x_1 .. x_n of x <- 69069 x + 1 (mod 2^32) from the state x_0, by doubling."""
    mask = np.uint64(0xFFFFFFFF)
    out = np.array([(int(x0) * 69069 + 1) & 0xFFFFFFFF], dtype=np.uint64)
    a, c = 69069, 1                              # the map that advances len(out) steps
    while len(out) < n:
        out = np.concatenate([out, (np.uint64(a) * out + np.uint64(c)) & mask])
        a, c = (a * a) & 0xFFFFFFFF, (a * c + c) & 0xFFFFFFFF
    return out[:n]


def _cumulative(parts):
    """Cumulative probabilities of all but the last alternative (last axis) from the alternatives' log weights; nan where
    no alternative has any weight (a cell no path reaches)."""
    tot = lae.reduce(np.stack(parts), axis=0)
    acc, cums = parts[0], []
    for p in parts[1:]:
        cums.append(acc)
        acc = lae(acc, p)
    with np.errstate(invalid="ignore"):
        return np.exp(np.stack(cums, axis=-1) - tot[..., None])


def record_cumulatives(cells, rows):
    """The cumulative probabilities a set of choice records stands for (cells[Lr+1, M+1, 8], rows[Lr+1, 8] words): T / 2^32,
    and where a threshold is 0, 1 if the fallback path lies at or before it (its ratio reached 1), else 0 (never taken)."""
    cells, rows = np.asarray(cells, dtype=np.uint32), np.asarray(rows, dtype=np.uint32)
    T, fb = cells[..., 0:3].astype(np.float64), (cells[..., 3] & 3).astype(np.int64)
    tM = np.where(T > 0, T / TWO32, np.where(fb[..., None] <= np.arange(3), 1.0, 0.0))
    pair = lambda t, f: np.where(t > 0, t.astype(np.float64) / TWO32, np.where(f == 0, 1.0, 0.0))
    bits = rows[:, 3]
    return SimpleNamespace(M=tM, I=pair(cells[..., 4], cells[..., 6] & 1), D=pair(cells[..., 5], (cells[..., 6] >> 2) & 1),
                           C=pair(rows[:, 0], bits & 1), J=pair(rows[:, 1], (bits >> 2) & 1), B=pair(rows[:, 2], (bits >> 4) & 1))


class RegionReference:
    """Region i..j (1-based) of the target <seq> under <model> (dp_reference.RefModel); Q: vectors per stripe of the
    optimized profile (rfv.shape[1] // 4), which fixes the E state's visiting order."""

    def __init__(self, model, Q, seq, i, j):
        seq = np.asarray(seq)
        self.m, self.M, self.Q = model, model.M, int(Q)
        self.sub = np.asarray(seq[i - 1:j], dtype=np.int64)
        self.Lr, self.L = len(self.sub), len(seq)
        assert 1 <= i <= j <= self.L and 4 * self.Q >= self.M
        self.ref = r = R.forward_backward(model, self.sub, True, cells=True, length=self.L)
        self.loop, self.move, self.emove, self.eloop = R.length_model(self.L, True)
        m, M, Lr, fx = model, self.M, self.Lr, r.fx
        k, km1 = slice(1, M + 1), slice(0, M)
        E, N, J, B, C = range(5)
        self.qM = np.full((Lr + 1, M + 2, 3), np.nan)
        self.qI, self.qD = np.full((Lr + 1, M + 2), np.nan), np.full((Lr + 1, M + 2), np.nan)
        self.qM[1:, k] = _cumulative([fx[:-1, B][:, None] + m.bm[k], r.fM[:-1, km1] + m.mm[k], r.fI[:-1, km1] + m.im[k],
                                      r.fD[:-1, km1] + m.dm[k]])
        self.qI[1:, k] = _cumulative([r.fM[:-1, k] + m.mi[k], r.fI[:-1, k] + m.ii[k]])[..., 0]
        if M > 1:
            self.qD[1:, 2:M + 1] = _cumulative([r.fM[1:, 1:M] + m.md[1:M], r.fD[1:, 1:M] + m.dd[1:M]])[..., 0]
        self.qC, self.qJ = np.full(Lr + 1, np.nan), np.full(Lr + 1, np.nan)
        self.qC[1:] = _cumulative([fx[:-1, C] + self.loop, fx[1:, E] + self.emove])[..., 0]
        self.qJ[1:] = _cumulative([fx[:-1, J] + self.loop, fx[1:, E] + self.eloop])[..., 0]
        self.qB = _cumulative([fx[:, N] + self.move, fx[:, J] + self.move])[..., 0]
        tot = r.fwd
        self.pM, self.pI, self.pD = np.exp(r.fM + r.bM - tot), np.exp(r.fI + r.bI - tot), np.exp(r.fD + r.bD - tot)
        self.pX = np.exp(fx + r.bx - tot)                    # (Lr + 1) x [E N J B C]: the state is on the path at that row
        kk = np.arange(4)[None, :] * self.Q + np.arange(self.Q)[:, None] + 1
        self.e_k = np.concatenate([kk, kk], axis=1).ravel()                       # node of every entry of E's visiting order
        self.e_d = np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), self.Q)            # 1: its delete cell
        self._e_cum = {}

    # ---- the E state
    def e_cum(self, row):
        """Cumulative probabilities over E(row)'s visiting order (nodes beyond M have no weight)."""
        if row not in self._e_cum:
            kc = np.minimum(self.e_k, self.M + 1)
            w = np.where(self.e_d == 1, self.ref.fD[row, kc], self.ref.fM[row, kc])
            self._e_cum[row] = np.exp(lae.accumulate(w) - self.ref.fx[row, 0])
        return self._e_cum[row]

    def e_pos(self, state, k):
        return ((k - 1) % self.Q) * 8 + (4 if state == sD else 0) + (k - 1) // self.Q

    # ---- one step, in plain terms (the self-checks walk enumerated paths with it)
    def step_interval(self, s0, row, k, s1, k1):
        """[lo, hi) of the deviate for which the traceback at state s0 (row, node k) goes to s1 (node k1 when s0 is E)."""
        if s0 == sM:
            cum, idx = list(self.qM[row, k]) + [1.0], {sB: 0, sM: 1, sI: 2, sD: 3}[s1]
        elif s0 == sE:
            cum, idx = self.e_cum(row), self.e_pos(s1, k1)
        else:
            q, first = {sD: (self.qD[row, k], sM), sI: (self.qI[row, k], sM), sC: (self.qC[row], sC), sJ: (self.qJ[row], sJ),
                        sB: (self.qB[row], sN)}[s0]
            cum, idx = [q, 1.0], 0 if s1 == first else 1
        return (cum[idx - 1] if idx > 0 else 0.0), cum[idx]

    def path_probability(self, path):
        """Product of the choice probabilities along a path [(state, k, row)] in forward order, S first."""
        p = 1.0
        for z in range(1, len(path)):
            s0, k, row = path[z]
            if s0 in DRAWS:
                lo, hi = self.step_interval(s0, row, k, path[z - 1][0], path[z - 1][1])
                p *= hi - lo
        return p

    # ---- thresholds
    def e_cum_all(self):
        """e_cum of every row, [Lr + 1, 8 Q] (row 0: nan)."""
        kc = np.minimum(self.e_k, self.M + 1)
        w = np.where(self.e_d == 1, self.ref.fD[:, kc], self.ref.fM[:, kc])
        with np.errstate(invalid="ignore"):
            return np.exp(lae.accumulate(w, axis=1) - self.ref.fx[:, 0:1])

    def record_e_cum(self, rows, md):
        """The cumulative sums the float32 walk compares its deviate with at E(row): the scaled Forward values md[row, k]
        (M, D) times the row's factor (float) (1 / xE) -- float32 products -- added up in double in the visiting order."""
        norm = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32)[:, 4]).view(np.float32)
        v = np.asarray(md, dtype=np.float32)[:, np.minimum(self.e_k, self.M), self.e_d]
        v = np.where(self.e_k <= self.M, v, np.float32(0.0)) * norm[:, None]
        assert v.dtype == np.float32
        return np.cumsum(v.astype(np.float64), axis=1)

    def threshold_distance(self, cells, rows, md):
        """Largest |T / 2^32 - q| over the choice points of the records whose cell (row) has a posterior of at least each
        floor of DECADES: {floor: distance}; for the E state the walk's cumulative sums stand where the other states have
        T / 2^32.  Points no float64 path reaches (q is nan) are left out of every floor."""
        t = record_cumulatives(cells, rows)
        M = self.M
        post_e = np.broadcast_to(self.pX[1:, 0:1], (self.Lr, len(self.e_k)))
        d, p = [np.abs(self.record_e_cum(rows, md)[1:] - self.e_cum_all()[1:]).ravel()], [post_e.ravel()]
        for got, want, post in ((t.M[1:, 1:], self.qM[1:, 1:M + 1], self.pM[1:, 1:M + 1]),
                                (t.I[1:, 1:], self.qI[1:, 1:M + 1], self.pI[1:, 1:M + 1]),
                                (t.D[1:, 2:], self.qD[1:, 2:M + 1], self.pD[1:, 2:M + 1]),
                                (t.C[1:], self.qC[1:], self.pX[1:, 4]), (t.J[1:], self.qJ[1:], self.pX[1:, 2]),
                                (t.B, self.qB, self.pX[:, 3])):
            diff = np.abs(got - want)
            if diff.ndim > post.ndim:
                diff = diff.max(axis=-1)
            d.append(diff.ravel())
            p.append(post.ravel())
        d, p = np.concatenate(d), np.concatenate(p)
        known = ~np.isnan(d)
        return {fl: float(d[known & (p >= fl)].max()) if (known & (p >= fl)).any() else 0.0 for fl in DECADES}

    # ---- sampled paths, deviate by deviate
    def rows_of(self, st, i, off):
        """The row of every step of concatenated traces (sample t: steps off[t] .. off[t+1] - 1)."""
        t_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
        big = self.Lr + 1
        return np.maximum.accumulate(np.asarray(i, dtype=np.int64) + t_of * big) - t_of * big, t_of

    def walk_check(self, st, k, i, off, x0):
        """Follow the sampled paths with the generator stream that starts from state x0.  For every deviate drawn (sample
        by sample, each from C(Lr) back to S): ok -- the step taken is the one float64 picks; dist -- else how far the
        deviate lies from the float64 interval of the step taken; sample -- whose deviate it is."""
        st, k, i = np.asarray(st, dtype=np.int64), np.asarray(k, dtype=np.int64), np.asarray(i, dtype=np.int64)
        rows, t_of = self.rows_of(st, i, off)
        emit = (st == sM) | (st == sI)
        assert np.array_equal(rows[emit], i[emit]), "a trace's residue numbers do not count up"
        z = np.nonzero(np.isin(st, DRAWS))[0]
        z = z[np.lexsort((-z, t_of[z]))]
        u = lcg_stream(x0, len(z)).astype(np.float64) / TWO32
        s0, s1, k0, k1, r0 = st[z], st[z - 1], k[z], k[z - 1], rows[z]
        lo, hi = np.zeros(len(z)), np.ones(len(z))
        sel = s0 == sM
        cum4 = np.concatenate([self.qM[r0[sel], k0[sel]], np.ones((int(sel.sum()), 1))], axis=1)
        idx = np.select([s1[sel] == sB, s1[sel] == sM, s1[sel] == sI], [0, 1, 2], 3)
        n = np.arange(len(idx))
        lo[sel], hi[sel] = np.where(idx > 0, cum4[n, np.maximum(idx - 1, 0)], 0.0), cum4[n, idx]
        for state, q, first in ((sD, self.qD[r0, k0], sM), (sI, self.qI[r0, k0], sM), (sC, self.qC[r0], sC), (sJ, self.qJ[r0], sJ),
                                (sB, self.qB[r0], sN)):
            sel = s0 == state
            head = s1[sel] == first
            lo[sel], hi[sel] = np.where(head, 0.0, q[sel]), np.where(head, q[sel], 1.0)
        for n in np.nonzero(s0 == sE)[0]:
            cum, pos = self.e_cum(int(r0[n])), self.e_pos(int(s1[n]), int(k1[n]))
            lo[n], hi[n] = (cum[pos - 1] if pos > 0 else 0.0), cum[pos]
        ok = (lo <= u) & (u < hi)
        with np.errstate(invalid="ignore"):
            dist = np.where(ok, 0.0, np.maximum(lo - u, u - hi))
        return SimpleNamespace(ok=ok, dist=dist, sample=t_of[z], state=s0)

    # ---- what an ensemble must reproduce
    def marginals(self):
        """Probabilities, per sampled path, of: M[r, k] / I[r, k] residue r emitted by M_k / I_k; D[r, k] D_k visited on row r;
        inside[r] residue r emitted inside a domain; start[r] / end[r] a domain's first / last residue is r; first[k] the
        first domain enters at node k; last[k] the last match state of the last domain is node k."""
        r, m, M, Lr, tot = self.ref, self.m, self.M, self.Lr, self.ref.fwd
        ppM, ppI, pN, pJ, pC = r.posteriors()
        start, end = np.zeros(Lr + 1), np.zeros(Lr + 1)
        start[1:], end[1:] = self.pX[:-1, 3], self.pX[1:, 0]
        first, last = np.zeros(M + 2), np.zeros(M + 2)
        k = slice(1, M + 1)
        e = m.e[self.sub]                                                # e[r - 1]: residue r
        first[k] = np.exp(r.fx[:-1, 1][:, None] + self.move + m.bm[k] + e[:, k] + r.bM[1:, k] - tot).sum(axis=0)
        g = np.full(M + 2, NEG)                                          # g[j]: D_j reaches E (by itself or down the chain)
        if M >= 1:
            g[M] = 0.0
        for j in range(M - 1, 0, -1):
            g[j] = lae(0.0, m.dd[j] + g[j + 1])
        leave = lae(0.0, m.md[k] + g[2:M + 2])                           # M_k reaches E without another match state
        tail = (Lr - np.arange(Lr + 1)) * self.loop + self.move          # E -> C, C emits the rest, C -> T
        last[k] = np.exp(r.fM[:, k] + leave + self.emove + tail[:, None] - tot).sum(axis=0)
        inside = np.zeros(Lr + 1)
        inside[1:] = 1.0 - (pN + pJ + pC)[1:]
        return {"M": ppM, "I": ppI, "D": self.pD, "inside": inside, "start": start, "end": end, "first": first, "last": last}

    # ---- null2 by trace
    def null2_of_domain(self, ks, degeneracy):
        """p7_Null2_ByTrace of one domain: ks -- the node of every residue-emitting step of it, match AND insert (upstream
        counts an insert's emission in the match slot of its node); every such step weighs 1 / len(ks)."""
        K = np.asarray(degeneracy).shape[1]
        null2 = np.ones(self.m.Kp)
        null2[:K] = np.exp(self.m.e[:K][:, np.asarray(ks, dtype=np.int64)]).sum(axis=1) / len(ks)
        return finish_null2(null2, degeneracy)

    def null2_sums(self, st, k, i, off, degeneracy):
        """n2[pos], pos = 1..Lr: the null2 odds ratio of region residue pos summed over the sampled paths -- 1 outside the
        domains and (upstream's second quirk) at the first residue of each domain."""
        st, k, i = np.asarray(st), np.asarray(k), np.asarray(i)
        n2 = np.zeros(self.Lr + 1)
        for t in range(len(off) - 1):
            a, b = int(off[t]), int(off[t + 1])
            per = np.ones(self.Lr + 1)
            for zb, ze in zip(a + np.nonzero(st[a:b] == sB)[0], a + np.nonzero(st[a:b] == sE)[0]):
                seg = slice(zb, ze + 1)
                emits = i[seg] > 0
                null2 = self.null2_of_domain(k[seg][emits], degeneracy)
                mi = i[seg][st[seg] == sM]
                sqfrom, sqto = int(mi[0]), int(mi[-1])
                per[sqfrom + 1:sqto + 1] = null2[self.sub[sqfrom:sqto]]
            n2 += per
        n2[0] = 0.0
        return n2


# ---- an independent statement of the path space: every complete path with its probability (tiny cases only)
def enumerate_full_paths(model, seq, length=None):
    """[(path, probability)] of every multihit path that emits exactly <seq>; path = [(state, k, row)], S first, T last."""
    m, M, L = model, model.M, len(seq)
    loop, move, emove, eloop = (float(np.exp(v)) for v in R.length_model(L if length is None else length, True))
    ex = lambda a: float(np.exp(a))
    out, path = [], [(sS, 0, 0)]

    def go(state, k, row, p):
        if p == 0.0:
            return
        path.append((state, k, row))
        em = lambda kk: ex(m.e[seq[row], kk])              # of the next residue
        if state == sN:
            if row < L:
                go(sN, 0, row + 1, p * loop)
            go(sB, 0, row, p * move)
        elif state == sB:
            if row < L:
                for k2 in range(1, M + 1):
                    go(sM, k2, row + 1, p * ex(m.bm[k2]) * em(k2))
        elif state in (sM, sD):
            go(sE, 0, row, p)
            if state == sM and row < L:
                go(sI, k, row + 1, p * ex(m.mi[k]))
            if k < M:
                go(sD, k + 1, row, p * ex(m.md[k] if state == sM else m.dd[k]))
                if row < L:
                    go(sM, k + 1, row + 1, p * ex(m.mm[k + 1] if state == sM else m.dm[k + 1]) * em(k + 1))
        elif state == sI:
            if row < L:
                go(sI, k, row + 1, p * ex(m.ii[k]))
                if k < M:
                    go(sM, k + 1, row + 1, p * ex(m.im[k + 1]) * em(k + 1))
        elif state == sE:
            go(sC, 0, row, p * emove)
            go(sJ, 0, row, p * eloop)
        elif state == sJ:
            if row < L:
                go(sJ, 0, row + 1, p * loop)
                go(sB, 0, row, p * move)
        elif state == sC:
            if row < L:
                go(sC, 0, row + 1, p * loop)
            else:
                out.append((path + [(sT, 0, row)], p * move))
        path.pop()

    go(sN, 0, 0, 1.0)
    return out


# ---- counting a sampled ensemble against the marginals
def within(count, S, p):
    """The rule of tests/test_host_emit.py::test_distribution: a count of S Bernoulli(p) trials."""
    return np.abs(count - S * p) <= 6.0 * np.sqrt(S * p * (1.0 - np.minimum(p, 1.0))) + 1.0


TRACE_FAMILIES = ("M", "I", "D")
DOM_FAMILIES = ("inside", "start", "end", "first", "last")
EXCLUSIVE = ("first", "last")          # exactly one event of the family per path


class Tally:
    """Counts of the indicator events over sampled ensembles.  A cell with S p >= 1 (S: the samples expected in all) is
    counted by itself.  The rarer cells of a family are pooled into one indicator per family, "the path has at least one of
    them": for the two families with exactly one event per path its probability is the sum of theirs; for the others that
    sum only bounds it from above (a path can hold two of them), and the pooled count is tested from above alone."""

    def __init__(self, marginals, S, families):
        self.p, self.S, self.families, self.n = marginals, S, families, 0
        self.rare = {f: marginals[f] * S < 1.0 for f in families}
        self.count = {f: np.zeros(marginals[f].shape, dtype=np.int64) for f in families}
        self.pooled = {f: 0 for f in families}

    def add_domains(self, dom, nsamples=NSAMPLES):
        """dom[n, 5]: sample, first / last residue, first / last node; a sample's domains first to last."""
        dom = np.asarray(dom, dtype=np.int64)
        self.n += nsamples
        hit = {f: np.zeros(nsamples, dtype=bool) for f in DOM_FAMILIES}
        firsts = np.nonzero(np.diff(dom[:, 0], prepend=-1) != 0)[0]
        lasts = np.nonzero(np.diff(dom[:, 0], append=-1) != 0)[0]
        assert len(firsts) == nsamples, "a sampled path without a domain"
        events = (("start", dom[:, 0], dom[:, 1]), ("end", dom[:, 0], dom[:, 2]), ("first", dom[firsts, 0], dom[firsts, 3]),
                  ("last", dom[lasts, 0], dom[lasts, 4]))
        for f, t, where in events:
            if f in self.families:
                np.add.at(self.count[f], where, 1)
                hit[f][t[self.rare[f][where]]] = True
        if "inside" in self.families:
            for t, a, b in dom[:, :3]:
                self.count["inside"][a:b + 1] += 1
                hit["inside"][t] |= bool(self.rare["inside"][a:b + 1].any())
        for f in DOM_FAMILIES:
            if f in self.families:
                self.pooled[f] += int(hit[f].sum())

    def add_traces(self, st, k, rows, t_of, nsamples=NSAMPLES):
        st = np.asarray(st)
        for f, code in (("M", sM), ("I", sI), ("D", sD)):
            sel = st == code
            np.add.at(self.count[f], (rows[sel], k[sel]), 1)
            hit = np.zeros(nsamples, dtype=bool)
            hit[t_of[sel][self.rare[f][rows[sel], k[sel]]]] = True
            self.pooled[f] += int(hit.sum())

    def violations(self):
        """([(family, cell, count, expected)], cells tested)."""
        bad, cells, S = [], 0, self.n
        assert S == self.S
        for f in self.families:
            p, c, rare = self.p[f], self.count[f], self.rare[f]
            ok = within(c, S, p) | rare
            bad += [(f, tuple(int(v) for v in ix), int(c[tuple(ix)]), float(S * p[tuple(ix)])) for ix in np.argwhere(~ok)]
            cells += int((~rare).sum())
            q = float(min(p[rare].sum(), 1.0))
            if rare.any() and S * q >= 1.0:
                cells += 1
                low_ok = f not in EXCLUSIVE or self.pooled[f] >= S * q - (6.0 * np.sqrt(S * q * (1.0 - q)) + 1.0)
                if not (self.pooled[f] <= S * q + 6.0 * np.sqrt(S * q * (1.0 - q)) + 1.0 and low_ok):
                    bad.append((f, "pooled", self.pooled[f], S * q))
        return bad, cells
