"""numpy restatement of the row order of p7x_vitpk.hip::vit_row (test infrastructure), next to vit_striped_emu.py, which
keeps the order the kernel had before: here the first pass of the D->D closure runs inside the register loop of every
row (register 0 counting as -32768), the stripe shift after the loop carries max(M->D, D->D exit) of a stripe into
register 0 of the next, and a target that asks for the closure (Dmax + ddbound > xB) enters the pass loop from there:
walk every stripe down from register 0, carry, until no register 0 improves.  tests/test_host_vit_row.py checks it
against the oracle's scalar recurrence; `passes`, if given, collects the pass count of every row that asked."""
import numpy as np
import oracle_lib

from vit_striped_emu import NEG, sat, unstripe


def vit_row_order(op, seq, T, P, passes=None, skip_pass_loop=False):
    p = op.p; M = p.M; L = len(seq)
    oracle_lib.lib().p7o_reconfig_length(op.ptr, L)
    tw, rw = unstripe(op)
    S = 2 * T
    assert S * P >= M and P >= 2
    node = np.array([[s * P + q + 1 for s in range(S)] for q in range(P)])        # [P][S]
    ok = node <= M
    def tab(t): return np.where(ok, tw[t][np.minimum(node, M + 1)], NEG)
    BM, MM, IM, DM, MD, MI, II, DD = [tab(t) for t in range(8)]
    base, xwe, xwm, ddb = int(p.base_w), int(p.xw[0][0]), int(p.xw[1][0]), int(p.ddbound_w)
    Mr = np.full((P, S), NEG, np.int64); Ir = Mr.copy(); Dr = Mr.copy()
    xN, xJ, xC = base, NEG, NEG
    xB = xN + xwm
    def shift(v):                       # value of the previous stripe, -32768 into stripe 0
        o = np.empty_like(v); o[0] = NEG; o[1:] = v[:-1]; return o
    for i in range(L):
        em = np.where(ok, rw[int(seq[i])][np.minimum(node, M + 1)], NEG)
        Mn = np.empty_like(Mr); In = np.empty_like(Mr); Dn = np.full_like(Mr, NEG)
        mp, ip, dp = shift(Mr[P - 1]), shift(Ir[P - 1]), shift(Dr[P - 1])
        dcv, dmax = None, NEG
        for q in range(P):
            sv = np.maximum(np.maximum(sat(xB + BM[q]), sat(mp + MM[q])), np.maximum(sat(ip + IM[q]), sat(dp + DM[q])))
            sv = sat(sv + em[q])
            Mn[q] = sv
            if q == 1: Dn[1] = dcv
            if q > 1: Dn[q] = np.maximum(dcv, sat(Dn[q - 1] + DD[q - 1]))        # first closure pass, in the loop
            dcv = sat(sv + MD[q])
            dmax = max(dmax, int(dcv.max()))
            In[q] = np.maximum(sat(Mr[q] + MI[q]), sat(Ir[q] + II[q]))
            mp, ip, dp = Mr[q], Ir[q], Dr[q]
        Dn[0] = shift(np.maximum(dcv, sat(Dn[P - 1] + DD[P - 1])))               # M->D and the stripe's D->D exit
        xE = int(Mn.max())
        if xE >= 32767: return 32767
        xC = max(xC, xE + xwe); xJ = max(xJ, xE + xwe); xB = max(xJ + xwm, xN + xwm)
        if dmax + ddb > xB and not skip_pass_loop:
            npass = 0
            while True:
                npass += 1
                for q in range(1, P):
                    Dn[q] = np.maximum(Dn[q], sat(Dn[q - 1] + DD[q - 1]))
                d0 = np.maximum(Dn[0], shift(sat(Dn[P - 1] + DD[P - 1])))
                changed = bool((d0 != Dn[0]).any())
                Dn[0] = d0
                if not changed or npass >= 2 * T: break
            if passes is not None: passes.append(npass)
        Mr, Ir, Dr = Mn, In, Dn
    return xC
