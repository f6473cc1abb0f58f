"""CPU tests of the long-target SSV scan in chained parts (models of more nodes than one launch of the kernel holds): the
plan of the parts, the tables of a part, and the host's merge of the rows the parts report -- host code behind the test
seams p7x_debug_ssv_plan, p7x_debug_ssv_part_tables and p7x_debug_ssv_merge_rows, no device."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_hmm
from pyhmmer_amd import _lib, easel, plan7

SSV_R = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 20, 24, 32, 48)       # the kernel's instantiated registers per lane


def ssv_plan(M, pair, forced=0):
    lo, hi, R = (np.zeros(8, dtype=np.int32) for _ in range(3))
    P = _lib.lib().p7x_debug_ssv_plan(M, pair, forced, lo.ctypes.data, hi.ctypes.data, R.ctypes.data, 8)
    assert 1 <= P <= 8, _lib.last_error()
    return [(int(lo[q]), int(hi[q]), int(R[q])) for q in range(P)]


def holds(R, top):
    """R registers per lane hold cells up to <top> in both row parities (the kernel's layout: 64 R global registers, register
    g = cells (2g - 1, 2g) on odd rows and (2g, 2g + 1) on even ones)."""
    return (top + 1) // 2 + 1 <= 64 * R


@pytest.mark.parametrize("M", [2, 60, 1203, 6141, 6142, 6143, 8190, 12282, 12283, 12284, 12288])
def test_plan_tiles_the_model(libp7x, M):
    for pair in (0, 1):
        for forced in (0, 2, 3, 4):
            parts = ssv_plan(M, pair, forced)
            assert parts[0][0] == 1 and parts[-1][1] == M
            for (_, hi, _), (lo, _, _) in zip(parts, parts[1:]):
                assert lo == hi + 1                                   # every node once, in order
            for lo, hi, R in parts:
                assert lo <= hi and R in SSV_R
            for lo, hi, R in parts[:-1]:
                assert hi - lo + 1 <= 128 * R - 2                     # the last node of a part with a successor, in both parities
            lo, hi, R = parts[-1]
            assert holds(R, hi - lo + 1 + pair)
            if forced and M >= 2 * forced and M <= forced * 6141:
                assert len(parts) == forced
            if M <= 6141 and not forced:
                assert len(parts) == 1 and R == [r for r in SSV_R if holds(r, M + pair)][0]
            if not forced:                                            # the fewest parts: one part less of the widest kernel does not hold M
                P = len(parts)
                assert P == 1 or (P - 2) * 6142 + (6142 - pair) < M
    assert len(ssv_plan(12288, 1)) == 3 and len(ssv_plan(12284, 0)) == 2


def test_plan_of_one_part_is_the_single_launch(libp7x):
    """For M <= 6,141 the unforced plan is one part with the R that p7x_debug_ssv_tables reports (nothing changes for those
    models); one node beyond the library's limit is refused with the text of every such refusal."""
    abc = easel.Alphabet.dna()
    for M in (60, 1203, 6141):
        hmm = random_hmm(M, seed=4000 + M, alphabet=abc)
        om = plan7.OptimizedProfile(hmm, plan7.Background(abc), 400)
        for pair in (0, 1):
            R, slack = C.c_int32(), C.c_int32()
            assert _lib.lib().p7x_debug_ssv_tables(om._handle, pair, C.byref(R), C.byref(slack), None, 0) > 0, _lib.last_error()
            assert ssv_plan(M, pair) == [(1, M, R.value)]
    limit = _lib.lib().p7x_max_model_length()
    assert limit == 12288
    assert len(ssv_plan(limit, 1)) >= 2
    assert _lib.lib().p7x_debug_ssv_plan(limit + 1, 1, 0, None, None, None, 0) < 0
    assert f"(M > {limit} nodes)" in _lib.last_error() and "6141" not in _lib.last_error()


@pytest.mark.parametrize("M", [6142, 12288])
def test_part_tables_against_the_oracle_profile(libp7x, oracle, M):
    """The table of every part (p7x_debug_ssv_part_tables), as test_ssv_scan_tables_against_the_oracle_profile checks the
    table of a whole model: cell c of a part of nodes lo .. hi is node lo - 1 + c, every packed pair is bias - rb[x][k] of the
    oracle's pressed-format byte costs at the global node, -512 outside the part -- cell 0, where the kernel puts the cut
    node's score, included -- and the virtual node (emission 0) follows the last node of the last part only."""
    abc = easel.Alphabet.dna()
    hmm = random_hmm(M, seed=4000 + M, alphabet=abc)
    bg = plan7.Background(abc)
    om = plan7.OptimizedProfile(hmm, bg, 400)
    op = oracle.OracleProfile(hmm, bg, 400)
    Q, bias = int(op.p.Q16), int(op.p.bias_b)
    rbv = np.asarray(op.arr("rbv")).astype(np.int64)
    k = np.arange(1, M + 1)
    sval = np.full((4, M + 3), -512, dtype=np.int64)
    sval[:, 1:M + 1] = bias - rbv[:4, ((k - 1) % Q) * 16 + (k - 1) // Q]
    for pair in (0, 1):
        parts = ssv_plan(M, pair)
        assert len(parts) >= 2 or (M == 6142 and not pair)
        for q, (plo, phi, pR) in enumerate(parts):
            lo_, hi_, R_ = C.c_int32(), C.c_int32(), C.c_int32()
            n = _lib.lib().p7x_debug_ssv_part_tables(om._handle, pair, 0, q, C.byref(lo_), C.byref(hi_), C.byref(R_), None, 0)
            assert n > 0, _lib.last_error()
            assert (lo_.value, hi_.value, R_.value) == (plo, phi, pR)
            tab = np.zeros(n, dtype=np.uint32)
            assert _lib.lib().p7x_debug_ssv_part_tables(om._handle, pair, 0, q, None, None, None, tab.ctypes.data, n) == n
            R, R4 = pR, (pR + 3) // 4
            assert n == 2 * 4 * R4 * 64 * 4
            t = tab.reshape(2, 4, R4, 64, 4)
            lo = (t & 0xffff).astype(np.int64); lo[lo >= 32768] -= 65536
            hi = (t >> 16).astype(np.int64); hi[hi >= 32768] -= 65536
            last = q + 1 == len(parts)
            # what every cell of the layout must hold, cells -1 .. 128 R
            cells = np.arange(-1, 128 * R + 1)
            node = plo - 1 + cells
            want = np.full((4, len(cells)), -512, dtype=np.int64)
            inside = (node >= plo) & (node <= phi)
            want[:, inside] = sval[:, node[inside]]
            if pair and last:
                want[:, node == phi + 1] = 0
            assert (want[:, cells == 0] == -512).all()
            j = np.arange(R)
            for par in (0, 1):
                for lane in range(64):
                    g = lane * R + j
                    c0 = 2 * g - 1 if par == 0 else 2 * g
                    for x in range(4):
                        assert np.array_equal(lo[par, x, j // 4, lane, j % 4], want[x, c0 + 1]), (pair, q, par, x, lane)
                        assert np.array_equal(hi[par, x, j // 4, lane, j % 4], want[x, c0 + 2]), (pair, q, par, x, lane)
                if 4 * R4 > R:
                    jj = np.arange(R, 4 * R4)
                    assert not t[par][:, jj // 4, :, jj % 4].any()
    assert _lib.lib().p7x_debug_ssv_part_tables(om._handle, 1, 0, 7, None, None, None, None, 0) < 0


def merge(Q16, recs):
    n = len(recs)
    pos = np.array([r[0] for r in recs], dtype=np.int64); strand = np.array([r[1] for r in recs], dtype=np.int32)
    k = np.array([r[2] for r in recs], dtype=np.int32); sc = np.array([r[3] for r in recs], dtype=np.int32)
    opos = np.zeros(n, dtype=np.int64); ostrand, ok, osc = (np.zeros(n, dtype=np.int32) for _ in range(3))
    m = _lib.lib().p7x_debug_ssv_merge_rows(Q16, n, pos.ctypes.data, strand.ctypes.data, k.ctypes.data, sc.ctypes.data,
                                            opos.ctypes.data, ostrand.ctypes.data, ok.ctypes.data, osc.ctypes.data)
    assert 0 <= m <= n, _lib.last_error()
    return [(int(opos[i]), int(ostrand[i]), int(ok[i]), int(osc[i])) for i in range(m)]


def test_merge_of_the_parts_rows(libp7x):
    """One row per (strand, position): the highest byte score; on a tie -- scores saturate at 255 -- the node that comes first
    as p7_SSVFilter_longtarget unstripes the row, key ((k - 1) % Q16) * 16 + (k - 1) / Q16, with the whole model's Q16."""
    Q16 = 768                                                   # M = 12288
    key = lambda k: ((k - 1) % Q16) * 16 + (k - 1) // Q16
    recs = [
        (500, 0, 4100, 240), (500, 0, 9000, 251),               # two parts, different scores: the higher one
        (700, 0, 5000, 255), (700, 0, 770, 255), (700, 0, 12000, 255),   # all saturated: node 770 = vector 1, byte 1 comes first
        (900, 0, 8000, 249),                                    # one part only
        (500, 1, 9000, 240), (500, 1, 4100, 251),               # the other strand, the same position: rows of their own
        (100, 1, 3, 255), (100, 1, 769, 255),                   # key(3) = 32, key(769) = 1: the later node wins the tie
        (900, 0, 8000, 249),                                    # a part that saw the same cell (the cut node, reported by both sides)
    ]
    assert key(770) < key(5000) < key(12000) and key(769) < key(3)
    want = [(500, 0, 9000, 251), (700, 0, 770, 255), (900, 0, 8000, 249), (100, 1, 769, 255), (500, 1, 4100, 251)]
    assert merge(Q16, recs) == want
    assert merge(Q16, recs[::-1]) == want                       # whatever order the device wrote them in
    assert merge(Q16, []) == []
    assert merge(Q16, [(5, 0, 1, 200)]) == [(5, 0, 1, 200)]
