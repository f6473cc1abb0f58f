"""The row loop of the lane-per-target MSV kernels (p7x_msv.hip: RowChunks, msv_fast_body, the tier kernels), at the smallest
shapes at which its order of reads, waits and rows can go wrong: one register tile with R % 8 == 4 and one with R % 8 == 0 at
both ends of every one-lane tier, and tiles of two, four and eight lanes per target.

130 targets per model: two full groups of 64 and a ragged one.  Lengths 0..40, 63, 64, 65, the rest 300, so that groups end
in the first and in the second half of their last 16-residue tile.  Every fourth target carries an ungapped stretch of the
model's consensus that ends at its last residue or at residue 8, 9, 16 or 17: the begin score moves (the re-bias branch of
the fast kernel) in the row next to a tile edge and in the last row.  One target is all '*': every row maximum stays below
the begin score, which the fast kernel cannot resolve, so its group is redone by the exact kernel.  Both conditions are
asserted from the oracle's own xJ.  Scores must equal the oracle's bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import random_hmm
from pyhmmer_amd import _lib, easel, plan7

pytestmark = pytest.mark.gpu

# the register tiles of p7x_msv.hip (P7X_TILES_TIER0..5) and msv_pick's rule, restated: the test needs a model length per tile
_R1 = list(range(8, 161, 4)) + [176, 192, 208, 224]
_R2 = list(range(120, 225, 8))
_R4 = [120, 128]
_R8 = list(range(64, 129, 8))


def msv_pick(M):
    need = (M + 1) // 2 + 1
    for K, rs in ((1, _R1), (2, _R2), (4, _R4)):
        for r in rs:
            if K * r >= need:
                return r, K
    for r in _R8:
        if 8 * r >= (M + 1) // 2:
            return r, 8
    return None


def msv_tier(R, K):
    if K == 1:
        return 0 if R <= 92 else (1 if R <= 136 else 2)
    return {2: 3, 4: 4, 8: 5}[K]


LARGEST_M = {}
for _M in range(1, 2049):
    LARGEST_M[msv_pick(_M)] = _M

TILES = [(8, 1), (12, 1), (88, 1), (92, 1), (96, 1), (100, 1), (132, 1), (136, 1), (140, 1), (224, 1),
         (120, 2), (224, 2), (120, 4), (128, 4), (64, 8), (128, 8)]
LENGTHS = list(range(0, 41)) + [63, 64, 65] + [300] * 86
AMBIGUOUS = 50                   # index of the all-'*' target (300 residues)
STRETCH_ENDS = (0, 8, 9, 16, 17)          # 0: at the target's last residue


@functools.lru_cache(maxsize=None)
def model(R, K, variant=0):
    M = LARGEST_M[(R, K)] - variant       # (variant 1: a second model of the same tile)
    assert msv_pick(M) == (R, K)
    hmm = random_hmm(M, seed=1000 + M)
    bg = plan7.Background(hmm.alphabet)
    return hmm, bg, plan7.OptimizedProfile(hmm, bg, 400)


@functools.lru_cache(maxsize=None)
def oracle_profile(R, K, variant=0):
    import oracle_lib
    hmm, bg, _ = model(R, K, variant)
    return oracle_lib.OracleProfile(hmm, bg, 400)


def _consensus(hmm):
    return np.argmax(hmm.match_emissions[1:], axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def stretch_length(R, K, variant=0):
    """The shortest consensus stretch at the end of a 300-residue background target that lifts xJ above base, by the oracle."""
    hmm, bg, om = model(R, K, variant)
    op = oracle_profile(R, K, variant)
    cons = _consensus(hmm)
    rng = np.random.default_rng(7)
    p = bg.residue_frequencies.astype(np.float64)
    seq = rng.choice(hmm.alphabet.K, size=300, p=p / p.sum()).astype(np.uint8)
    for n in range(4, min(hmm.M, 17) + 1):
        s = seq.copy()
        s[300 - n:] = cons[:n]
        if op.msv(s)[2] > om.base:
            return n
    return min(hmm.M, 17)


@functools.lru_cache(maxsize=None)
def block(keys):
    """The 130 targets; planted stretches come from the models <keys> in turn.  Returns the block and the oracle's xJ per model."""
    models = [model(*k) for k in keys]
    abc = models[0][0].alphabet
    rng = np.random.default_rng(len(keys) * 1000 + keys[0][0] * 10 + keys[0][1])
    p = models[0][1].residue_frequencies.astype(np.float64)
    p /= p.sum()
    seqs = []
    for t, L in enumerate(LENGTHS):
        x = rng.choice(abc.K, size=L, p=p).astype(np.uint8)
        if t == AMBIGUOUS:
            x[:] = 27
        elif t % 4 == 0 and L > 0:
            q = (t // 4) % len(keys)
            hmm = models[q][0]
            cons = _consensus(hmm)
            end = STRETCH_ENDS[(t // 4) % len(STRETCH_ENDS)]
            if end == 0 or end > L:
                end = L
            n = min(stretch_length(*keys[q]) + (t // 20) % 2, end, hmm.M)        # (some one residue longer: other maxima)
            k0 = int(rng.integers(0, hmm.M - n + 1))
            x[end - n:end] = cons[k0:k0 + n]
        seqs.append(easel.DigitalSequence(abc, name=f"t{t}", sequence=x))
    blk = easel.DigitalSequenceBlock(abc, seqs)
    want = [oracle_profile(*k).msv_block(blk.packed()) for k in keys]
    return blk, want


def check_conditions(key, want):
    """From the oracle's xJ: the re-bias branch ran in at least ten targets, and one group is ambiguous."""
    hmm, bg, om = model(*key)
    above = int(np.sum(want > om.base))
    assert above >= 10, (key, above)
    om300 = plan7.OptimizedProfile(hmm, bg, 300)          # the begin score of a 300-residue target
    F0 = max(om300.base - om300.tjb - om300.tbm, 0) - om300.tec
    assert F0 > 0 and 0 <= want[AMBIGUOUS] <= F0, (key, int(want[AMBIGUOUS]), F0)      # no row maximum above the begin score


@pytest.fixture
def lane_kernels():
    _lib.set_debug_option("small_block", 0)
    _lib.set_debug_option("msv_long_groups", 0)
    yield
    for name in ("small_block", "msv_long_groups", "msv_f16", "msv_exact"):
        _lib.set_debug_option(name, -1)


@pytest.mark.parametrize("R,K", TILES)
def test_per_tile_kernels_bit_exact(R, K, lane_kernels):
    blk, (want,) = block(((R, K),))
    check_conditions((R, K), want)
    om = model(R, K)[2]
    for flavour, options in (("half", {}), ("int16", {"msv_f16": 0}), ("exact", {"msv_exact": 1})):
        for name, value in options.items():
            _lib.set_debug_option(name, value)
        try:
            got = plan7.SequenceDatabase(blk).filters(om, msv=True)["xJ"]
        finally:
            for name in options:
                _lib.set_debug_option(name, -1)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (R, K, flavour, bad[:8], got[bad[:8]], want[bad[:8]])


# three profiles of one tier and one of another: a batch needs two classes to take the tier launches
TIER_BATCHES = [
    ((8, 1), (12, 1), (92, 1), (96, 1)),
    ((88, 1), (92, 1), (12, 1), (140, 1)),
    ((96, 1), (100, 1), (136, 1), (8, 1)),
    ((132, 1), (136, 1), (100, 1), (120, 2)),
    ((140, 1), (224, 1), (140, 1, 1), (88, 1)),
    ((120, 2), (224, 2), (120, 2, 1), (132, 1)),
    ((120, 4), (128, 4), (120, 4, 1), (64, 8)),
    ((64, 8), (128, 8), (64, 8, 1), (120, 4)),
]


@pytest.mark.parametrize("keys", TIER_BATCHES, ids=lambda ks: "+".join(f"{k[0]}x{k[1]}" for k in ks))
def test_tier_kernels_bit_exact(keys, lane_kernels):
    assert len({msv_tier(*k[:2]) for k in keys[:3]}) == 1 and msv_tier(*keys[3][:2]) != msv_tier(*keys[0][:2])
    blk, want = block(keys)
    abc = model(*keys[0])[0].alphabet
    pli = plan7.Pipeline(abc)
    oms = [model(*k)[2] for k in keys]
    db = plan7.SequenceDatabase(blk)
    nq, n = len(oms), len(blk)
    handles = (C.c_void_p * nq)(*[om._handle for om in oms])
    bgf = np.ascontiguousarray(pli.background.residue_frequencies, dtype=np.float32)
    cfg = pli._cfg()
    xJ, xC, stage = np.zeros((nq, n), dtype=np.int32), np.zeros((nq, n), dtype=np.int32), np.zeros((nq, n), dtype=np.uint8)
    st = _lib.lib().p7x_search_batch_raw(C.byref(cfg), handles, nq, bgf.ctypes.data, db._handle, xJ.ctypes.data, xC.ctypes.data, stage.ctypes.data)
    assert st == 0, _lib.last_error()
    for q, key in enumerate(keys):
        bad = np.nonzero(xJ[q] != want[q])[0]
        assert bad.size == 0, (key, bad[:8], xJ[q][bad[:8]], want[q][bad[:8]])
