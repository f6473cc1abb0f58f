"""The packed Viterbi filter for models of 641 to 2,048 nodes (p7x_vitpk.hip: vitpk_kernel<32, P>, two targets per
wavefront, and vitpk_kernel<64, P>, one), on the gap-rich models of tests/gap_models.py.

Every new instantiation runs the largest and the smallest model it serves; 2,049 nodes is the first length that stays
with the wave-per-target kernel.  A model's deletion corridors are longer than three times the wave-per-target kernel's
nodes per lane (11 to 32 here), and a stripe of the packed kernel is P <= 20 nodes, so a target that deletes a corridor
carries D across more than three stripes and the closure needs several passes.  The block holds bridge targets with
background neighbours, random targets, and the lengths at which the residue fetch of 4T rows changes: 1, 4T - 1, 4T,
4T + 1 and 8T + 1 rows for T = 32 and for T = 64.  Their number is odd: the last wavefront of <32, P> holds one target
and a masked group.  The oracle's scalar recurrence is the authority; every comparison is integer equality of xC.

The informativeness condition of tests/test_gpu_vit_gaps.py holds for every model below with the oracle alone (checked
on the CPU for these seeds: 61 to 71 of the 197 targets score above every background target and below 32,767)."""
import functools

import numpy as np
import pytest

import gap_models
from conftest import synthetic_block
from pyhmmer_amd import easel, hmmer, plan7

pytestmark = pytest.mark.gpu

P32 = tuple(range(11, 21))          # vitpk_pick: T = 32 serves M <= 64 P, T = 64 serves M <= 128 P
P64 = tuple(range(11, 17))
EDGE_LENGTHS = (1, 127, 128, 129, 257, 255, 256, 513)      # 4T - 1, 4T, 4T + 1, 8T + 1 for T = 32 and T = 64


def _range_ends():
    """(M, T, P): the smallest and the largest model of every new instantiation; (2049, 0, 0) stays with vit_kernel."""
    out, prev = [], 640
    for T, plist in ((32, P32), (64, P64)):
        for P in plist:
            out += [(prev + 1, T, P), (2 * T * P, T, P)]
            prev = 2 * T * P
    assert {641, 1280, 1281, 2048} <= {m for m, _, _ in out} and len(out) == 32
    return out + [(2049, 0, 0)]


CASES = _range_ends()
IDS = [f"M{m}-T{t}-P{p}" if t else f"M{m}-wave" for m, t, p in CASES]


@functools.lru_cache(maxsize=None)
def _case(M):
    """Model, block and the oracle's scalar scores, computed once for both settings of "vit_wide"."""
    import oracle_lib
    hmm = gap_models.gappy_hmm(M, seed=5000 + M)
    bg = plan7.Background(hmm.alphabet)
    rng = np.random.default_rng(M)
    seqs = gap_models.with_background_neighbours(gap_models.bridge_targets(hmm, 80, seed=M), seed=M)
    lengths = list(rng.integers(1, 421, size=29)) + list(EDGE_LENGTHS)
    seqs += list(synthetic_block(len(lengths), 0, seed=M, alphabet=hmm.alphabet, lengths=lengths))
    assert len(seqs) == 197 and {len(s) for s in seqs} >= set(EDGE_LENGTHS)
    built = np.array([s.name.startswith("bridge") for s in seqs])
    blk = easel.DigitalSequenceBlock(hmm.alphabet, seqs)
    op = oracle_lib.OracleProfile(hmm, bg, 400)
    want = np.array([op.vit(s.sequence, scalar=True)[2] for s in seqs])
    want.setflags(write=False)
    return hmm, bg, blk, built, want


def _informative(built, want):
    background_max = int(want[~built].max())
    return int(((want > background_max) & (want < 32767)).sum()), background_max


def _xc(hmm, bg, blk, wide):
    """xC of the lane family ("small_block" = 0) with "vit_wide" as given.  The packed tables are laid out when a
    profile's device image is built, so every setting gets a profile of its own."""
    from pyhmmer_amd import _lib
    _lib.set_debug_option("small_block", 0)
    _lib.set_debug_option("vit_wide", wide)
    try:
        om = plan7.OptimizedProfile(hmm, bg, 400)
        return plan7.SequenceDatabase(blk).filters(om, msv=False, viterbi=True)["xC"]
    finally:
        _lib.set_debug_option("vit_wide", -1)
        _lib.set_debug_option("small_block", -1)


@pytest.mark.parametrize("M,T,P", CASES, ids=IDS)
def test_every_wide_instantiation_at_both_ends_of_its_range(M, T, P):
    hmm, bg, blk, built, want = _case(M)
    informative, background_max = _informative(built, want)
    assert 4 * informative >= len(blk), (informative, len(blk), background_max)
    for rep in range(2):
        got = _xc(hmm, bg, blk, -1)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"M={M} (T, P)=({T}, {P}) rep={rep}: {bad.size} differ from the scalar oracle, first "
                               f"{[(blk[int(i)].name, len(blk[int(i)]), int(got[i]), int(want[i])) for i in bad[:5]]}")


@pytest.mark.parametrize("M,T,P", CASES, ids=IDS)
def test_vit_wide_off_gives_the_same_scores(M, T, P):
    """Option "vit_wide" = 0 sends the models beyond 640 nodes to vit_kernel, as before the wide instantiations."""
    hmm, bg, blk, built, want = _case(M)
    narrow, wide = _xc(hmm, bg, blk, 0), _xc(hmm, bg, blk, 1)
    assert np.array_equal(narrow, wide), np.nonzero(narrow != wide)[0][:8]
    assert np.array_equal(narrow, want)


def _planted_block(hmms, n, seed):
    """n background targets of 40 to 600 residues; every eighteenth carries a domain: the consensus of 60 to 160
    consecutive nodes of one of the models, one residue in seven redrawn, or a bridge target of that model."""
    abc = hmms[0].alphabet
    rng = np.random.default_rng(seed)
    filler = synthetic_block(n, 0, seed=seed, alphabet=abc, lengths=rng.integers(40, 601, size=n))
    bridges = {h.M: gap_models.bridge_targets(h, 8, seed=seed) for h in hmms}
    seqs, nplanted = [], 0
    for i, f in enumerate(filler):
        x = np.array(f.sequence)
        if i % 18 == 0:
            h = hmms[(i // 18) % len(hmms)]
            if (i // 18) % 3 == 2:
                dom = np.array(bridges[h.M][(i // 18) % 8].sequence)
            else:
                cons = np.array([abc.symbols.index(c.upper()) for c in h.consensus], dtype=np.uint8)
                w = int(rng.integers(60, 161))
                a = int(rng.integers(0, h.M - min(w, h.M) + 1))
                dom = cons[a:a + w].copy()
                redraw = rng.random(dom.size) < 1.0 / 7.0
                dom[redraw] = rng.integers(0, abc.K, size=int(redraw.sum()))
            at = int(rng.integers(0, 20))
            x = np.concatenate([x[:at], dom, x[at:]])
            nplanted += 1
        seqs.append(easel.DigitalSequence(abc, name=f"t{i}", sequence=x.astype(np.uint8)))
    return easel.DigitalSequenceBlock(abc, seqs), nplanted


def test_mixed_batch_gives_the_same_hits_with_and_without_the_wide_kernels():
    """Four profiles of 100, 700, 1,300 and 2,048 nodes in one batch (<8, 8>, <32, 11>, <64, 11>, <64, 16>) against 2,001
    targets with planted domains: stage counts and hits (names, scores, domain coordinates) with "vit_wide" 1 and 0.
    "small_block" = 0 picks the lane kernels whatever the number of compute units (a block of 2,001 targets would
    otherwise count as small on a 256-CU device)."""
    from pyhmmer_amd import _lib
    hmms = [gap_models.gappy_hmm(M, seed=5000 + M) for M in (100, 700, 1300, 2048)]
    blk, nplanted = _planted_block(hmms, 2001, seed=17)
    assert nplanted >= 100

    def search(wide):
        _lib.set_debug_option("small_block", 0)
        _lib.set_debug_option("vit_wide", wide)
        try:
            out = []
            for hits in hmmer.hmmsearch(hmms, blk, batch=4):
                out.append((dict(hits.stage_counts),
                            [(h.name, h.score, [(d.env_from, d.env_to, d.alignment.target_from, d.alignment.target_to,
                                                 d.alignment.hmm_from, d.alignment.hmm_to, d.score) for d in h.domains])
                             for h in hits]))
            return out
        finally:
            _lib.set_debug_option("vit_wide", -1)
            _lib.set_debug_option("small_block", -1)

    wide, narrow = search(1), search(0)
    assert len(wide) == len(narrow) == 4
    for hmm, w, n in zip(hmms, wide, narrow):
        assert w[0] == n[0], (hmm.M, w[0], n[0])
        assert w[1] == n[1], hmm.M
        assert len(w[1]) >= 5, (hmm.M, len(w[1]), w[0])          # the planted domains are found: the comparison is about something
