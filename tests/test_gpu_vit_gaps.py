"""The Viterbi filter kernels on gap-rich models, where the D->D chain decides the score (tests/gap_models.py).

The instantiation sweeps of tests/test_gpu_filters.py draw deletion-poor models and mostly saturated homologs: a
packed kernel (p7x_vitpk.hip) whose cross-stripe carry were wrong from the second closure pass on, or a wave-per-target
kernel (p7x_vitfwd.hip: vit_kernel) that lost a carry between lanes, would pass them.  Here every model has deletion
corridors longer than three stripes, every built target scores by deleting one, stays below saturation, and shares its
wavefront with a background target of the same length (the carry restricted to the targets that asked for the
closure).  tests/test_host_vit_gaps.py shows on the CPU that these scores change when the closure stops early.
The plain scalar recurrence of the oracle is the final authority for xC."""
import functools

import numpy as np
import pytest

import gap_models
from conftest import synthetic_block
from pyhmmer_amd import easel, plan7

pytestmark = pytest.mark.gpu

FWD_TOL_NATS = 2e-3      # as tests/test_gpu_filters.py: |fwd_gpu - fwd_oracle| in nats, plus 1e-5 |fwd|


@pytest.fixture(params=["one-target-per-wavefront kernels for small blocks", "lane-per-target kernels"])
def kernel_family(request):
    """As in tests/test_gpu_filters.py: small blocks take the wave-per-target MSV / Viterbi kernels, option "small_block"
    = 0 sends the same block through the lane-per-target MSV and the packed Viterbi kernels (M <= 640)."""
    from pyhmmer_amd import _lib
    _lib.set_debug_option("small_block", 0 if request.param.startswith("lane") else -1)
    yield request.param
    _lib.set_debug_option("small_block", -1)


@functools.lru_cache(maxsize=None)
def _case(M):
    """Model, profile, block and the oracle's scores, computed once for both kernel families."""
    import oracle_lib
    hmm = gap_models.gappy_hmm(M, seed=5000 + M)
    bg = plan7.Background(hmm.alphabet)
    rng = np.random.default_rng(M)
    seqs = gap_models.with_background_neighbours(gap_models.bridge_targets(hmm, 120, seed=M), seed=M)
    seqs += list(synthetic_block(40, 0, seed=M, alphabet=hmm.alphabet, lengths=rng.integers(1, 421, size=40)))
    assert len(seqs) % 16 != 0                   # no multiple of the 4 * 64 / T targets of a packed block, T = 8 or 16
    built = np.array([s.name.startswith("bridge") for s in seqs])
    blk = easel.DigitalSequenceBlock(hmm.alphabet, seqs)
    op = oracle_lib.OracleProfile(hmm, bg, 400)
    want = {"xJ": op.msv_block(blk.packed()),
            "xC": np.array([op.vit(s.sequence)[2] for s in seqs]),
            "scalar": np.array([op.vit(s.sequence, scalar=True)[2] for s in seqs]),
            "fwd": np.array([op.fwd(s.sequence)[1] for s in seqs])}
    for v in want.values():
        v.setflags(write=False)
    return hmm, bg, blk, built, want


@pytest.mark.parametrize("M", [31, 32, 262, 271, 272, 320, 321, 352,
                               639, 640,                      # the packed kernel in the lane family, vit_kernel in the other
                               641, 1000, 2049, 4097])        # vit_kernel only; beyond 2,048 nodes its rolled loops
def test_viterbi_filter_on_deletion_corridors(M, kernel_family):
    hmm, bg, blk, built, want = _case(M)
    # the input must keep discriminating: a quarter of the block scores above every background target and below saturation
    background_max = int(want["scalar"][~built].max())
    informative = int(((want["scalar"] > background_max) & (want["scalar"] < 32767)).sum())
    assert 4 * informative >= len(blk), (informative, len(blk), background_max)
    om = plan7.OptimizedProfile(hmm, bg, 400)
    for rep in range(2):
        got = plan7.SequenceDatabase(blk).filters(om, msv=True, viterbi=True, forward=True)
        assert np.array_equal(got["xJ"], want["xJ"]), f"M={M} rep={rep}"
        bad = np.nonzero(got["xC"] != want["xC"])[0]
        assert bad.size == 0, f"M={M} rep={rep}: {bad.size} differ from the striped oracle, first {[(blk[int(i)].name, int(got['xC'][i]), int(want['xC'][i])) for i in bad[:5]]}"
        assert np.array_equal(got["xC"], want["scalar"]), f"M={M} rep={rep}"
        ok = np.isfinite(want["fwd"])
        assert np.array_equal(np.isfinite(got["fwd"]), ok)
        err = np.abs(got["fwd"][ok] - want["fwd"][ok])
        tol = FWD_TOL_NATS + 1e-5 * np.abs(want["fwd"][ok])
        assert np.all(err < tol), f"M={M} rep={rep}: Forward off by {float(err.max()):.2e} nats at worst"


def _seam_case():
    import oracle_lib
    M = 262
    hmm = gap_models.gappy_hmm(M, seed=5000 + M)
    abc = hmm.alphabet
    bg = plan7.Background(abc)
    rng = np.random.default_rng(262)
    motifs = gap_models.bridge_targets(hmm, 12, seed=9)
    seqs = []
    for i, (m, filler) in enumerate(zip(motifs, synthetic_block(12, 0, seed=8, alphabet=abc, lengths=rng.integers(2000, 5001, size=12)))):
        at = int(rng.integers(0, len(filler) - len(m)))
        x = np.array(filler.sequence)
        x[at:at + len(m)] = m.sequence
        seqs.append(easel.DigitalSequence(abc, name=f"long{i}", sequence=x))
    seqs += gap_models.with_background_neighbours(gap_models.bridge_targets(hmm, 150, seed=10), seed=10)
    lengths = sorted((len(s) for s in seqs), reverse=True)
    assert len(seqs) == 312 and lengths[11] >= 2000 > 768 > 3 * lengths[len(seqs) // 2] and lengths[4] > lengths[5]
    op = oracle_lib.OracleProfile(hmm, bg, 400)
    want = np.array([op.vit(s.sequence, scalar=True)[2] for s in seqs])
    assert np.array_equal(want, [op.vit(s.sequence)[2] for s in seqs])
    assert int((want[12:] < 32767).sum()) >= 150 and int((want[:12] < 32767).sum()) >= 6
    return hmm, bg, seqs, lengths, want


def test_long_target_seam_of_the_packed_kernel_on_a_gap_rich_model():
    """The longest targets of a database (the head of its length-sorted list) leave the packed kernel for vit_kernel, and
    the packed kernel starts behind them (nskip_ptr).  A dozen targets of 2,000-5,000 residues, each a bridge motif in
    background, and 300 short ones: every xC against the oracle, first with the database's own cut (all twelve long
    targets go to vit_kernel), then with option "vit_long_cut" set to the length of the sixth longest, so that five go
    there and the first wavefront of the packed kernel holds seven long targets and a short one."""
    from pyhmmer_amd import _lib
    hmm, bg, seqs, lengths, want = _seam_case()
    blk = easel.DigitalSequenceBlock(hmm.alphabet, seqs)
    om = plan7.OptimizedProfile(hmm, bg, 400)
    _lib.set_debug_option("small_block", 0)
    try:
        for cut in (-1, lengths[5]):
            _lib.set_debug_option("vit_long_cut", cut)
            db = plan7.SequenceDatabase(blk)            # the cut is taken when the database is built
            got = db.filters(om, msv=False, viterbi=True)["xC"]
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"cut={cut}: {[(seqs[int(i)].name, int(got[i]), int(want[i])) for i in bad[:8]]}"
    finally:
        _lib.set_debug_option("vit_long_cut", -1)
        _lib.set_debug_option("small_block", -1)
