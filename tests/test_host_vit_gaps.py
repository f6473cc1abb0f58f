"""The inputs of tests/test_gpu_vit_gaps.py, checked without a GPU: on the gap-rich models of tests/gap_models.py the three
CPU statements of the Viterbi filter agree (striped oracle, scalar oracle, numpy restatement of the packed kernel),
and the targets DISCRIMINATE: their scores are below saturation and change when the D->D closure of the packed
kernel is cut short, or when the model loses its D->D chains.  A kernel whose cross-stripe carry were wrong from its
second pass on could not pass the GPU file on these targets; on conftest.random_hmm models it could."""
import functools

import numpy as np
import pytest

import gap_models
import vit_striped_emu
from pyhmmer_amd import plan7

NTARGETS = 60


@functools.lru_cache(maxsize=None)
def _measure(M, T, P):
    """Per target of the model: xC of the striped oracle, the scalar oracle and the emulator; the emulator's xC with the
    closure stopped after one and after two passes; and every closure's pass count."""
    import oracle_lib
    assert gap_models.packed_shape(M) == (T, P)
    hmm = gap_models.gappy_hmm(M, seed=5000 + M)
    op = oracle_lib.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400)
    targets = gap_models.bridge_targets(hmm, NTARGETS, seed=M)
    assert max(len(s) for s in targets) <= 70
    passes = []
    cols = {k: [] for k in ("striped", "scalar", "emu", "cap1", "cap2")}
    for s in targets:
        cols["striped"].append(op.vit(s.sequence)[2])
        cols["scalar"].append(op.vit(s.sequence, scalar=True)[2])
        cols["emu"].append(vit_striped_emu.vit_striped(op, s.sequence, T, P, passes))
        cols["cap1"].append(vit_striped_emu.vit_striped(op, s.sequence, T, P, max_pass=1))
        cols["cap2"].append(vit_striped_emu.vit_striped(op, s.sequence, T, P, max_pass=2))
    return {k: np.array(v) for k, v in cols.items()}, passes


PACKED = [(32, 8, 2), (262, 8, 17), (320, 8, 20), (352, 16, 11), (640, 16, 20)]


@pytest.mark.parametrize("M,T,P", PACKED)
def test_the_three_cpu_viterbi_filters_agree_on_gap_rich_models(M, T, P, oracle):
    sc, _ = _measure(M, T, P)
    assert np.array_equal(sc["striped"], sc["scalar"]), np.nonzero(sc["striped"] != sc["scalar"])[0]
    assert np.array_equal(sc["emu"], sc["scalar"]), np.nonzero(sc["emu"] != sc["scalar"])[0]


@pytest.mark.parametrize("M,T,P", PACKED)
def test_bridge_targets_depend_on_the_later_closure_passes(M, T, P, oracle):
    """Measured (seed 5000 + M, 60 targets): non-overflowing / changed after one pass / after two / deepest closure
      M =  32 (8, 2)    47 / 47 / 47 / 11        M = 352 (16, 11)  40 / 40 / 40 / 9
      M = 262 (8, 17)   44 / 44 / 44 /  8        M = 640 (16, 20)  51 / 51 / 51 / 9
      M = 320 (8, 20)   49 / 49 / 49 /  6
    against 0 / 0 at P >= 17 on conftest.random_hmm models.  The bounds below are conditions on the generator."""
    sc, passes = _measure(M, T, P)
    ok = sc["scalar"] < 32767
    cap1, cap2 = int((ok & (sc["cap1"] != sc["scalar"])).sum()), int((ok & (sc["cap2"] != sc["scalar"])).sum())
    print(f"M={M} (T, P)=({T}, {P}): {int(ok.sum())} of {NTARGETS} below saturation, {cap1} change with the closure stopped "
          f"after 1 pass, {cap2} after 2 passes; deepest closure {max(passes)} passes (2T = {2 * T})")
    assert 2 * int(ok.sum()) >= NTARGETS
    assert cap1 >= 10
    assert cap2 >= 4
    assert 3 <= max(passes) <= 2 * T


@pytest.mark.parametrize("M", [641, 1000, 2049])
def test_bridge_targets_of_wave_kernel_models_score_through_the_delete_chain(M, oracle):
    """Models beyond the packed kernel: every corridor is longer than three times the wave-per-target kernel's nodes per
    lane, so a target that deletes one carries D across more than two lane boundaries.  The score of such a target must
    change when the model loses its D->D chains (tDD = 1e-6, the mass moved into D->M)."""
    hmm = gap_models.gappy_hmm(M, seed=5000 + M)
    C = gap_models.wave_nodes_per_lane(M)
    assert all(c1 - c0 + 1 > 2 * C for c0, c1 in gap_models.corridors(hmm))
    bg = plan7.Background(hmm.alphabet)
    op = oracle.OracleProfile(hmm, bg, 400)
    flat = oracle.OracleProfile(gap_models.without_delete_chains(hmm), bg, 400)
    targets = gap_models.bridge_targets(hmm, NTARGETS, seed=M)
    xc = np.array([op.vit(s.sequence)[2] for s in targets])
    assert np.array_equal(xc, [op.vit(s.sequence, scalar=True)[2] for s in targets])
    ok = xc < 32767
    uses_chain = int((ok & (xc != np.array([flat.vit(s.sequence)[2] for s in targets]))).sum())
    print(f"M={M} (C = {C}): {int(ok.sum())} of {NTARGETS} below saturation, {uses_chain} of them score through a D->D chain")
    assert 2 * int(ok.sum()) >= NTARGETS
    assert uses_chain >= 10


def test_generator_follows_its_description():
    """Corridors of at least 3P nodes with tDD >= 0.95 and a cheap way in, insert-rich nodes, rows that sum to one, the
    boundary conventions of conftest.random_hmm; neighbours of the same length."""
    for M in (31, 262, 640, 1000):
        hmm = gap_models.gappy_hmm(M, seed=5000 + M)
        t = np.asarray(hmm.transition_probabilities, dtype=np.float64)
        cors = gap_models.corridors(hmm)
        assert cors
        for c0, c1 in cors:
            assert c1 - c0 >= 3 * gap_models.stripe_nodes(M) and c0 >= 10 and c1 + 9 <= M
            assert t[c0:c1, gap_models.DD].min() >= 0.9499 and t[c0 - 1, gap_models.MD] >= 0.2999
        rich = gap_models.insert_rich(hmm)
        assert rich and all(t[k, gap_models.MI] >= 0.199 and t[k, gap_models.II] >= 0.899 for k in rich)
        assert np.allclose(t[:, 0:3].sum(axis=1), 1.0, atol=1e-6) and np.allclose(t[:, 3:5].sum(axis=1), 1.0, atol=1e-6)
        assert np.allclose(t[:, 5:7].sum(axis=1), 1.0, atol=1e-6)
        assert t[M, gap_models.MD] == 0.0 and t[M, gap_models.DD] == 0.0 and t[0, gap_models.DD] == 0.0
        targets = gap_models.bridge_targets(hmm, 20, seed=1)
        both = gap_models.with_background_neighbours(targets, seed=1)
        assert len(both) == 40 and all(len(both[2 * i]) == len(both[2 * i + 1]) for i in range(20))
        assert [s.name for s in both[0::2]] == [s.name for s in targets]
