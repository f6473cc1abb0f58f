"""The row order of p7x_vitpk.hip::vit_row, restated in numpy (tests/vit_row_emu.py), against the oracle's scalar
recurrence, without a GPU: the first closure pass inside the register loop, the D->D exit on the stripe shift, the pass
loop entered from there.  Models and targets are those of tests/test_gpu_vit_row.py (gap-rich models; corridors that
start at node P, P + 1 and 2P + 1), a dozen bridge targets each and one mover; and the same targets must change their
score when the pass loop is left out (the in-loop pass alone is not the closure), else they would not test it."""
import numpy as np
import pytest

import gap_models
import vit_row_emu
import test_gpu_vit_row as cases
from pyhmmer_amd import plan7

TILES = [(8, 2), (8, 4), (8, 10), (8, 17), (16, 11), (16, 20)]


def _profile(hmm, oracle):
    return oracle.OracleProfile(hmm, plan7.Background(hmm.alphabet), 400)


@pytest.mark.parametrize("T,P", TILES)
def test_row_order_agrees_with_the_scalar_oracle_on_gap_rich_models(T, P, oracle):
    M = cases.served(T, P)[1]
    hmm = gap_models.gappy_hmm(M, seed=cases.SEED_MODEL + M)
    op = _profile(hmm, oracle)
    targets = gap_models.bridge_targets(hmm, 12, seed=cases.SEED_TARGETS + M)
    if M <= 160:
        targets.append(cases.mover_targets(hmm, op, 1, cases.SEED_TARGETS + M)[0][0])
    passes, cut = [], 0
    for s in targets:
        want = op.vit(s.sequence, scalar=True)[2]
        assert vit_row_emu.vit_row_order(op, s.sequence, T, P, passes) == want, s.name
        cut += want < 32767 and vit_row_emu.vit_row_order(op, s.sequence, T, P, skip_pass_loop=True) != want
    print(f"<{T}, {P}> M={M}: {cut} of {len(targets)} targets change without the pass loop; passes per asking row {np.mean(passes):.2f}, deepest {max(passes)}")
    assert cut >= 3 and max(passes) <= 2 * T


@pytest.mark.parametrize("T,P", TILES)
def test_row_order_with_a_corridor_that_starts_at_a_stripe_boundary(T, P, oracle):
    for c0 in (P, P + 1, 2 * P + 1):
        M = 2 * T * P
        hmm = cases.boundary_hmm(M, P, c0, seed=cases.SEED_MODEL + M + c0)
        op = _profile(hmm, oracle)
        for s in cases.boundary_targets(hmm, 8, seed=cases.SEED_TARGETS + M):
            assert vit_row_emu.vit_row_order(op, s.sequence, T, P) == op.vit(s.sequence, scalar=True)[2], (c0, s.name)
