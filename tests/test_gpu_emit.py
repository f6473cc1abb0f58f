"""HMM.emit_block on the device (p7x_emit.hip) against its host twin (test seam "host_emit" = 1): the same tables, the same
counter-based generator, comparisons only -- so the same bytes, lengths, attempts and traces, for every shape at which
the kernel takes another path: a partial wavefront, exactly one, one over, several blocks; tables in LDS and tables read
through L2; slots that hold their sequence and slots that do not (second launch)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, hmmer, plan7
from test_host_emit import all_delete_hmm, check_paths, long_insert_hmm, sampled

pytestmark = pytest.mark.gpu


def both(hmm, N, *, seed=42, traces=True, cap=-1, lds=-1):
    """(the device's block, the host twin's) under the same options."""
    _lib.set_debug_option("emit_cap", cap)
    _lib.set_debug_option("emit_lds", lds)
    try:
        dev = hmm.emit_block(N, seed=seed, traces=traces)
        _lib.set_debug_option("host_emit", 1)
        twin = hmm.emit_block(N, seed=seed, traces=traces)
    finally:
        for name in ("host_emit", "emit_cap", "emit_lds"):
            _lib.set_debug_option(name, -1)
    assert dev.on_device and not twin.on_device
    return dev, twin


def assert_same(dev, twin):
    assert len(dev) == len(twin) and dev.cap == twin.cap and dev.redrawn == twin.redrawn
    for name in ("lengths", "offsets", "attempts", "states", "nodes"):
        a, b = getattr(dev, name), getattr(twin, name)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), name
    assert np.array_equal(dev.block.packed().dsq, twin.block.packed().dsq)


MODELS = {
    "M1": lambda: sampled(1, 3),
    "M2": lambda: sampled(2, 4),
    "gaps": all_delete_hmm,                                      # attempts > 0 for one sequence in six
    "amino300": lambda: random_hmm(300, 8),                      # 106 KB of tables: read through L2
    "dna": lambda: random_hmm(50, 3, alphabet=easel.Alphabet.dna()),
}


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_device_equals_host_twin(libp7x, name, N):
    hmm = MODELS[name]()
    dev, twin = both(hmm, N)
    assert_same(dev, twin)
    if N:
        check_paths(hmm, dev)
    if name == "gaps" and N == 1000:
        assert (dev.attempts > 0).any()


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1000])
def test_overflowed_slots_are_redrawn_in_a_second_launch(libp7x, N):
    hmm = long_insert_hmm()
    dev, twin = both(hmm, N, cap=8)
    assert_same(dev, twin)
    assert dev.cap == 8 and dev.redrawn == int((dev.lengths > 8).sum()) and (dev.redrawn > N // 2 or N == 0)
    whole, _ = both(hmm, N)                                      # the default slots: the same sequences
    assert np.array_equal(whole.block.packed().dsq, dev.block.packed().dsq) and np.array_equal(whole.nodes, dev.nodes)
    plain, twin = both(hmm, N, cap=8, traces=False)
    assert plain.states is None and np.array_equal(plain.block.packed().dsq, dev.block.packed().dsq)


@pytest.mark.parametrize("redrawn", [63, 64, 65])
def test_second_launch_of_a_partial_a_whole_and_one_wavefront_over(libp7x, redrawn):
    """The second launch runs one lane per sequence that outgrew its slot: N is chosen, from the twin's lengths (sequence i
    does not depend on N), so that exactly 63, 64 and 65 of them do."""
    hmm = long_insert_hmm()
    _, twin = both(hmm, 200, cap=8)
    N = int(np.searchsorted(np.cumsum(twin.lengths > 8), redrawn)) + 1
    assert N <= 200
    dev, twin = both(hmm, N, cap=8)
    assert dev.redrawn == redrawn
    assert_same(dev, twin)
    check_paths(hmm, dev)


def test_longest_model(libp7x):
    hmm = random_hmm(libp7x.p7x_max_model_length(), 21)
    dev, twin = both(hmm, 8)
    assert_same(dev, twin)
    check_paths(hmm, dev)
    longer = random_hmm(libp7x.p7x_max_model_length() + 1, 21)
    with pytest.raises(ValueError):
        longer.emit_block(8)


def test_tables_in_lds_or_through_l2(libp7x):
    hmm = sampled(40, 6)                                         # 15 KB of tables: staged in LDS unless told otherwise
    in_lds, twin = both(hmm, 300)
    through_l2, _ = both(hmm, 300, lds=0)
    assert_same(in_lds, twin)
    assert_same(through_l2, twin)


def test_sequence_does_not_depend_on_the_launch(libp7x):
    hmm = load_hmms("PF02826")[0]
    few, many = hmm.emit_block(65, seed=7), hmm.emit_block(1000, seed=7)
    assert few.on_device and many.on_device
    for i in range(65):
        assert np.array_equal(few[i].sequence, many[i].sequence)
    assert not np.array_equal(hmm.emit_block(65, seed=8)[0].sequence, few[0].sequence)


def test_round_trip_through_hmmsearch(libp7x):
    """The model finds its own emissions.  The floor of 90 % keeps the test from passing on nothing; through the host twin
    and tests/host_pipeline.py all 200 of these sequences are reported (and included) hits of the default pipeline."""
    hmm = load_hmms("PF02826")[0]
    db = hmm.emit_block(200)
    (hits,) = list(hmmer.hmmsearch([hmm], db.block))
    reported = {h.name for h in hits if h.reported}
    assert len(reported) >= 180 and reported <= {f"2-Hacid_dh_C-sample{i}" for i in range(200)}
    direct = plan7.Pipeline(hmm.alphabet).search_hmm(hmm, db)    # the emitted database itself, resident on first use
    assert {h.name for h in direct if h.reported} == reported
    msa = hmmer.hmmalign(hmm, db.block[:8])
    assert len(msa.sequences) == 8


def test_slots_and_packed_block_go_back_to_the_pool(libp7x):
    """After a call the emitter holds its table and the per-sequence arrays (a few hundred KB here), not the slots (N x cap
    bytes, six times that with traces) nor the packed block: they are parked in the slab pool for whoever asks next."""
    def held():
        out = (C.c_int64 * 4)()
        assert libp7x.p7x_debug_memory_stats(0, out) == 0
        return out[0] - out[1]                                   # obtained from the runtime and not parked
    hmm, N = random_hmm(300, 8), 4000
    before = held()
    db = hmm.emit_block(N, traces=True)
    assert db.on_device and db.cap >= 300
    assert held() - before < N * db.cap


def test_errors_and_empty_block(libp7x):
    hmm = load_hmms("PF02826")[0]
    with pytest.raises(ValueError):
        hmm.emit_block(-1)
    empty = hmm.emit_block(0)
    assert len(empty) == 0 and empty.block.packed().dsq.tolist() == [255]
    hits = plan7.Pipeline(hmm.alphabet).search_hmm(hmm, empty)
    assert len(hits) == 0
