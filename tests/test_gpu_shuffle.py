"""Decoy sequences on the device (p7x_shuffle.hip): the kernels give the bytes of the host twin in every mode, for amino and
DNA, across run boundaries, on the long path, at every slab and run after run; and the decoys go through hmmsearch and
nhmmer as a block."""
import ctypes as C

import numpy as np
import pytest

import shuffle_cases as sc
from conftest import GOLDEN, load_hmms
from pyhmmer_amd import _lib, easel, hmmer
from test_gpu_search import _hit_fields

pytestmark = pytest.mark.gpu

AMINO, DNA = easel.Alphabet.amino(), easel.Alphabet.dna()
ALPHABETS = {"amino": AMINO, "dna": DNA}
MODES = [("mono", 0), ("di", 0), ("window", 7), ("window", 300), ("reverse", 0)]


@pytest.fixture(autouse=True)
def options(libp7x):
    _lib.set_debug_option("host_shuffle", -1)
    _lib.set_debug_option("shuffle_slab", -1)
    yield
    _lib.set_debug_option("host_shuffle", -1)
    _lib.set_debug_option("shuffle_slab", -1)


def twin(block, **kw):
    _lib.set_debug_option("host_shuffle", 1)
    try:
        out = block.shuffle(**kw)
    finally:
        _lib.set_debug_option("host_shuffle", -1)
    assert not out.on_device
    return out


def planned(block, mode):
    pk = block.packed()
    runs, longs, slab = C.c_int64(), C.c_int64(), C.c_int32()
    assert _lib.lib().p7x_shuffle_plan(pk.offsets.ctypes.data, pk.lengths.ctypes.data, pk.n, sc.MODES.index(mode), C.byref(runs), C.byref(longs),
                                       C.byref(slab)) == 0
    return runs.value, longs.value, slab.value


def assert_device_equals_twin(block, slabs=(-1,), seed=42, modes=MODES):
    """Every mode at every slab: the device block, twice, against the twin's; returns the device blocks of the last slab."""
    outs = {}
    for mode, window in modes:
        want = twin(block, seed=seed, mode=mode, window=window).packed().dsq
        for slab in slabs:
            _lib.set_debug_option("shuffle_slab", slab)
            first, second = block.shuffle(seed=seed, mode=mode, window=window), block.shuffle(seed=seed, mode=mode, window=window)
            assert first.on_device and second.on_device
            assert (first.runs, first.long_sequences) == planned(block, mode)[:2], (mode, slab)
            got = first.packed().dsq
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (mode, window, slab, bad[:8].tolist())
            assert np.array_equal(second.packed().dsq, got), (mode, window, slab, "second run")
            outs[(mode, window)] = first
        _lib.set_debug_option("shuffle_slab", -1)
    return outs


@pytest.mark.parametrize("abc", sorted(ALPHABETS))
def test_every_length_edge(abc):
    alphabet = ALPHABETS[abc]
    rng = np.random.default_rng(3)
    block = sc.make_block([sc.random_codes(rng, L, alphabet) for L in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)], alphabet)
    outs = assert_device_equals_twin(block)
    assert all(o.long_sequences == 0 and o.runs == 1 for o in outs.values())
    for (mode, window), o in outs.items():
        for s, g in zip(block, sc.decoys(o)):
            sc.check_invariants(s.sequence, g, mode, window, alphabet.Kp)


@pytest.mark.parametrize("abc", sorted(ALPHABETS))
def test_run_boundaries_and_the_long_path(abc):
    """Slab 512: spans of 449 .. 451 bytes one per run, 511 and more on the long path (mode di: all of them, its region is 256
    bytes); some short sequences around them so that runs of several sequences end at a long one."""
    alphabet = ALPHABETS[abc]
    rng = np.random.default_rng(4)
    lengths = [30, 447, 448, 449, 12, 0, 511, 512, 5, 513, 2000, 100, 200, 208, 1, 100, 200, 209]
    block = sc.make_block([sc.random_codes(rng, L, alphabet) for L in lengths], alphabet)
    _lib.set_debug_option("shuffle_slab", 512)
    assert planned(block, "mono") == (7, 4, 512) and planned(block, "di")[1] == 7
    outs = assert_device_equals_twin(block, slabs=(512,))
    assert outs[("mono", 0)].long_sequences == 4 and outs[("mono", 0)].runs == 7
    assert outs[("di", 0)].long_sequences == 7 and outs[("di", 0)].long_sequences > 0
    for (mode, window), o in outs.items():
        for s, g in zip(block, sc.decoys(o)):
            sc.check_invariants(s.sequence, g, mode, window, alphabet.Kp)


def test_more_sequences_than_lanes():
    rng = np.random.default_rng(5)
    block = sc.make_block([sc.random_codes(rng, 1, AMINO) for _ in range(300)], AMINO)
    outs = assert_device_equals_twin(block, slabs=(-1, 64))
    assert planned(block, "mono")[0] == 2
    assert np.array_equal(outs[("mono", 0)].packed().dsq, block.packed().dsq)


@pytest.mark.parametrize("abc", sorted(ALPHABETS))
def test_a_thousand_random_lengths_at_three_slabs(abc):
    alphabet = ALPHABETS[abc]
    rng = np.random.default_rng(6)
    block = sc.make_block([sc.random_codes(rng, L, alphabet) for L in rng.integers(1, 401, size=1000).tolist()], alphabet)
    assert_device_equals_twin(block, slabs=(512, 4096, -1))
    _lib.set_debug_option("shuffle_slab", 512)
    assert planned(block, "di")[1] > 0 and planned(block, "mono")[1] == 0


def test_proteome_and_bmyd(proteome):
    assert len(proteome) == 2100 and int((proteome.packed().lengths > 2000).sum()) == 5
    outs = assert_device_equals_twin(proteome, modes=[("mono", 0), ("di", 0), ("window", 20), ("reverse", 0)])
    assert outs[("mono", 0)].long_sequences == 0 and outs[("mono", 0)].runs == planned(proteome, "mono")[0] > 8
    with easel.SequenceFile(GOLDEN / "seqs" / "bmyD.fna", digital=True, alphabet=DNA) as sf:
        bmyd = sf.read_block()
    assert_device_equals_twin(bmyd, slabs=(-1, 512), modes=[("di", 0)])


def test_decoys_through_hmmsearch(proteome, models):
    """PF02826 against the mono decoys of the fixture proteome (seed 42), from the device block: the counters of the source
    search, the hits of the twin-made block, and no decoy below an E-value of 1e-3 (0.001 expected at Z = 2,100: a statement
    about the calibrated statistics).  Observed on an MI355X at seed 42: the hit list is empty -- 0 hits, 0 reported, so there
    is no smallest E-value to record; no decoy passed the filters."""
    hmm = models["PF02826"][0]
    source = next(hmmer.hmmsearch([hmm], proteome))
    dev = proteome.shuffle(seed=42, mode="mono")
    assert dev.on_device and dev._list is None
    got, want = next(hmmer.hmmsearch([hmm], dev)), next(hmmer.hmmsearch([hmm], twin(proteome, seed=42, mode="mono")))
    assert dev._list is None                                                    # searched as packed arrays
    assert (got.searched_sequences, got.searched_residues) == (source.searched_sequences, source.searched_residues) == (2100, proteome.total_length())
    assert _hit_fields(got) == _hit_fields(want)
    assert all(h.name.endswith("-shuffled") for h in got)
    evalues = [h.evalue for h in got]
    print(f"decoy search: {len(got)} hits, {sum(h.reported for h in got)} reported, smallest E-value {min(evalues) if evalues else None}")
    assert all(e >= 1e-3 for e in evalues), (len(got), min(evalues))


def test_decoys_through_nhmmer():
    """bmyD.hmm against the di decoys of bmyD.fna: the long-target pipeline takes the block and returns a list.  Observed on an
    MI355X at seed 42: 0 hits."""
    hmm = load_hmms("bmyD")[0]
    with easel.SequenceFile(GOLDEN / "seqs" / "bmyD.fna", digital=True, alphabet=DNA) as sf:
        bmyd = sf.read_block()
    decoys = bmyd.shuffle(seed=42, mode="di")
    assert decoys.on_device
    for s, g in zip(bmyd, sc.decoys(decoys)):
        sc.check_invariants(s.sequence, g, "di", 0, DNA.Kp)
    hits = next(hmmer.nhmmer(hmm, decoys))
    print(f"nhmmer on di decoys: {len(hits)} hits, E-values {[h.evalue for h in hits]}")
    assert isinstance(list(hits), list)
