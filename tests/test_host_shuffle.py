"""Decoy sequences on the host (p7x_shuffle.cpp: the twin of the shuffle kernels, through DigitalSequence.shuffle and the seam
"host_shuffle"): the bytes of a plain-Python restatement for reverse / mono / window, the invariants of every mode, the
independence of a sequence from the rest of its block, the uniformity of mono and di by counting, the argument checks and
the layout of a ShuffledBlock."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import shuffle_cases as sc
from pyhmmer_amd import _lib, easel, errors

AMINO, DNA = easel.Alphabet.amino(), easel.Alphabet.dna()
ALPHABETS = {"amino": AMINO, "dna": DNA}
LENGTHS = [0, 1, 2, 3, 64, 65, 257]
SEEDS = [1, 2 ** 32 - 1]


@pytest.fixture(autouse=True)
def host_twin(libp7x):
    _lib.set_debug_option("host_shuffle", 1)
    _lib.set_debug_option("shuffle_slab", -1)
    yield
    _lib.set_debug_option("host_shuffle", -1)
    _lib.set_debug_option("shuffle_slab", -1)


def windows_of(L):
    return sorted({w for w in (1, 2, 7, L - 1, L, L + 1) if w >= 1})


@pytest.mark.parametrize("abc", sorted(ALPHABETS))
def test_twin_equals_the_restatement(abc):
    """reverse / mono / window byte for byte, one sequence through DigitalSequence.shuffle and the same sequences as a block
    through the seam (sequence i of a block draws from the stream of index i)."""
    alphabet = ALPHABETS[abc]
    rng = np.random.default_rng(11)
    seqs = [sc.random_codes(rng, L, alphabet) for L in LENGTHS]
    assert any(int(s.max()) >= alphabet.K for s in seqs if len(s) > 60)          # degenerate codes are among them
    block = sc.make_block(seqs, alphabet)
    for seed in SEEDS:
        for mode in ("reverse", "mono"):
            got = sc.decoys(block.shuffle(seed=seed, mode=mode))
            for i, (s, g) in enumerate(zip(seqs, got)):
                assert g.tolist() == sc.restated(s, mode, seed, seq=i), (mode, seed, len(s))
                assert block[i].shuffle(seed=seed, mode=mode).sequence.tolist() == sc.restated(s, mode, seed, seq=0)
        for i, s in enumerate(seqs):
            L = len(s)
            one = easel.DigitalSequence(alphabet, name="q", sequence=s)
            mono = one.shuffle(seed=seed, mode="mono").sequence.tolist()
            for w in windows_of(L):
                got = one.shuffle(seed=seed, mode="window", window=w).sequence.tolist()
                assert got == sc.restated(s, "window", seed, window=w), (seed, L, w)
                if w >= L:
                    assert got == mono, (seed, L, w)
        # windows in a block: every sequence with its own stream
        for w in (1, 2, 7, 64, 65):
            got = sc.decoys(block.shuffle(seed=seed, mode="window", window=w))
            for i, (s, g) in enumerate(zip(seqs, got)):
                assert g.tolist() == sc.restated(s, "window", seed, seq=i, window=w), (seed, len(s), w)


def test_the_restated_philox_is_the_librarys(libp7x):
    """The restatement's generator against the library's one block (p7x_debug_philox): the two were written apart."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        key = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64).astype(np.uint32)
        ctr = rng.integers(0, 2 ** 32, size=4, dtype=np.uint64).astype(np.uint32)
        out = np.zeros(4, dtype=np.uint32)
        assert libp7x.p7x_debug_philox(key.ctypes.data, ctr.ctypes.data, out.ctypes.data) == 0
        assert tuple(out.tolist()) == sc.philox4x32_10(tuple(key.tolist()), tuple(ctr.tolist()))


@pytest.mark.parametrize("abc", sorted(ALPHABETS))
def test_invariants_of_every_mode(abc):
    alphabet = ALPHABETS[abc]
    rng = np.random.default_rng(23)
    lengths = [0, 1, 2, 3] + rng.integers(0, 401, size=196).tolist()
    seqs = [sc.random_codes(rng, L, alphabet) for L in lengths]
    block = sc.make_block(seqs, alphabet)
    for mode, window in (("mono", 0), ("di", 0), ("window", 7), ("window", 50), ("reverse", 0)):
        out = block.shuffle(seed=9, mode=mode, window=window)
        assert not out.on_device and out.mode == mode and out.window == window and out.seed == 9
        got = sc.decoys(out)
        assert len(got) == len(seqs) == 200
        for s, g in zip(seqs, got):
            sc.check_invariants(s, g, mode, window, alphabet.Kp)
        if mode in ("mono", "di"):
            changed = sum(not np.array_equal(s, g) for s, g in zip(seqs, got) if len(s) >= 20)
            assert changed >= 0.95 * sum(len(s) >= 20 for s in seqs), mode           # a shuffle, not a copy


def test_determinism_and_independence():
    rng = np.random.default_rng(31)
    seqs = [sc.random_codes(rng, L, AMINO) for L in rng.integers(20, 300, size=40).tolist()]
    block = sc.make_block(seqs, AMINO)
    for mode, window in (("mono", 0), ("di", 0), ("window", 13)):
        a, b = sc.decoys(block.shuffle(seed=3, mode=mode, window=window)), sc.decoys(block.shuffle(seed=3, mode=mode, window=window))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        other = sc.decoys(block.shuffle(seed=4, mode=mode, window=window))
        assert all(not np.array_equal(x, y) for x, y in zip(a, other)), mode           # L >= 20: a different seed, different bytes
        zero = sc.decoys(block.shuffle(seed=0, mode=mode, window=window))              # seed 0 is a seed like any other
        assert all(np.array_equal(x, y) for x, y in zip(zero, sc.decoys(block.shuffle(seed=0, mode=mode, window=window))))
        assert all(not np.array_equal(x, y) for x, y in zip(zero, a))
        for k in (1, 7, 39):
            head = sc.decoys(block[:k].shuffle(seed=3, mode=mode, window=window))
            assert len(head) == k and all(np.array_equal(x, y) for x, y in zip(head, a))
        first = sc.make_block(seqs[:1], AMINO).shuffle(seed=3, mode=mode, window=window)
        alone = block[0].shuffle(seed=3, mode=mode, window=window)
        assert np.array_equal(first[0].sequence, alone.sequence) and np.array_equal(alone.sequence, a[0])
        assert (first[0].name, first[0].description, first[0].accession) == (alone.name, alone.description, alone.accession)
    # the threads of the twin do not matter
    pk = block.packed()
    outs = []
    for threads in (1, 3, 16):
        dsq = np.empty_like(pk.dsq)
        st = _lib.lib().p7x_shuffle_host(AMINO.type_code, pk.dsq.ctypes.data, pk.offsets.ctypes.data, pk.lengths.ctypes.data, pk.n, pk.dsq.shape[0],
                                         1, 0, 3, threads, dsq.ctypes.data, None)
        assert st == 0
        outs.append(dsq)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[0], block.shuffle(seed=3, mode="di").packed().dsq)


def test_mono_is_uniform():
    """72,000 copies of one sequence of six distinct residues: each of the 720 permutations within six standard deviations
    of n / 720, sigma^2 = n (1/720) (719/720) -- about 1.4e-6 false alarms expected over the 720 cells."""
    n = 72000
    src = np.array([0, 3, 5, 8, 12, 19], dtype=np.uint8)
    pk = easel.PackedBlock.from_arrays(np.concatenate([[255], np.tile(np.append(src, 255), n)]).astype(np.uint8),
                                       1 + 7 * np.arange(n, dtype=np.int64), np.full(n, 6, dtype=np.int32))
    dsq, stats = easel._shuffle_packed(AMINO, pk, 0, 0, 42, host=True, threads=4)
    rows = dsq[1:].reshape(n, 7)
    assert np.all(rows[:, 6] == 255) and np.all(np.sort(rows[:, :6], axis=1) == np.sort(src))
    keys = (rows[:, :6].astype(np.int64) * (32 ** np.arange(6))).sum(axis=1)
    values, counts = np.unique(keys, return_counts=True)
    assert len(values) == 720
    mean, sigma = n / 720, (n * (1 / 720) * (719 / 720)) ** 0.5
    assert np.all(np.abs(counts - mean) <= 6 * sigma), (counts.min(), counts.max(), mean, sigma)


DI_CASES = [("dna", "GCTTAGTTGG"), ("amino", "LQQVQCVLVV")]      # T -> T and Q -> Q can be drawn as last edges: rejected attempts


@pytest.mark.parametrize("abc,text", DI_CASES)
def test_di_is_uniform(abc, text):
    alphabet = ALPHABETS[abc]
    src = alphabet.encode(text)
    arrangements = sc.di_arrangements(src)
    assert 9 <= len(src) <= 10 and 20 <= len(arrangements) <= 200
    assert tuple(src.tolist()) in arrangements
    n = 1000 * len(arrangements)
    got = Counter(tuple(d.tolist()) for d in sc.decoys(sc.make_block([src] * n, alphabet).shuffle(seed=42, mode="di")))
    assert set(got) <= set(arrangements)
    p = 1 / len(arrangements)
    mean, sigma = n * p, (n * p * (1 - p)) ** 0.5
    for a in arrangements:
        assert abs(got[a] - mean) <= 6 * sigma, (a, got[a], mean, sigma)


def test_di_enumerator_and_forced_rejections():
    """The enumerator against a filter over every permutation; and ACACACGG, whose only arrangement is itself while two of the
    three last edges C can draw (C -> A) close a cycle with A -> C: two attempts in three are rejected, and the answer stands."""
    for text in ("ACACACGG", "ACGTACGA", "AACCAACA", "GATTACAGA"):
        src = DNA.encode(text)
        assert sc.di_arrangements(src) == sc.di_arrangements_by_permutation(src), text
    src = DNA.encode("ACACACGG")
    assert sc.di_arrangements(src) == [tuple(src.tolist())]
    out = sc.decoys(sc.make_block([src] * 500, DNA).shuffle(seed=1, mode="di"))
    assert all(np.array_equal(d, src) for d in out)
    # a case with rejections and more than one answer: every decoy is an arrangement, and all of them turn up
    src = DNA.encode("ACACACGGTCAG")
    arrangements = set(sc.di_arrangements(src))
    got = {tuple(d.tolist()) for d in sc.decoys(sc.make_block([src] * 4000, DNA).shuffle(seed=1, mode="di"))}
    assert got <= arrangements and (len(arrangements) > 60 or got == arrangements)


def test_arguments_and_layout(libp7x):
    rng = np.random.default_rng(41)
    seqs = [sc.random_codes(rng, L, DNA) for L in (5, 0, 31, 1, 200)]
    block = sc.make_block(seqs, DNA)
    one = block[0]
    for call in (block.shuffle, one.shuffle):
        with pytest.raises(errors.InvalidParameter) as err:
            call(mode="k-mer")
        assert err.value.name == "mode" and err.value.choices == ["mono", "di", "window", "reverse"]
        with pytest.raises(errors.InvalidParameter) as err:
            call(mode="mono", window=-1)
        assert err.value.name == "window" and err.value.hint
        with pytest.raises(errors.InvalidParameter) as err:
            call(mode="window", window=0)
        assert err.value.name == "window" and err.value.hint
        for seed in (-1, 2 ** 32):
            with pytest.raises(errors.InvalidParameter) as err:
                call(seed=seed)
            assert err.value.name == "seed" and err.value.hint
        call(seed=0), call(seed=2 ** 32 - 1)
    out = block.shuffle(seed=7, mode="mono")
    assert isinstance(out, easel.ShuffledBlock) and isinstance(out, easel.DigitalSequenceBlock) and out.alphabet == DNA
    assert out.source_block is block and (out.mode, out.seed, out.window) == ("mono", 7, 0)
    assert not out.on_device and out.long_sequences == 0 and out.runs == 1 and out.kernel_us >= 0
    src_pk, pk = block.packed(), out.packed()
    assert np.array_equal(pk.offsets, src_pk.offsets) and np.array_equal(pk.lengths, src_pk.lengths)
    assert pk.dsq.shape == src_pk.dsq.shape and np.array_equal(pk.dsq == 255, src_pk.dsq == 255)
    assert len(out) == 5 and out.total_length() == block.total_length()
    for i in (0, 4, -1):
        d, s = out[i], block[i]
        assert (d.name, d.description, d.accession) == (f"{s.name}-shuffled", s.description, s.accession)
        assert len(d) == len(s) and d.alphabet == DNA
    assert out._list is None                                    # indexing made no list
    strtab, name_off, desc_off = out._strtab, out._name_off, out._desc_off
    cstr = lambda o: bytes(strtab[o:]).split(b"\0", 1)[0].decode()
    assert [cstr(int(o)) for o in name_off] == [f"s{i}-shuffled" for i in range(5)]
    assert [cstr(int(o)) for o in desc_off] == [f"sequence {i}" for i in range(5)]
    assert [s.name for s in out] == [f"s{i}-shuffled" for i in range(5)]
    # the decoys of a block that is itself kept packed (the FASTA reader's): names from its tables
    lazy = easel._LazyDigitalSequenceBlock(DNA, src_pk, *block.shuffle(mode="reverse")._string_tables())
    again = lazy.shuffle(seed=7, mode="mono")
    assert again[2].name == "s2-shuffled-shuffled" and lazy._list is None
    assert bytes(again._strtab[int(again._name_off[4]):]).split(b"\0", 1)[0] == b"s4-shuffled-shuffled"
    assert np.array_equal(again.packed().dsq, pk.dsq)
    # an empty block, and a block of empty sequences
    assert len(easel.DigitalSequenceBlock(DNA).shuffle()) == 0
    assert easel.DigitalSequenceBlock(DNA).shuffle().packed().dsq.tolist() == [255]
    assert sc.make_block([[], []], DNA).shuffle(mode="di").packed().dsq.tolist() == [255, 255, 255]
    # without a device and without the seam the block call has nothing to fall back to
    if libp7x.p7x_device_count() == 0:
        _lib.set_debug_option("host_shuffle", -1)
        with pytest.raises(errors.DeviceUnavailable):
            block.shuffle()
        assert len(one.shuffle()) == len(one)                   # one sequence needs no device


def test_plan_and_abi(libp7x):
    """The new symbols are bound; the plan: runs of at most 256 sequences whose span (sentinels included) fits the slab, half
    of it in mode di; a sequence that alone does not fit is long; the slab is clamped to a multiple of 64 from 64 up."""
    for name in ("p7x_shuffle_block", "p7x_shuffle_host", "p7x_shuffle_plan"):
        assert name in _lib.declared_symbols() and hasattr(libp7x, name)

    def plan(lengths, mode):
        lengths = np.asarray(lengths, dtype=np.int32)
        runs, longs, slab = C.c_int64(), C.c_int64(), C.c_int32()
        assert libp7x.p7x_shuffle_plan(None, lengths.ctypes.data, len(lengths), mode, C.byref(runs), C.byref(longs), C.byref(slab)) == 0
        return runs.value, longs.value, slab.value

    assert plan([], 0) == (0, 0, 65536)
    assert plan([1] * 300, 0) == (2, 0, 65536)                  # more sequences than lanes
    _lib.set_debug_option("shuffle_slab", 512)
    assert plan([510], 0) == (1, 0, 512) and plan([511], 0) == (0, 1, 512)
    assert plan([254], 1) == (1, 0, 512) and plan([255], 1) == (0, 1, 512)
    assert plan([254, 255], 0) == (1, 0, 512) and plan([255, 255], 0) == (2, 0, 512)      # 1 + 255 + 256 = 512 fits, 513 does not
    assert plan([447, 448, 449, 511, 512, 513, 2000], 0) == (3, 4, 512)
    assert plan([100, 2000, 100], 3) == (2, 1, 512)             # a long sequence closes the run before it
    _lib.set_debug_option("shuffle_slab", 1)
    assert plan([62], 0) == (1, 0, 64) and plan([63], 0) == (0, 1, 64)
    _lib.set_debug_option("shuffle_slab", 200)
    assert plan([], 0)[2] == 192
    # what is not a packed block is refused
    dsq = np.array([255, 1, 2, 255], dtype=np.uint8)
    out = np.empty_like(dsq)
    off, bad_len = np.array([1], dtype=np.int64), np.array([3], dtype=np.int32)
    assert libp7x.p7x_shuffle_host(DNA.type_code, dsq.ctypes.data, off.ctypes.data, bad_len.ctypes.data, 1, 4, 0, 0, 1, 1, out.ctypes.data, None) == 11
    good_len = np.array([2], dtype=np.int32)
    assert libp7x.p7x_shuffle_host(DNA.type_code, dsq.ctypes.data, off.ctypes.data, good_len.ctypes.data, 1, 4, 7, 0, 1, 1, out.ctypes.data, None) == 11
    dsq[1] = 18                                                  # outside the DNA alphabet: refused by di, a symbol for mono
    assert libp7x.p7x_shuffle_host(DNA.type_code, dsq.ctypes.data, off.ctypes.data, good_len.ctypes.data, 1, 4, 1, 0, 1, 1, out.ctypes.data, None) == 11
    assert libp7x.p7x_shuffle_host(DNA.type_code, dsq.ctypes.data, off.ctypes.data, good_len.ctypes.data, 1, 4, 0, 0, 1, 1, out.ctypes.data, None) == 0
