"""MSA.identity_filter, compute_weights, mark_fragments, select, sequence_weights without a device (test seam
"host_pairid" = 1: the host twin of the kernel of p7x_msapair.hip compares the same integers; "host_build" = 1 for the
position-based weights): the reference's recorded cases (tests/test_easel/test_msa.py:91-171, 423-464), the float
threshold, LuxC at 0.62, and the twin against a plain numpy restatement of the definitions (msa_identity_cases.py)."""
import io

import numpy as np
import pytest

from conftest import GOLDEN
from pyhmmer_amd import _lib, easel, errors
import msa_identity_cases as ic

AMINO, DNA = easel.Alphabet.amino(), easel.Alphabet.dna()

FOUR_DNA = b"# STOCKHOLM 1.0\n\nseq1  ..AAAAAAAA\nseq2  AAAAAAAAAA\nseq3  CCCCCCCCCC\nseq4  GGGGGGGGGG\n//\n"
FRAGMENTS = b"# STOCKHOLM 1.0\n\nseq1  ..AAAAAA..\nseq2  .....AAAA.\nseq3  .CCC.CCCCC\nseq4  GGGGGGGGGG\n//\n"
IDENTICAL = b"# STOCKHOLM 1.0\n\nseq1 AAAAA\nseq2 AAAAA\nseq3 AAAAA\nseq4 AAAAA\nseq5 AAAAA\n//\n"
CONTRIVED = b"# STOCKHOLM 1.0\n\nseq1 AAAAA\nseq2 AAAAA\nseq3 CCCCC\nseq4 CCCCC\nseq5 TTTTT\n//\n"
NITROGENASE = b"# STOCKHOLM 1.0\n\nNIFE_CLOPA GYVGS\nNIFD_AZOVI GFDGF\nNIFD_BRAJA GYDGF\nNIFK_ANASP GYQGG\n//\n"


@pytest.fixture(autouse=True)
def host_twin(libp7x):
    _lib.set_debug_option("host_pairid", 1)
    _lib.set_debug_option("host_build", 1)
    yield
    for name in ("host_pairid", "host_build", "pairid_tile"):
        _lib.set_debug_option(name, -1)


def luxc(name="LuxC.sto"):
    with easel.MSAFile(GOLDEN / "msa" / name, digital=True, alphabet=AMINO) as f:
        return f.read()


def places3(got, want):
    """assertAlmostEqual(places=3) of the reference, element by element."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (len(want),)
    assert all(round(abs(g - w), 3) == 0 for g, w in zip(got, want)), (got, want)


# ----------------------------------------------------------------------------- 1. the reference's recorded cases
def check_recorded_cases():
    """Every recorded case (the host twin's here, the device's in test_gpu_msa_identity.py)."""
    msa = ic.parse(FOUR_DNA, DNA)
    out = msa.identity_filter(1.0)
    assert len(out.sequences) == 3 and out.names[0] == "seq2"
    out = msa.identity_filter(1.0, preference="origorder")
    assert len(out.sequences) == 3 and out.names[0] == "seq1"
    out = msa.identity_filter(1.0, preference="random", seed=11)
    assert len(out.sequences) == 3 and out.names[0] in ("seq1", "seq2")
    assert msa.identity_filter(1.0, preference="random", seed=11).names == out.names

    filtered, expected = luxc().identity_filter(), luxc("LuxC.weighted.sto")
    assert len(filtered.sequences) == len(expected.sequences) == 13
    assert filtered.names == expected.names
    assert np.array_equal(filtered._codes(), expected._codes())

    places3(ic.parse(IDENTICAL, DNA).compute_weights("blosum"), [1.0] * 5)
    places3(ic.parse(IDENTICAL, AMINO).compute_weights("blosum"), [1.0] * 5)
    places3(ic.parse(IDENTICAL, AMINO).compute_weights("pb"), [1.0] * 5)
    for method in ("pb", "blosum"):
        places3(ic.parse(CONTRIVED, AMINO).compute_weights(method), [0.833333, 0.833333, 0.833333, 0.833333, 1.66667])
    nif = ic.parse(NITROGENASE, AMINO)
    places3(nif.compute_weights("pb"), [1.066667, 1.066667, 0.800000, 1.066667])
    got = nif.compute_weights("blosum")
    places3(got, [1.333333, 0.666667, 0.666667, 1.333333])
    assert got is nif.sequence_weights              # stored, and returned


def test_recorded_cases():
    check_recorded_cases()


def test_mark_fragments():
    msa = ic.parse(FRAGMENTS, DNA)
    assert msa.mark_fragments(0.5).tolist() == [False, True, False, False]
    assert msa.mark_fragments(0.95).tolist() == [True, True, True, False]
    assert msa.textize().mark_fragments(0.5).tolist() == [False, True, False, False]
    with pytest.raises(ValueError):
        easel.TextMSA().mark_fragments(200.0)
    with pytest.raises(errors.InvalidParameter):
        msa.mark_fragments(-0.1)


# ----------------------------------------------------------------------------- 2. the threshold is a C float
def test_float_threshold():
    """Rows 2 and 3 of nitrogenase are identical in exactly 4 of 5: (double)(float) 0.8 is above 4 / 5 in double."""
    nif = ic.parse(NITROGENASE, AMINO)
    idents, length = ic.lib_counts(nif._codes(), AMINO.type_code)
    assert idents[1, 2] == 4 and length.tolist() == [5, 5, 5, 5]
    assert float(np.float32(0.8)) > 4 / 5
    assert len(nif.identity_filter(0.8, preference="origorder").sequences) == 4
    assert nif.identity_filter(0.79, preference="origorder").names == ("NIFE_CLOPA", "NIFD_AZOVI", "NIFK_ANASP")


# ----------------------------------------------------------------------------- 3. LuxC at 0.62
def test_luxc_at_062():
    """9 rows, 8 clusters, largest identity 0.792: figures of the numpy restatement (msa_identity_cases.py) run on a CPU,
    not of upstream; the restatement is evaluated again here and the library must agree with it."""
    msa = luxc()
    ax = msa._codes()
    linked = ic.linked_matrix(ax, 20, 0.62)
    assert int(ic.greedy_keep(linked, range(13)).sum()) == 9
    assert len(set(ic.cluster_labels(linked).tolist())) == 8
    assert round(ic.max_identity_of(ax, 20), 3) == 0.792
    assert len(msa.identity_filter(0.62, preference="origorder").sequences) == 9
    cluster, ncl, _ = ic.lib_linkage(ax, AMINO.type_code, 0.62)
    assert ncl == 8 and np.array_equal(cluster, ic.cluster_labels(linked))
    assert np.allclose(msa.compute_weights("blosum"), ic.blosum_weights(linked), rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------- 4. the twin against the restatement
@pytest.mark.parametrize("n", [1, 2, 3, 65, 130])
def test_twin_equals_the_restatement(n):
    for alen in (1, 3, 5, 64, 257):
        amino = (n + alen) % 2 == 0
        abc = AMINO if amino else DNA
        ax = ic.generated(n, alen, amino)
        msa = ic.as_msa(ax, amino)
        assert np.array_equal(msa._codes(), ax)
        want_idents, want_len = ic.pair_counts(ax, abc.K)
        orders = {"origorder": np.arange(n), "conscover": ic.conscover_order(ax, abc.K, abc.Kp), "random": msa._filter_order("random", seed=5)}
        assert np.array_equal(msa._filter_order("conscover"), orders["conscover"])
        assert sorted(orders["random"].tolist()) == list(range(n))
        for tile in (-1, 1, 3, 64) if alen in (5, 257) else (-1, 7):
            _lib.set_debug_option("pairid_tile", tile)
            idents, length = ic.lib_counts(ax, abc.type_code)
            assert np.array_equal(idents, want_idents) and np.array_equal(length, want_len), (n, alen, tile)
            for t in ic.THRESHOLDS:
                linked = ic.linked_matrix(ax, abc.K, t)
                for pref, order in orders.items():
                    keep, _ = ic.lib_filter(ax, abc.type_code, order, t)
                    assert np.array_equal(keep, ic.greedy_keep(linked, order)), (n, alen, tile, t, pref)
                cluster, ncl, _ = ic.lib_linkage(ax, abc.type_code, t)
                assert np.array_equal(cluster, ic.cluster_labels(linked)) and ncl == len(set(cluster.tolist())), (n, alen, tile, t)
                rows_a, rows_b = np.arange(n)[::-1], np.arange(0, n, 2)
                bits, flags = ic.lib_links(ax, abc.type_code, t, rows_a, rows_b)
                sub = linked[np.ix_(rows_a, rows_b)]
                assert np.array_equal(bits, ic.pack_bits(sub)) and np.array_equal(flags, sub.any(axis=1)), (n, alen, tile, t)
        _lib.set_debug_option("pairid_tile", -1)
        # through the Python layer: the rows kept, in the alignment's order
        linked = ic.linked_matrix(ax, abc.K, 0.62)
        for pref, order in orders.items():
            out = msa.identity_filter(0.62, preference=pref, seed=5)
            assert out.names == tuple(f"row{i}" for i in np.flatnonzero(ic.greedy_keep(linked, order))), (n, alen, pref)


def test_limits_and_bad_input():
    ax = ic.generated(3, 5)
    with pytest.raises(OverflowError):
        ic.lib_counts(np.zeros((4097, 1), dtype=np.uint8), AMINO.type_code)
    with pytest.raises(OverflowError):
        ic.lib_linkage(np.zeros(((1 << 18) + 1, 1), dtype=np.uint8), AMINO.type_code, 0.62)
    with pytest.raises(OverflowError):
        ic.lib_filter(np.zeros((1, 65536), dtype=np.uint8), AMINO.type_code, [0], 0.62)
    with pytest.raises(ValueError):
        ic.lib_filter(ax, AMINO.type_code, [0, 0, 1], 0.62)               # no permutation
    with pytest.raises(ValueError):
        ic.lib_counts(np.full((2, 2), 29, dtype=np.uint8), AMINO.type_code)     # no code of the alphabet


# ----------------------------------------------------------------------------- 5. select, sequence_weights, WT lines
def test_select():
    with easel.MSAFile(GOLDEN / "msa" / "LuxC.hmmalign.sto") as f:
        msa = f.read()
    assert msa.posterior_probabilities is not None and msa.reference is not None
    sub = msa.select(sequences=[2, 0, 2], columns=range(1, 4))
    assert type(sub) is type(msa) and sub.names == (msa.names[0], msa.names[2])
    assert sub.alignment == (msa.alignment[0][1:4], msa.alignment[2][1:4])
    assert sub.posterior_probabilities == [msa.posterior_probabilities[0][1:4], msa.posterior_probabilities[2][1:4]]
    assert sub.reference == msa.reference[1:4] and sub.pp_consensus == msa.pp_consensus[1:4]
    assert sub._accs == [msa._accs[0], msa._accs[2]] and sub.name == msa.name
    assert msa.select() == msa and msa.select() is not msa
    t = easel.TextMSA(name="msa", sequences=[easel.TextSequence(name=f"seq{i + 1}", sequence=s) for i, s in enumerate(("ATGC", "ATCC", "ATGA"))])
    assert t.select(sequences=[0, 2]).names == ("seq1", "seq3")
    assert t.select(columns=range(1, 4)).alignment == ("TGC", "TCC", "TGA")
    for kw in ({"sequences": [3]}, {"columns": [4]}, {"sequences": [-1]}):
        with pytest.raises(IndexError):
            t.select(**kw)
    d = luxc("LuxC.weighted.sto")
    assert np.array_equal(d.select(sequences=[1, 5]).sequence_weights, d.sequence_weights[[1, 5]])
    assert d.select(sequences=[1, 5]).alphabet == AMINO


def test_sequence_weights():
    msa = ic.parse(NITROGENASE, AMINO)
    assert msa.sequence_weights.tolist() == [1.0] * 4
    msa.sequence_weights = [0.5, 1.5, 1.0, 1.0004]
    assert msa.sequence_weights.tolist() == [0.5, 1.5, 1.0, 1.0004]
    with pytest.raises(ValueError, match="dimension mismatch"):
        msa.sequence_weights = [1.0, 1.0]
    with pytest.raises(ValueError, match="must sum to 4"):
        msa.sequence_weights = [1.0, 1.0, 1.0, 1.01]
    assert msa.sequence_weights.tolist() == [0.5, 1.5, 1.0, 1.0004]
    del msa.sequence_weights
    assert msa.sequence_weights.tolist() == [1.0] * 4


def test_msafile_reads_weights():
    msa = luxc("LuxC.weighted.sto")
    wt = [float(l.split()[3]) for l in (GOLDEN / "msa" / "LuxC.weighted.sto").read_text().splitlines() if l.startswith("#=GS") and l.split()[2] == "WT"]
    assert len(wt) == 13 and msa.sequence_weights.tolist() == wt
    assert luxc().sequence_weights.tolist() == [1.0] * 13               # no WT lines: the default
    with easel.MSAFile(GOLDEN / "msa" / "LuxC.weighted.sto") as f:
        assert f.read().sequence_weights.tolist() == wt                 # text mode too


# ----------------------------------------------------------------------------- 6. the InvalidParameter of the two methods
BAD_ARGUMENTS = [("fragment_threshold", -0.1), ("fragment_threshold", 1.5), ("consensus_fraction", -0.1), ("consensus_fraction", 1.5),
                 ("sample_threshold", -1), ("sample_count", -1), ("max_fragments", -1), ("preference", "best")]


@pytest.mark.parametrize("name,value", BAD_ARGUMENTS)
def test_invalid_parameters(name, value):
    msa = ic.parse(NITROGENASE, AMINO)
    for call in (msa.identity_filter, lambda **kw: msa.compute_weights("pb", **kw)):
        with pytest.raises(errors.InvalidParameter) as e:
            call(**{name: value})
        assert e.value.name == name and e.value.value == value
        assert (e.value.choices == ["conscover", "origorder", "random"]) if name == "preference" else (e.value.hint is not None)


def test_methods():
    msa = ic.parse(NITROGENASE, AMINO)
    with pytest.raises(errors.InvalidParameter) as e:
        msa.compute_weights("upgma")
    assert e.value.name == "method" and e.value.choices == ["pb", "gsc", "blosum"]
    with pytest.raises(NotImplementedError):
        msa.compute_weights("gsc")
    with pytest.raises(NotImplementedError, match="amino"):
        ic.parse(IDENTICAL, DNA).compute_weights("pb")
    places3(msa.compute_weights("PB"), [1.066667, 1.066667, 0.8, 1.066667])      # the method's case is ignored


def test_reference_columns_rule_the_order():
    """With a #=GC RF line the consensus columns are its columns, unless ignore_rf: here they cover seq1's span only."""
    text = FOUR_DNA.replace(b"//\n", b"#=GC RF ..xxxxxxxx\n//\n")
    msa = ic.parse(text, DNA)
    assert msa.identity_filter(1.0).names[0] == "seq1"                      # a tie: the original order
    assert msa.identity_filter(1.0, ignore_rf=True).names[0] == "seq2"


# ----------------------------------------------------------------------------- 7. no device, no seam
def test_no_device_is_an_error(libp7x):
    if libp7x.p7x_device_count() != 0:
        return                                                             # only where there is no device
    _lib.set_debug_option("host_pairid", -1)
    msa = ic.parse(NITROGENASE, AMINO)
    with pytest.raises(errors.DeviceUnavailable):
        msa.identity_filter()
    with pytest.raises(errors.DeviceUnavailable):
        msa.compute_weights("blosum")
    with pytest.raises(errors.DeviceUnavailable):
        ic.lib_counts(msa._codes(), AMINO.type_code)
