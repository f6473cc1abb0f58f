"""Builder.build_msa on the device (p7x_msabuild.hip) against its host twin (test seam "host_build" = 1).  Every sum over the
rows of the alignment is a sum of integers -- counts, or weights in fixed point -- so the kernels must give the twin's bytes
whatever the grid and the row chunk ("build_rows"); then the LuxC model, its calibration against the fixture's STATS lines,
a library build in one calibration batch, and a search with the built model against the search with the fixture."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GOLDEN
from pyhmmer_amd import _lib, easel, errors, hmmer, plan7
import msa_cases as mc
from test_host_build_msa import check_luxc_model, luxc_msa, sampled_msa

pytestmark = pytest.mark.gpu

ARRAYS = ("column_counts", "weights", "weighted_counts", "map", "node_counts", "transition_counts", "weight_columns", "fragments")


def counts_of(builder, msa, host, rows=-1):
    _lib.set_debug_option("host_build", 1 if host else -1)
    _lib.set_debug_option("build_rows", rows)
    try:
        c = builder._msa_counts(msa)
    finally:
        _lib.set_debug_option("host_build", -1)
        _lib.set_debug_option("build_rows", -1)
    assert bool(c.on_device) == (not host)
    return {name: getattr(c, name) for name in ARRAYS}


def assert_same_bytes(dev, twin, what):
    for name in ARRAYS:
        assert dev[name].dtype == twin[name].dtype and dev[name].shape == twin[name].shape, (what, name)
        assert dev[name].tobytes() == twin[name].tobytes(), (what, name)


@pytest.fixture(scope="module")
def builder():
    return plan7.Builder(mc.AMINO)


def test_luxc_counts_are_the_twins(builder):
    msa = luxc_msa()
    twin = counts_of(builder, msa, host=True)
    assert twin["map"].shape == (400,)
    for rows in (-1, 1, 7, 64):
        assert_same_bytes(counts_of(builder, msa, host=False, rows=rows), twin, ("LuxC", rows))


@pytest.mark.parametrize("alen", [3, 4, 5, 255, 256, 257, 700])
def test_constructed_shapes(builder, alen):
    """1 to 65 rows by 3 to 700 columns: a partial dword, exactly one, one over; a partial tile of columns, exactly one (256
    for the counts, 128 and 256 for the weighted counts), one over, several; every row chunk crossed."""
    for n in (1, 2, 63, 64, 65):
        for ends in (True, False):
            msa = mc.msa_of(mc.random_rows(n, alen, seed=1000 * alen + n, ends_consensus=ends), name=f"c{n}x{alen}")
            twin = counts_of(builder, msa, host=True)
            cons = set(twin["map"].tolist())
            if n >= 63 and alen >= 255:             # (in a few columns most rows may hold no residue at all, and weigh nothing)
                assert ((0 in cons) and (alen - 1 in cons)) == ends, (n, alen, ends)
            for rows in (1, 7, 64):
                assert_same_bytes(counts_of(builder, msa, host=False, rows=rows), twin, (n, alen, ends, rows))


def test_deep_alignment_with_fragments(builder, models):
    msa = sampled_msa(models["PF02826"][0], 3000, 7)
    rows = list(msa._rows)
    alen = len(msa)
    for i in range(30):                                 # 30 rows cut to a third of the columns, somewhere
        r = 100 * i + 3
        lo = (37 * i) % (alen // 2)
        rows[r] = "-" * lo + rows[r][lo:lo + alen // 3] + "-" * (alen - lo - alen // 3)
    cut = mc.msa_of(rows, name="deep", names=list(msa.names))
    twin = counts_of(builder, cut, host=True)
    assert int(twin["fragments"].sum()) == 30 and twin["fragments"][3::100][:30].all()
    dev = counts_of(builder, cut, host=False)
    assert_same_bytes(dev, twin, "deep")
    assert_same_bytes(counts_of(builder, cut, host=False), dev, "deep, second run")
    assert_same_bytes(counts_of(builder, cut, host=False, rows=7), twin, "deep, rows of 7")


def test_insert_counts_beyond_64_bits():
    """The alignment of test_host_build_msa.py whose I->I count passes 2^64: the kernel's two sums are the twin's."""
    n, alen = 4096, 4200
    b = plan7.Builder(mc.AMINO, architecture="hand", weighting="none")
    msa = mc.msa_of(["A" + "C" * (alen - 2) + "D"] * n, rf="x" + "." * (alen - 2) + "x", names=[f"r{i}" for i in range(n)])
    twin = counts_of(b, msa, host=True)
    assert int(twin["transition_counts"][1, 4]) + (int(twin["transition_counts"][1, 7]) << 20) == n * (alen - 3) << 40
    assert_same_bytes(counts_of(b, msa, host=False), twin, "beyond 64 bits")


def test_build_msa_luxc(builder, models):
    """The host assertions on the device's model, and the calibration against the fixture's STATS lines: lambda = ln 2 +
    1.44 / (M relent); the locations within four standard errors of a location fitted from 200 samples, 4 / (lambda
    sqrt 200) = 0.40 bits (the stream is upstream's for seed 42: the measured distances are in DESIGN.md 3.15)."""
    bg = plan7.Background(mc.AMINO)
    hmm, profile, om = builder.build_msa(luxc_msa(), bg)
    check_luxc_model(hmm, bg, models["LuxC"][0])
    ev = hmm.evalue_parameters.as_vector()
    want = models["LuxC"][0].evalue_parameters.as_vector()
    lam = math.log(2.0) + 1.44 / (hmm.M * hmm.mean_match_relative_entropy(bg))
    print("lambda", ev[1], lam, "mu/tau distances", [float(ev[i] - want[i]) for i in (0, 2, 4)])
    for i in (1, 3, 5):
        assert abs(ev[i] - lam) <= 1e-5 and abs(ev[i] - 0.69925) <= 1e-5
    bound = 4.0 / (lam * math.sqrt(200.0))
    assert abs(bound - 0.40) < 0.005
    for i, fixture in ((0, -11.3057), (2, -12.2470), (4, -5.7663)):
        assert abs(want[i] - fixture) < 1e-4
        assert abs(ev[i] - fixture) <= bound, (i, ev[i], fixture)
    assert np.array_equal(om.evalue_parameters.as_vector(), ev) and profile.M == hmm.M


def test_build_msa_block_equals_single_builds(builder, models):
    bg = plan7.Background(mc.AMINO)
    short = {h.name: h for h in models["RREFam"]}
    msas = [luxc_msa(), sampled_msa(models["PF02826"][0], 60, 3), sampled_msa(models["KR"][0], 40, 4),
            sampled_msa(short["Thiaglutamate_B_RRE"], 40, 7), sampled_msa(short["Trifolitoxin_RRE"], 40, 10)]
    block = builder.build_msa_block(msas, bg)
    assert len(block) == 5
    for msa, (hmm, profile, om) in zip(msas, block):
        one, p1, om1 = builder.build_msa(msa, bg)
        one.creation_time = hmm.creation_time
        assert hmm == one
        assert np.array_equal(om.evalue_parameters.as_vector(), om1.evalue_parameters.as_vector())
        assert np.array_equal(om.rbv, om1.rbv) and np.array_equal(om.rwv, om1.rwv) and np.array_equal(om.rfv, om1.rfv)


def test_search_with_the_built_model(builder, models):
    bg = plan7.Background(mc.AMINO)
    built, _, _ = builder.build_msa(luxc_msa(), bg)
    with easel.SequenceFile(GOLDEN / "seqs" / "LuxC.faa", digital=True, alphabet=mc.AMINO) as sf:
        block = sf.read_block()
    got = list(hmmer.hmmsearch([built], block))[0]
    want = list(hmmer.hmmsearch([models["LuxC"][0]], block))[0]
    assert len(want) > 0 and [h.name for h in got] == [h.name for h in want]
    for a, b in zip(got, want):
        assert abs(a.score - b.score) <= 0.1, (a.name, a.score, b.score)


def test_refusals(builder):
    bg = plan7.Background(mc.AMINO)
    wide = mc.msa_of(["A" * 65536, "A" * 65536], name="wide")
    with pytest.raises(OverflowError, match="65,535"):
        builder.build_msa(wide, bg)
    ax = np.zeros((2 ** 20 + 1, 1), dtype=np.uint8)
    h = C.c_void_p()
    st = _lib.lib().p7x_msa_counts(3, ax.ctypes.data, ax.shape[0], 1, None, 1, 0.5, 0.5, 0, C.byref(h))
    assert st == 16 and "2^20" in _lib.last_error()
    dna = easel.DigitalMSA._from_rows(["a", "b"], ["ACGT", "ACGT"], ["", ""], ["", ""], alphabet=easel.Alphabet.dna())
    dna.name = "dna"
    with pytest.raises(errors.AlphabetMismatch):
        builder.build_msa(dna, bg)
    with pytest.raises(errors.AlphabetMismatch):
        builder.build_msa(luxc_msa(), plan7.Background(easel.Alphabet.dna()))
