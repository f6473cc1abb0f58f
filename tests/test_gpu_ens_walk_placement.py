"""ens_walk_kernel (p7x_ensemble.hip) under every placement of its working set: row records, residues, null2 accumulators,
match odds and Forward rows each in LDS or in memory, the record caches from their minimum to their maximum, launches
beyond 64 KiB of LDS.  Every placement takes another code path of the walk; the product's 32 KiB cap reaches whichever the
shapes at hand happen to select, so the option "ens_lds_kb" is set here to reach each of them on purpose.

ensemble_cases.PLACEMENTS lists the (case, cap) pairs, built from the plan the kernel itself follows (p7x_ens_plan.hpp through
plan7.ens_walk_plan); tests/test_host_ens_walk_plan.py holds the plan's arithmetic and the placement classes the list must
cover.  Under each placement the walks are the device-order host twin's, integer for integer (the twin is held to float64
deviate by deviate in tests/test_host_ensemble_reference.py), the null2 sums lie within the host module's bound of float64
null2 by trace, and they equal the default placement's word for word: every residue's accumulator receives the same float
additions in the same order wherever it lives, from the same odds whichever memory they are read from.

Not reached at test size: cache_ok == false needs (Lr + 1)(M + 1) >= 2^27, a 4 GB workspace.  Nor is the overflow of a
region's domain records (status bit 16): no small region was found whose samples average more than 4 + 4 Lr / (M + 16)
domains."""
import numpy as np
import pytest

import ensemble_cases as EC
from conftest import load_hmms
from pyhmmer_amd import _lib, easel, plan7
from test_gpu_envelopes import _records, _repeat_protein

pytestmark = pytest.mark.gpu

CASES = tuple(dict.fromkeys(EC.PLACEMENT_CASES + EC.LEN_NAMES))
EDGES = ("len63", "len64", "len65", "len511", "len512", "len513")


@pytest.fixture
def lds_cap():
    """Sets option ens_lds_kb (KiB; -1: the library's default) and restores the default whatever happens."""
    try:
        yield lambda kb: _lib.set_debug_option("ens_lds_kb", kb)
    finally:
        _lib.set_debug_option("ens_lds_kb", -1)


@pytest.fixture(scope="module")
def db():
    return plan7.SequenceDatabase(EC.block(CASES))


@pytest.fixture
def report(capsys):
    def emit(line):
        with capsys.disabled():
            print("\n[ens-walk-placement] " + line, end="", flush=True)
    return emit


_default_n2 = {}


def _walk(db, name, seed):
    c = EC.case(name)
    return db.ensemble(c.om, CASES.index(name), c.start, c.end, seed=seed, device=True)


def _check(db, lds_cap, report, name, kb):
    p = EC.plan(name, kb)
    report(f"{name} ens_lds_kb {kb}: {EC.placement_class(p)}, caches {p.mbits} / {p.idbits} bits {'by row' if p.by_row else 'hashed'}, "
           f"lds_bytes {p.lds_bytes}")
    for seed in EC.EXACT_SEEDS:
        if (name, seed) not in _default_n2:
            lds_cap(-1)
            status, dom, n2 = _walk(db, name, seed)
            assert status == 0
            _default_n2[(name, seed)] = n2
        lds_cap(kb)
        status, dom, n2 = _walk(db, name, seed)
        lds_cap(-1)
        assert status == 0, (name, kb, seed, status)
        twin = EC.twin_traces(name, seed, EC.DEVICE)[4]
        assert dom.shape == twin.shape, (name, kb, seed, dom.shape, twin.shape)
        if not np.array_equal(dom, twin):
            bad = int(np.argmax((dom != twin).any(axis=1)))
            raise AssertionError((name, kb, seed, "domain", bad, dom[bad].tolist(), twin[bad].tolist()))
        want = EC.null2_reference(name, seed, EC.DEVICE)
        d = np.abs(n2[1:] - want[1:])
        assert (d <= EC.null2_bound(name, want)[1:]).all(), (name, kb, seed, float(d.max()))
        got, ref = n2.view(np.uint32), _default_n2[(name, seed)].view(np.uint32)
        if not np.array_equal(got, ref):
            bad = np.nonzero(got != ref)[0]
            raise AssertionError((name, kb, seed, "null2 sums differ from the default placement's", len(bad), int(bad[0]),
                                  float(n2[bad[0]]), float(_default_n2[(name, seed)][bad[0]])))


@pytest.mark.parametrize("name,kb", EC.PLACEMENTS, ids=[f"{n}-{kb}" for n, kb in EC.PLACEMENTS])
def test_every_placement_walks_the_twins_paths(db, lds_cap, report, name, kb):
    _check(db, lds_cap, report, name, kb)


@pytest.mark.parametrize("name", EDGES)
def test_region_length_edges_with_nothing_in_lds(db, lds_cap, report, name):
    """1 KiB: the launch gets its minimum and everything stays in memory, the accumulators of regions that would otherwise
    sit in registers included (their default placement runs in tests/test_gpu_ensemble_reference.py)."""
    p = EC.plan(name, 1)
    assert EC.placement_class(p) == "rs-global-fd" and "-global-" not in EC.placement_class(EC.plan(name))
    _check(db, lds_cap, report, name, 1)


def test_regions_of_one_launch_place_themselves_independently(lds_cap, report):
    """Twelve repeat proteins of 2 to 13 copies of the KR domain, regions of some 600 to 3,600 residues in one walk launch: the
    launch's LDS comes from the longest region, and every region places itself within it.  Whatever the cap, the search
    equals the search whose ensembles the host samples -- with the library's defaults, and with the near-threshold guard
    off, when no region goes back to the host and the kernel's own walks decide every envelope."""
    hmm = load_hmms("KR")[0]
    abc = hmm.alphabet
    seqs = [easel.DigitalSequence(abc, name=f"rep{n}", sequence=_repeat_protein(hmm, n, 1 + n % 3, 70 + n)) for n in range(2, 14)]
    db2 = plan7.SequenceDatabase(easel.DigitalSequenceBlock(abc, seqs))
    counts = lambda hits: [(h.nregions, h.nclustered, h.noverlaps, h.nenvelopes) for h in hits]
    with EC.host_order(EC.DEVICE):                  # the host samples in the kernels' summation order (tests/test_gpu_ensembles.py)
        host = plan7.Pipeline(abc, host_ensembles=True).search_hmm(hmm, db2)
        want, want_counts = _records(host), counts(host)
        assert sum(h.nclustered for h in host) > 0
        lens = [len(s) for s in seqs]
        for kb in (1, 24, 128):
            classes = sorted({EC.placement_class(plan7.ens_walk_plan(hmm.M, n, maxLr=max(lens), lds_kb=kb)) for n in lens})
            report(f"repeat proteins of {min(lens)} to {max(lens)} residues, ens_lds_kb {kb}: whole-target regions would be {classes}")
            lds_cap(kb)
            dev = plan7.Pipeline(abc).search_hmm(hmm, db2)
            exact = plan7.Pipeline(abc, ens_guard=0.0).search_hmm(hmm, db2)
            lds_cap(-1)
            assert _records(dev) == want, kb
            assert counts(dev) == want_counts, kb
            # ... and without the near-threshold guard, which hands a region with a close call back to the host (most regions
            # of this length have one): every region's own walks on the device, none redone, the same search
            g = exact.guard_counts
            report(f"ens_lds_kb {kb}: regions sampled on the device / redone by the host: with the guard {dev.guard_counts['ens_device']} / "
                   f"{dev.guard_counts['ens_redone']}, without {g['ens_device']} / {g['ens_redone']}")
            assert g["ens_device"] > 0 and g["ens_redone"] == 0, (kb, g)
            assert _records(exact) == want, kb
            assert counts(exact) == want_counts, kb
