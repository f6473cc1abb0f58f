"""Where ens_walk_kernel keeps each piece of a region's working set (p7x_ens_plan.hpp, through the host-only seam
p7x_debug_ens_walk_plan / plan7.ens_walk_plan): the arithmetic the kernel, the host's LDS budget and the tests share.  No GPU:
tests/test_gpu_ens_walk_placement.py runs the kernel under every placement listed here.

The invariants are held over a grid of model lengths, region lengths and LDS caps.  The coverage condition pins which
placement classes ensemble_cases.PLACEMENTS reaches: a change to the arithmetic that makes one unreachable fails here and
says which one.

Out of reach at test size, and therefore in no class below: cache_ok == false (cell numbers beyond the caches' 27-bit tags)
needs (Lr + 1)(M + 1) >= 2^27, a 4 GB workspace."""
import itertools

import pytest

import ensemble_cases as EC
from pyhmmer_amd import _lib, plan7

GRID_M = (1, 5, 64, 65, 262, 513, 2049, 6145, 8193, 12288)
GRID_LR = (1, 31, 32, 63, 64, 65, 130, 511, 512, 513, 841, 1500, 5000, 20000)
CAPS = (None,) + tuple(range(1, 129))
DEFAULT_MOST = 32 * 1024
CACHE_MIN = 4096


@pytest.mark.parametrize("M", GRID_M)
def test_plan_invariants(libp7x, M):
    for Lr, kb in itertools.product(GRID_LR, CAPS):
        p = plan7.ens_walk_plan(M, Lr, lds_kb=kb)
        at = (M, Lr, kb, p)
        secs = [(name, *p.sections[name]) for name in plan7.ENS_WALK_SECTIONS if p.sections[name] is not None]
        assert all(off % 16 == 0 for _, off, _ in secs), at                                   # 16-byte aligned
        assert secs[0][1] == 0
        for (_, off, size), (_, nxt, _) in zip(secs, secs[1:]):                               # in order, no overlap
            assert size > 0 and off + size <= nxt, at
        before = [s for s in secs if s[0] not in ("mcache", "idcache")]
        assert before[-1][1] + before[-1][2] <= p.used_before_caches <= p.lds_bytes - CACHE_MIN, at
        assert p.sections["mcache"] == (p.used_before_caches, 16 << p.mbits) and p.sections["idcache"][1] == 16 << p.idbits, at
        assert p.sections["idcache"][0] + p.sections["idcache"][1] == p.used_after_caches <= p.lds_bytes, at
        assert 7 <= p.mbits <= 12 and 6 <= p.idbits <= 10, at
        assert p.lds_bytes >= p.least, at
        if kb is None:
            assert p.lds_bytes <= max(p.least, DEFAULT_MOST), at
        else:
            assert p.lds_bytes == max(p.least, min(p.want, kb * 1024)), at
        # what is in LDS has a section, what is not has none
        assert (p.sections["rows"] is not None) == (p.sections["norm"] is not None) == p.rows_in_lds, at
        assert (p.sections["sq"] is not None) == p.sq_in_lds and (p.sections["n2"] is not None) == (p.n2_home == "lds"), at
        assert (p.sections["rft"] is not None) == p.rft_in_lds and (p.sections["md"] is not None) == p.md_in_lds, at
        if p.rows_in_lds:
            assert p.sections["rows"][1] == 16 * (Lr + 1) and p.sections["norm"][1] == 4 * (Lr + 1), at
        if p.sq_in_lds:
            assert p.sections["sq"][1] == Lr, at
        if p.n2_home == "lds":
            assert p.sections["n2"][1] == 4 * (Lr + 1), at
        if p.rft_in_lds:
            assert p.sections["rft"][1] == 128 * (M + 1), at
        if p.md_in_lds:
            assert p.sections["md"][1] == 64 * (M + 1), at
        assert p.sections["cnt"][1] >= 4 * (M + 2), at
        if p.n2_home == "regs":
            assert Lr <= 512 and p.sq_in_lds, at
        assert p.by_row == (Lr < 2 ** (p.mbits - 2)), at
        assert p.cache_ok == ((Lr + 1) * (M + 1) < 2 ** 27 - 2), at


def test_a_region_of_a_larger_launch_plans_inside_the_launchs_budget(libp7x):
    """The launch's LDS comes from its longest model and region; a shorter region of it places itself within that."""
    for kb in (None, 1, 24, 128):
        big = plan7.ens_walk_plan(262, 3600, lds_kb=kb)
        small = plan7.ens_walk_plan(65, 130, maxM=262, maxLr=3600, lds_kb=kb)
        assert small.lds_bytes == big.lds_bytes and small.used_after_caches <= small.lds_bytes
        assert small.least == big.least and small.want == big.want
    with pytest.raises(Exception):
        plan7.ens_walk_plan(65, 130, maxM=64)
    with pytest.raises(Exception):
        plan7.ens_walk_plan(65, 130, maxLr=129)
    with pytest.raises(Exception):
        plan7.ens_walk_plan(0, 130)


def test_unset_cap_honours_the_option(libp7x):
    try:
        _lib.set_debug_option("ens_lds_kb", 77)
        assert plan7.ens_walk_plan(262, 841) == plan7.ens_walk_plan(262, 841, lds_kb=77)
        assert plan7.ens_walk_plan(262, 841, lds_kb=9) != plan7.ens_walk_plan(262, 841, lds_kb=77)
    finally:
        _lib.set_debug_option("ens_lds_kb", -1)
    assert plan7.ens_walk_plan(262, 841) == plan7.ens_walk_plan(262, 841, lds_kb=32)


# ------------------------------------------------------------------------------------------------ coverage of PLACEMENTS
SHORT = ("rs-global-fd", "rS-regs-fd", "RS-regs-fd", "RS-regs-fD", "RS-regs-Fd", "RS-regs-FD")
LONG = ("rs-global-fd", "rS-global-fd", "rS-lds-fd", "Rs-global-fd", "RS-global-fd", "RS-lds-fd", "RS-lds-fD", "RS-lds-Fd", "RS-lds-FD")
REQUIRED = [("tier2_M65", c) for c in SHORT] + [("KR_x3", c) for c in LONG] + [("len1500", "rS-global-fD"), ("len1500", "rS-lds-FD")]


def _plans():
    return {(name, kb): EC.plan(name, kb) for name, kb in EC.PLACEMENTS}


def test_placements_cover_every_class(libp7x):
    plans = _plans()
    assert EC.case("tier2_M65").Lr == 130 and EC.case("KR_x3").Lr == 841 and EC.case("KR_x3").hmm.M == 262
    reached = {(name, EC.placement_class(p)) for (name, kb), p in plans.items()}
    missing = [rc for rc in REQUIRED if rc not in reached]
    assert not missing, f"placement classes no entry of PLACEMENTS reaches: {missing}"
    caches = {
        "7 match bits, hashed": any(p.mbits == 7 and not p.by_row for p in plans.values()),
        "by row at 8 bits or fewer (len63)": any(n == "len63" and p.by_row and p.mbits <= 8 for (n, _), p in plans.items()),
        "12 / 10 bits by row (tier48_M2049 at 128)": (lambda p: p.mbits == 12 and p.idbits == 10 and p.by_row)(plans[("tier48_M2049", 128)]),
        "at least 11 bits, hashed (KR_x3 at 128)": (lambda p: p.mbits >= 11 and not p.by_row)(plans[("KR_x3", 128)]),
        "the caches at their minimum, 7 / 7 bits (4 KiB) and 8 / 6": {(7, 7), (8, 6)} <= {(p.mbits, p.idbits) for p in plans.values()},
    }
    assert all(caches.values()), [k for k, v in caches.items() if not v]
    assert sum(p.lds_bytes > 65536 for p in plans.values()) >= 2
    assert all((name, 128) in plans for name in EC.PLACEMENT_CASES)
    assert len(set(EC.PLACEMENTS)) == len(EC.PLACEMENTS)


def test_the_default_placements_of_the_reference_cases(libp7x, capsys):
    """What the suite reaches without the option: reported, and the region-length cases sit where their edges matter --
    accumulators in registers up to 512 residues, elsewhere beyond."""
    classes = {name: EC.placement_class(EC.plan(name)) for name in EC.NAMES}
    with capsys.disabled():
        print("\n[ens-walk-plan] default placements: " + ", ".join(f"{n} {c}" for n, c in classes.items()), end="", flush=True)
    for n in (63, 64, 65, 511, 512):
        assert "-regs-" in classes[f"len{n}"]
    assert "-regs-" not in classes["len513"] and "-regs-" not in classes["len1500"]
