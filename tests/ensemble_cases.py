"""The regions on which the stochastic-traceback ensembles are held to the float64 reference (test input only), shared by
tests/test_host_ensemble_reference.py and tests/test_gpu_ensemble_reference.py, with the reference of each computed once.

Tier cases: one random_hmm per tier C of nodes per lane of the Forward fill (P7X_NODE_TIERS), at the smallest length that
takes the tier (M = 64 C_prev + 1; M = 5 for C = 1), and M = 64 C for C = 1, 5 and 48 (the first rolled tier).  The target is
consensus fragments of FRAGMENT nodes between SPACER-residue spacers in descending model order (tests/tandem_targets.py: no
single pass through the model chains two of them, so the region is multi-domain and its Forward rows are rescaled): the
model's last FRAGMENT nodes, a fragment that starts on the first node of a lane (k = z C + 1) and one on node 1.  From C = 48
on the first of the three is left out and the region is 80 residues (the reference and the copied records stay small).

Gap-rich cases, where the I and D choice points carry weight: gap_models.gappy_hmm with bridge targets over its deletion
corridors and through its insert-rich node, and the long-insert model of tests/test_host_emit.py.  One background-only
target and one KR protein of three emitted copies complete the list.

Region-length cases (_len_case): the tier-2 model on regions of 63 / 64 / 65, 511 / 512 / 513 and 1,500 residues, the lengths
at which the walk kernel's C / J runs and its per-lane accumulators change path.

PLACEMENTS: the (case, LDS cap) pairs under which tests/test_gpu_ens_walk_placement.py runs the walk kernel, one for every
placement of its working set that the plan (p7x_ens_plan.hpp, through plan7.ens_walk_plan) yields for six of the cases;
tests/test_host_ens_walk_plan.py holds the list of placement classes they must cover."""
import contextlib
from types import SimpleNamespace

import numpy as np

import dp_reference as R
import ensemble_reference as ER
import gap_models
from conftest import load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, plan7

TIERS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 96, 128, 192)        # P7X_NODE_TIERS (p7x_kernels.hpp)
FULL_TIERS = (1, 5, 48)
FRAGMENT, SPACER = 30, 10
DIST_SEEDS = tuple(range(101, 126))                 # 25 x 200 samples for the distribution tests
EXACT_SEEDS = (42, 1, 7, 123456789)


def tier_lengths():
    """[(C, M)]: the smallest model of every tier, and the full ones of FULL_TIERS."""
    out = [(1, 5)] + [(c, 64 * p + 1) for p, c in zip(TIERS, TIERS[1:])] + [(c, 64 * c) for c in FULL_TIERS]
    assert all(next(t for t in TIERS if t >= (m + 63) // 64) == c for c, m in out)
    return out


TIER_NAMES = tuple(f"tier{c}_M{m}" for c, m in tier_lengths())
OTHER_NAMES = ("gappy", "long_insert", "background", "KR_x3")
LEN_MODEL = 65                                      # the model of tier2_M65
LEN_SPARSE, LEN_DENSE = (63, 64, 65, 511, 512, 1500), (513,)
LEN_NAMES = tuple(f"len{n}" for n in sorted(LEN_SPARSE + LEN_DENSE))
NAMES = TIER_NAMES + OTHER_NAMES + LEN_NAMES


def _consensus(hmm):
    return np.argmax(np.asarray(hmm.match_emissions)[1:], axis=1).astype(np.uint8)


def _spacer(rng, n=SPACER):
    return rng.integers(0, 20, size=n).astype(np.uint8)


def _tandem(rng, pieces):
    parts = [_spacer(rng)]
    for p in pieces:
        parts += [p, _spacer(rng)]
    return np.concatenate(parts)


def _tier_case(name, C, M):
    hmm = random_hmm(M, seed=7000 + M)
    rng = np.random.default_rng([M, 31])
    cons, n = _consensus(hmm), min(FRAGMENT, M)
    z = max(1, (M // C) // 2)
    lane_first = z * C + 1 if z * C + n <= M else 1                # node the lane-aligned fragment starts on
    starts = ([M - n + 1] if C < 48 else []) + [lane_first, 1]
    seq = _tandem(rng, [cons[k - 1:k - 1 + n] for k in starts])
    start, end = (1, len(seq)) if C < 48 else (6, 85)
    assert end - start + 1 <= (150 if C < 48 else 80) and end <= len(seq)
    return SimpleNamespace(name=name, hmm=hmm, seq=seq, start=start, end=end, lane_first=lane_first)


def _gappy_case():
    hmm = gap_models.gappy_hmm(120, 7)
    rng = np.random.default_rng(12)
    tg = gap_models.bridge_targets(hmm, 10, 3)
    pieces = [np.asarray(tg[i].sequence, dtype=np.uint8) for i in (3, 4, 0)]       # two corridors; an insert; one corridor
    seq = _tandem(rng, pieces)
    return SimpleNamespace(name="gappy", hmm=hmm, seq=seq, start=1, end=len(seq))


def _long_insert_case():
    from test_host_emit import long_insert_hmm
    hmm = long_insert_hmm()
    rng = np.random.default_rng(13)
    cons = _consensus(hmm)
    seq = _tandem(rng, [cons[10:30], np.concatenate([cons[:10], _spacer(rng, 25), cons[10:30]])])
    return SimpleNamespace(name="long_insert", hmm=hmm, seq=seq, start=1, end=len(seq))


def _background_case():
    hmm = random_hmm(100, seed=7100)
    seq = np.random.default_rng(14).integers(0, 20, size=60).astype(np.uint8)
    return SimpleNamespace(name="background", hmm=hmm, seq=seq, start=1, end=len(seq))


def _kr_case():
    hmm = load_hmms("KR")[0]
    rng = np.random.default_rng(15)
    copies = []
    for s in range(1, 40):                           # three sequences emitted by the model, none of them a short fragment
        e = np.asarray(hmm.emit_sequence(easel.Randomness(s, fast=True)).sequence, dtype=np.uint8)
        if hmm.M // 2 <= len(e) <= hmm.M + 20:
            copies.append(e)
        if len(copies) == 3:
            break
    seq = _tandem(rng, copies)
    return SimpleNamespace(name="KR_x3", hmm=hmm, seq=seq, start=1, end=len(seq))


def _len_case(name, Lr):
    """Region-length edges of the walk kernel on the tier-2 model, the full region 1..Lr: a C / J run looks at min(64, i) rows
    at once and lane l keeps the accumulators of residues l + 1 + 64 j, j < 8 (63 / 64 / 65; 511 / 512 / 513).  Sparse: three
    consensus fragments (nodes 36.., 33.., 1..) in background residues, four roughly equal spacers, so that the C / J runs
    between the domains are long.  Dense (513): tandem fragments between SPACER-residue spacers, cycling through the three
    start nodes, about ten domains per sample, so that finished domains keep moving over the accumulators' lanes."""
    hmm = random_hmm(LEN_MODEL, seed=7000 + LEN_MODEL)
    cons, starts = _consensus(hmm), (36, 33, 1)
    if Lr in LEN_DENSE:
        rng = np.random.default_rng([LEN_MODEL, Lr, 41])
        parts, total, z = [_spacer(rng)], SPACER, 0
        while total < Lr:
            k = starts[z % 3]
            parts += [cons[k - 1:k - 1 + FRAGMENT], _spacer(rng)]
            total, z = total + FRAGMENT + SPACER, z + 1
        seq = np.concatenate(parts)[:Lr]
    else:
        rng = np.random.default_rng([LEN_MODEL, Lr, 37])
        n = FRAGMENT if Lr >= 3 * FRAGMENT + 40 else (Lr - 8) // 3
        bg = Lr - 3 * n
        gaps = [bg // 4 + (1 if g < bg % 4 else 0) for g in range(4)]
        parts = [_spacer(rng, gaps[0])]
        for g, k in enumerate(starts, start=1):
            parts += [cons[k - 1:k - 1 + n], _spacer(rng, gaps[g])]
        seq = np.concatenate(parts)
    assert len(seq) == Lr
    return SimpleNamespace(name=name, hmm=hmm, seq=seq, start=1, end=Lr)


_cases, _refs = {}, {}


def case(name):
    if name not in _cases:
        if name in TIER_NAMES:
            c = _tier_case(name, *tier_lengths()[TIER_NAMES.index(name)])
        elif name in LEN_NAMES:
            c = _len_case(name, int(name[3:]))
        else:
            c = {"gappy": _gappy_case, "long_insert": _long_insert_case, "background": _background_case, "KR_x3": _kr_case}[name]()
        c.om = plan7.OptimizedProfile(c.hmm, plan7.Background(c.hmm.alphabet), 400)
        c.Lr = c.end - c.start + 1
        _cases[name] = c
    return _cases[name]


def reference(name):
    """The float64 reference of a case's region, computed once per session and left unchanged."""
    if name not in _refs:
        c = case(name)
        model = R.RefModel.from_oprofile(c.om)
        _refs[name] = ER.RegionReference(model, c.om.rfv.shape[1] // 4, c.seq, c.start, c.end)
    return _refs[name]


def seed_state(seed):
    """The generator state a region's 200 walks start from: easel.Randomness(seed, fast=True), whose stream
    tests/test_host_emit.py pins; the state is the deviate times 2^32."""
    rng = easel.Randomness(seed, fast=True)
    x0 = rng.getstate()[2]
    assert int(rng.random() * ER.TWO32) == (x0 * 69069 + 1) & 0xFFFFFFFF
    return x0


def block(names):
    abc = case(names[0]).hmm.alphabet
    return easel.DigitalSequenceBlock(abc, [easel.DigitalSequence(abc, name=n, sequence=case(n).seq) for n in names])


# ---- the host twin on a case, in either summation order, and the bounds the two test modules share
UPSTREAM, DEVICE = 0, 1
NSAMPLES = ER.NSAMPLES
FLOAT32_ORDERS = 2.0 ** -21          # the project's measured bound between the two float32 summation orders


@contextlib.contextmanager
def host_order(order):
    """The host twin sums in upstream's striped order (the default) or, order = DEVICE, in the kernels' lane-chunk order."""
    _lib.set_debug_option("host_order", 1 if order == DEVICE else -1)
    try:
        yield
    finally:
        _lib.set_debug_option("host_order", -1)


_records, _traces, _dref, _n2ref = {}, {}, {}, {}


def twin_records(name, order):
    if (name, order) not in _records:
        c = case(name)
        with host_order(order):
            _records[(name, order)] = plan7.ensemble_records(c.om, c.start, c.end, residues=c.seq)
    return _records[(name, order)]


def twin_traces(name, seed, order, keep=True):
    """(st, k, i, off, dom, n2) of the twin's 200 walks."""
    if (name, seed, order) in _traces:
        return _traces[(name, seed, order)]
    c = case(name)
    with host_order(order):
        got = plan7.ensemble_traces(c.om, c.seq, c.start, c.end, seed=seed)
    if keep:
        _traces[(name, seed, order)] = got
    return got


def d_ref(name):
    """Largest |T / 2^32 - q| of the upstream-order twin (the oracle's bits: tests/test_oracle_domains.py) over the choice
    points whose cell has a float64 posterior of at least ensemble_reference.FLOOR."""
    if name not in _dref:
        _dref[name] = reference(name).threshold_distance(*twin_records(name, UPSTREAM))
    return _dref[name][ER.FLOOR]


def threshold_bound(name):
    """What the device order (twin or kernel) is held to on the same cells: four times the upstream order's own distance,
    the margin of every float64-reference test here, and never less than the spread of the two float32 orders."""
    return max(4.0 * d_ref(name), FLOAT32_ORDERS)


def degeneracy(name):
    import oracle_lib
    return oracle_lib.degeneracy_sets(case(name).hmm.alphabet.K)


def null2_reference(name, seed, order):
    """Float64 null2 by trace summed over the twin's own 200 paths."""
    if (name, seed, order) not in _n2ref:
        st, k, i, off, dom, n2 = twin_traces(name, seed, order)
        _n2ref[(name, seed, order)] = reference(name).null2_sums(st, k, i, off, degeneracy(name))
    return _n2ref[(name, seed, order)]


def null2_ref_distance(name):
    """Largest |n2 - float64| of the upstream-order twin over the exact seeds and the region's residues."""
    return max(float(np.abs(twin_traces(name, s, UPSTREAM)[5][1:] - null2_reference(name, s, UPSTREAM)[1:]).max()) for s in EXACT_SEEDS)


def null2_bound(name, n2ref):
    """Per residue, for the device order: four times the upstream order's distance, or 200 float32 roundings of the sum."""
    return np.maximum(4.0 * null2_ref_distance(name), NSAMPLES * 2.0 ** -23 * n2ref)



# ---- the placements of the walk kernel's working set (p7x_ens_plan.hpp) that the cases are run under
PLACEMENT_CASES = ("tier2_M65", "KR_x3", "len513", "len1500", "tier48_M2049", "len63")
LDS_KB_RANGE = range(1, 129)                       # what option ens_lds_kb is swept over


def plan(name, lds_kb=None):
    """The plan of a case's region in a launch of its own (what SequenceDatabase.ensemble makes) under an LDS cap of lds_kb KiB."""
    c = case(name)
    return plan7.ens_walk_plan(c.hmm.M, c.Lr, lds_kb=lds_kb)


def placement_class(p):
    """rows R/r, residues S/s - the accumulators' home - odds F/f, Forward rows D/d; a capital means in LDS."""
    return f"{'R' if p.rows_in_lds else 'r'}{'S' if p.sq_in_lds else 's'}-{p.n2_home}-{'F' if p.rft_in_lds else 'f'}{'D' if p.md_in_lds else 'd'}"


def _placements():
    """[(case, lds_kb)]: for each case of PLACEMENT_CASES the smallest cap of every distinct placement of the five pieces, the
    smallest caps that give the smallest cache geometry (fewest match bits; fewest insert / delete bits) and the largest,
    and 128 KiB."""
    out = []
    for name in PLACEMENT_CASES:
        plans = {kb: plan(name, kb) for kb in LDS_KB_RANGE}
        keep, seen = set(), set()
        for kb in LDS_KB_RANGE:
            cls = placement_class(plans[kb])
            if cls not in seen:
                seen.add(cls)
                keep.add(kb)
        # (7 match bits always come with 7 insert / delete bits: 4 KiB are left at the least; 6 come with 8 match bits)
        geometry = {kb: (p.mbits, p.idbits) for kb, p in plans.items()}
        fewest_id = min(g[::-1] for g in geometry.values())[::-1]
        for g in (min(geometry.values()), fewest_id, max(geometry.values())):
            keep.add(min(kb for kb in LDS_KB_RANGE if geometry[kb] == g))
        keep.add(LDS_KB_RANGE[-1])
        out += [(name, kb) for kb in sorted(keep)]
    return out


PLACEMENTS = _placements()
