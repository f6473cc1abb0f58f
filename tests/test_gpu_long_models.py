"""Models and phmmer queries beyond 8,192 nodes on the device: the tier of 192 nodes per lane of every
wave-per-target kernel (filters, parsers, envelope / ensemble / alignment kernels, calibration), through the public
interface, against the oracle and the host twins.  Lengths: the first model beyond the old limit, the last model of every
new tier and the first of the next, and p7x_max_model_length().  Targets are short (tests/long_models.py)."""
import functools
import sys
import time

import numpy as np
import pytest

import gap_models
import long_models
from pyhmmer_amd import _lib, easel, hmmer, plan7
from test_gpu_align import PP_TOL
from test_gpu_calibrate import FWD_TOL, TAU_MARGIN
from test_gpu_envelopes import ENV_TOL_BITS, ENV_TOL_REL_LONG
from test_gpu_filters import FWD_TOL_NATS, _oracle_scores
from test_host_builder import LENGTHS, N, fit, oracle_scores, sample, stream_of

pytestmark = pytest.mark.gpu

LONG_M = long_models.long_lengths()
BCK_TOL_NATS = 5e-3          # tests/test_gpu_filters.py: backward_parser against the oracle
TWINS = dict(host_envelopes=True, host_regions=True, host_ensembles=True)


@pytest.fixture(autouse=True, scope="module")
def _host_twin_in_the_device_order():
    """As tests/test_gpu_envelopes.py: the host twins sum in the device's lane-chunk order (option "host_order" = 1)."""
    _lib.set_debug_option("host_order", 1)
    yield
    _lib.set_debug_option("host_order", -1)


def test_lengths_are_beyond_the_old_limit():
    assert LONG_M[0] == 8193 and LONG_M[-1] == long_models.limit() and len(LONG_M) >= 2


# ------------------------------------------------------------------------------------------------ 1. filters
@pytest.mark.parametrize("M", LONG_M)
def test_filters_of_every_new_instantiation_vs_oracle(M, oracle):
    """MSV and Viterbi bit for bit, Forward within the project's bound, Backward's total score within the bound of
    test_gpu_filters: 90 background targets of 1 ... 419 residues and six fragments on the first lane, the last lane and
    lane boundaries."""
    hmm, bg, res, node, frags = long_models.case(M)
    blk = long_models.filter_block(M)
    om = plan7.OptimizedProfile(hmm, bg, 400)
    op = oracle.OracleProfile(hmm, bg, 400)
    t0 = time.perf_counter()
    got = plan7.SequenceDatabase(blk).filters(om, msv=True, viterbi=True, forward=True)
    t1 = time.perf_counter()
    want = _oracle_scores(op, blk, want=("msv", "vit", "fwd"))
    assert np.array_equal(got["xJ"], want["msv"]), f"M={M}: {np.nonzero(got['xJ'] != want['msv'])[0][:8]}"
    assert np.array_equal(got["xC"], want["vit"]), f"M={M}: {np.nonzero(got['xC'] != want['vit'])[0][:8]}"
    assert int((want["vit"][-6:] > want["vit"][:-6].max()).sum()) >= 5          # the fragments are what scores
    ok = np.isfinite(want["fwd"])
    assert np.array_equal(np.isfinite(got["fwd"]), ok)
    err = np.abs(got["fwd"][ok] - want["fwd"][ok])
    print(f"[long] M={M} filters {1e3 * (t1 - t0):.0f} ms, max |fwd - oracle| {err.max():.2e} nat", file=sys.stderr)
    assert np.all(err < FWD_TOL_NATS + 1e-5 * np.abs(want["fwd"][ok]))
    worst = 0.0
    for s in blk:
        st, bsc = op.bck(s.sequence)[:2]
        dev = om.backward_parser(s)
        if np.isfinite(bsc):
            worst = max(worst, abs(dev - bsc))
            assert dev == pytest.approx(bsc, abs=BCK_TOL_NATS), (M, s.name)
    print(f"[long] M={M} max |bck - oracle| {worst:.2e} nat", file=sys.stderr)


# ------------------------------------------------------------------------------------------------ 2. D chains
def test_viterbi_d_chains_across_192_node_lanes(oracle, monkeypatch):
    """A gap-rich model of 8,193 nodes (deletion corridors of more than three lanes' worth of nodes, tests/gap_models.py) and
    targets that are one domain only through a corridor: the D->D carry crosses lane boundaries of the 192-node layout."""
    M = 8193
    monkeypatch.setattr(gap_models, "_TIERS", gap_models._TIERS + long_models.NEW_TIERS)
    assert gap_models.stripe_nodes(M) == 192
    hmm = gap_models.gappy_hmm(M, seed=5000 + M)
    assert max(c1 - c0 for c0, c1 in gap_models.corridors(hmm)) >= 3 * 192
    bg = plan7.Background(hmm.alphabet)
    seqs = gap_models.with_background_neighbours(gap_models.bridge_targets(hmm, 60, seed=M), seed=M)
    blk = easel.DigitalSequenceBlock(hmm.alphabet, seqs)
    op = oracle.OracleProfile(hmm, bg, 400)
    want = np.array([op.vit(s.sequence)[2] for s in seqs])
    scalar = np.array([op.vit(s.sequence, scalar=True)[2] for s in seqs])
    built = np.array([s.name.startswith("bridge") for s in seqs])
    informative = int(((scalar > scalar[~built].max()) & (scalar < 32767)).sum())
    assert 4 * informative >= len(blk), (informative, len(blk))
    om = plan7.OptimizedProfile(hmm, bg, 400)
    got = plan7.SequenceDatabase(blk).filters(om, msv=False, viterbi=True)["xC"]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(blk[int(i)].name, int(got[i]), int(want[i])) for i in bad[:5]]
    assert np.array_equal(got, scalar)


# ------------------------------------------------------------------------------------------------ 3. / 4. envelopes
def _compare(hmm, db, **opts):
    """Device against the host twins, as _compare of tests/test_gpu_envelopes.py (its tolerances; every integer field and
    alignment string identical).  Returns (device hits, host-twin hits, domains compared)."""
    rtol = ENV_TOL_REL_LONG
    dev_hits = plan7.Pipeline(hmm.alphabet, **opts).search_hmm(hmm, db)
    host_hits = plan7.Pipeline(hmm.alphabet, **TWINS, **opts).search_hmm(hmm, db)
    dev = sorted(long_models.records(dev_hits), key=lambda r: r[0])
    host = sorted(long_models.records(host_hits), key=lambda r: r[0])
    assert [r[0] for r in dev] == [r[0] for r in host]
    ndom = 0
    for (name, sa, da), (_, sb, dbb) in zip(dev, host):
        assert np.allclose(sa, sb, atol=ENV_TOL_BITS, rtol=rtol), (name, sa, sb)
        assert len(da) == len(dbb), name
        for (ia, fa), (ib, fb) in zip(da, dbb):
            assert np.allclose(fa, fb, atol=ENV_TOL_BITS, rtol=rtol), (name, fa, fb)
            assert ia == ib, (name, ia, ib)
            ndom += 1
    return dev_hits, host_hits, ndom


@pytest.mark.parametrize("M", LONG_M)
def test_envelopes_ensembles_and_regions_equal_the_host_twins(M):
    """Pipeline.search_hmm on the device against host_envelopes + host_regions + host_ensembles: six fragments and three targets of
    two copies of a fragment around a 30-residue spacer; at least one of their regions is resolved by a traceback ensemble."""
    hmm, bg, res, node, frags = long_models.case(M)
    db = plan7.SequenceDatabase(long_models.domain_block(M))
    t0 = time.perf_counter()
    dev, host, ndom = _compare(hmm, db, E=1e3, domE=1e3)
    print(f"[long] M={M} three-stage comparison {time.perf_counter() - t0:.1f} s, {ndom} domains", file=sys.stderr)
    assert ndom >= 6
    twos = [h for h in host if h.name.startswith("two")]
    assert len(twos) == 3 and all(len(h.domains) >= 2 for h in twos)
    assert any(h.nclustered >= 1 for h in twos), [(h.name, h.nregions, h.nclustered, h.nenvelopes) for h in twos]     # a region was sampled
    by_name = {h.name: h for h in dev}
    for h in twos:
        d = by_name[h.name]
        assert (d.nregions, d.nclustered, d.nenvelopes) == (h.nregions, h.nclustered, h.nenvelopes), h.name
    assert dev.guard_counts["ens_device"] + dev.guard_counts["ens_redone"] >= 1, dev.guard_counts        # the ensemble kernel ran


@pytest.mark.parametrize("M", LONG_M)
def test_ensemble_kernel_equals_the_host_ensemble(M):
    """The ensemble kernels alone (multihit Forward fill and the walk) at every new tier: the two-copy targets, each as one
    region, sampled on the device and by the host twin: the same domains in the same order, the same null2 sums."""
    from test_gpu_ensembles import _same_ensemble
    hmm, bg, res, node, frags = long_models.case(M)
    seqs = long_models.two_domain_targets(M)
    db = plan7.SequenceDatabase(easel.DigitalSequenceBlock(hmm.alphabet, seqs))
    om = plan7.OptimizedProfile(hmm, bg, 400)
    assert sum(_same_ensemble(db, om, t, 1, len(s)) for t, s in enumerate(seqs)) >= 3 * 200


def test_full_length_self_hit():
    """The model's own emission as a target: one envelope of about 8,000 x 8,193 cells."""
    M = 8193
    hmm, bg, res, node, frags = long_models.case(M)
    abc = hmm.alphabet
    blk = easel.DigitalSequenceBlock(abc, [easel.DigitalSequence(abc, name="self", sequence=np.array(res))])
    assert len(blk[0]) >= 7800
    dev, host, ndom = _compare(hmm, plan7.SequenceDatabase(blk), E=1e3, domE=1e3)
    assert ndom >= 1 and len(dev) == 1
    a = max(dev[0].domains, key=lambda d: d.score).alignment
    assert a.hmm_to - a.hmm_from >= 7000


# ------------------------------------------------------------------------------------------------ 5. calibration
CAL_M = [300, 8192] + LONG_M


@pytest.fixture(scope="module")
def cal_world(libp7x, oracle):
    abc = easel.Alphabet.amino()
    bg = plan7.Background(abc)
    f = bg.residue_frequencies.astype(np.float64)
    rng = np.random.default_rng(78)
    builder = plan7.Builder(abc)
    stream = stream_of(bg)
    hmms = [builder._model(easel.DigitalSequence(abc, name=f"q{M}", sequence=rng.choice(abc.K, size=M, p=f / f.sum()).astype(np.uint8)), bg)
            for M in CAL_M]
    oms = [plan7.OptimizedProfile(h, bg, 100) for h in hmms]
    ev, raw = plan7._calibrate(oms, device=0, seed=42, want_scores=True)            # one batch mixing old and new tiers
    lens = np.concatenate([np.full(N, L, np.int32) for L in LENGTHS])
    offs = np.zeros(3 * N, np.int64)
    flat = [np.array([255], np.uint8)]
    pos = 1
    for st in range(3):
        for i in range(N):
            offs[st * N + i] = pos
            flat += [sample(stream, st, i), np.array([255], np.uint8)]
            pos += LENGTHS[st] + 1
    db = plan7.SequenceDatabase.from_packed(abc, np.concatenate(flat), offs, lens, device=0)
    cpu, par = [], []
    for h, om in zip(hmms, oms):
        mh = _lib.lib().p7x_oprofile_match_relent(om._handle)
        sc, ovf, xraw = oracle_scores(oracle.OracleProfile(h, bg, 100), stream)
        assert not ovf.any()
        cpu.append(dict(sc=sc, raw=xraw, ev=fit(sc, ovf, mh)[1], mh=mh))
        got = db.filters(om, msv=True, viterbi=True, forward=True)
        par.append(dict(xJ=got["xJ"][:N].copy(), xC=got["xC"][N:2 * N].copy(), fwd=got["fwd"][2 * N:].astype(np.float32).copy()))
    return dict(oms=oms, hmms=hmms, ev=ev, raw=raw, cpu=cpu, par=par)


def test_calibration_of_a_batch_mixing_old_and_new_tiers(cal_world):
    """Raw xJ / xC bit for bit the oracle's and p7x_filters_batch's, Forward equal to p7x_filters_batch and within 2e-3 nat of
    the oracle; mu and lambda equal to the CPU path, tau within TAU_MARGIN x the largest oracle-versus-p7x_filters_batch
    difference over these models, measured here (the rule of tests/test_gpu_calibrate.py)."""
    w = cal_world
    worst = 0.0
    for M, raw, cpu, par in zip(CAL_M, w["raw"], w["cpu"], w["par"]):
        assert np.array_equal(raw[0], cpu["raw"][0]) and np.array_equal(raw[0], par["xJ"]), M
        assert np.array_equal(raw[1], cpu["raw"][1]) and np.array_equal(raw[1], par["xC"]), M
        fwd = raw[2].view(np.float32)
        assert np.all(np.isfinite(fwd)), M
        d = float(np.max(np.abs(fwd - cpu["sc"][2])))
        assert d <= FWD_TOL, (M, d)
        assert np.array_equal(fwd, par["fwd"]), (M, float(np.max(np.abs(fwd - par["fwd"]))))
        sc = cpu["sc"].copy()
        sc[2] = par["fwd"]
        worst = max(worst, abs(float(fit(sc, None, cpu["mh"])[1][4]) - float(cpu["ev"][4])))
    print(f"[long] largest |tau(oracle) - tau(p7x_filters_batch)| over {len(CAL_M)} models: {worst:.3g}", file=sys.stderr)
    for M, om, h, ev, cpu in zip(CAL_M, w["oms"], w["hmms"], w["ev"], w["cpu"]):
        assert np.array_equal(ev[[0, 1, 2, 3, 5]], cpu["ev"][[0, 1, 2, 3, 5]]), (M, ev, cpu["ev"])
        assert abs(float(ev[4]) - float(cpu["ev"][4])) <= TAU_MARGIN * worst, (M, ev[4], cpu["ev"][4], worst)
        assert np.array_equal(om.evalue_parameters.as_vector(), ev) and np.array_equal(h._evparam, ev), M


def test_calibration_alone_equals_the_batch(cal_world):
    for M, om, raw, ev in zip(CAL_M, cal_world["oms"], cal_world["raw"], cal_world["ev"]):
        e1, r1 = plan7._calibrate([om], want_scores=True)
        assert np.array_equal(r1[0], raw) and np.array_equal(e1[0], ev), M


# ------------------------------------------------------------------------------------------------ 6. phmmer
def _flat(hits):
    return [(h.name, round(h.score, 4), round(h.bias, 4), h.evalue,
             [(d.score, d.i_evalue, d.c_evalue, d.env_from, d.env_to, d.alignment.hmm_from, d.alignment.hmm_to,
               d.alignment.target_from, d.alignment.target_to) for d in h.domains]) for h in hits]


@functools.lru_cache(maxsize=None)
def _phmmer_world():
    abc = easel.Alphabet.amino()
    p = plan7.Background(abc).residue_frequencies.astype(np.float64)
    p /= p.sum()
    rng = np.random.default_rng(9000)
    draw = lambda L: rng.choice(abc.K, size=L, p=p).astype(np.uint8)
    queries = [easel.DigitalSequence(abc, name=f"q{i}_{L}", sequence=draw(L)) for i, L in enumerate((300, 9000, 300))]
    seqs = list(queries)
    long_q = np.asarray(queries[1].sequence)
    for i in range(20):              # fragments of the long query: its start, its end, and lane boundaries of the 192-node layout
        lo = [0, 9000 - 400, 192 - 200, 23 * 192 - 200, 46 * 192 - 200][i] if i < 5 else int(rng.integers(0, 9000 - 400))
        L = 400 if i < 5 else int(rng.integers(150, 401))
        lo = max(0, lo)
        seqs.append(easel.DigitalSequence(abc, name=f"frag{i}", sequence=long_q[lo:lo + L].copy()))
    seqs += [easel.DigitalSequence(abc, name=f"bg{i}", sequence=draw(int(rng.integers(50, 400)))) for i in range(200)]
    return queries, easel.DigitalSequenceBlock(abc, seqs)


def test_phmmer_long_query_between_short_ones():
    queries, db = _phmmer_world()
    together = list(hmmer.phmmer(queries, db))
    assert len(together) == 3 and all(h.query is q for h, q in zip(together, queries))
    for q, hits in zip(queries, together):
        alone = next(hmmer.phmmer([q], db))
        assert _flat(hits) == _flat(alone), q.name
    long_hits = together[1]
    twin = next(hmmer.phmmer([queries[1]], db, **TWINS))
    dev = sorted(long_models.records(long_hits), key=lambda r: r[0])
    host = sorted(long_models.records(twin), key=lambda r: r[0])
    assert [r[0] for r in dev] == [r[0] for r in host] and len(dev) >= 21
    for (name, sa, da), (_, sb, dbb) in zip(dev, host):
        assert np.allclose(sa, sb, atol=ENV_TOL_BITS, rtol=ENV_TOL_REL_LONG), name
        assert len(da) == len(dbb), name
        for (ia, fa), (ib, fb) in zip(da, dbb):
            assert ia == ib, (name, ia, ib)
            assert np.allclose(fa, fb, atol=ENV_TOL_BITS, rtol=ENV_TOL_REL_LONG), (name, fa, fb)
    best, best_twin = long_hits[0], next(h for h in twin if h.name == queries[1].name)
    assert best.name == queries[1].name and len(best.domains) == 1
    a, b = best.domains[0].alignment, best_twin.domains[0].alignment
    assert (a.hmm_from, a.hmm_to, a.target_from, a.target_to) == (b.hmm_from, b.hmm_to, b.target_from, b.target_to)
    assert a.hmm_from == a.target_from and a.hmm_to == a.target_to and a.hmm_to - a.hmm_from >= 8900


def test_phmmer_query_beyond_the_limit_raises_at_its_position():
    queries, db = _phmmer_world()
    limit = long_models.limit()
    abc = db.alphabet
    rng = np.random.default_rng(5)
    too_long = easel.DigitalSequence(abc, name="too_long", sequence=rng.integers(0, abc.K, size=limit + 1).astype(np.uint8))
    it = hmmer.phmmer([queries[0], too_long, queries[2]], db)
    first = next(it)
    assert first.query is queries[0] and _flat(first) == _flat(next(hmmer.phmmer([queries[0]], db)))
    with pytest.raises(ValueError, match=str(limit)):
        next(it)


# ------------------------------------------------------------------------------------------------ 7. hmmalign
def test_hmmalign_traces_equal_the_host_twin():
    """TraceAligner.compute_traces at M = 8,193 (alignment mode of the envelope kernel, 192 nodes per lane): two full emissions
    and two fragments against host_align = 1."""
    M = 8193
    hmm, bg, res, node, frags = long_models.case(M)
    abc = hmm.alphabet
    res2, _ = long_models.emit_with_nodes(hmm, np.random.default_rng([16, M]))
    seqs = [easel.DigitalSequence(abc, name=n, sequence=np.array(s)) for n, s in
            (("full0", res), ("full1", res2), ("frag_first", frags[0]), ("frag_boundary", frags[3]))]
    block = easel.DigitalSequenceBlock(abc, seqs)
    aligner = plan7.TraceAligner()
    dev = aligner.compute_traces(hmm, block)
    _lib.set_debug_option("host_align", 1)
    try:
        host = plan7.TraceAligner().compute_traces(hmm, block)
    finally:
        _lib.set_debug_option("host_align", -1)
    assert len(dev) == len(host) == 4 and host.ndevice == 0
    assert dev.ndevice + dev.nflagged == 4 and dev.ndevice >= 1, (dev.ndevice, dev.nflagged)
    for s, d, h in zip(block, dev, host):
        assert np.array_equal(d.st, h.st) and np.array_equal(d.k, h.k) and np.array_equal(d.i, h.i), s.name
        assert float(np.abs(d.posterior_probabilities - h.posterior_probabilities).max()) <= PP_TOL, s.name
    md = aligner.align_traces(hmm, block, dev, all_consensus_cols=True)
    mh = aligner.align_traces(hmm, block, host, all_consensus_cols=True)
    assert md.alignment == mh.alignment and md.posterior_probabilities == mh.posterior_probabilities and md.pp_consensus == mh.pp_consensus
