"""CPU tests of the scan orientation of long targets (nhmmscan): the collect rule of p7x_scan_collect_longtargets -- a
model's hits are those of its lone nhmmer search, E-values times the number of models, thresholds on the scaled values --,
the launch plan of the batched SSV scan (p7x_debug_ssv_batch_plan), and the errors of the Python entry points that need no
device.  The per-model lists come from the CPU seam of the nhmmer tests: the oracle's sequential SSV scan seeds the
windows, the product's host tail (p7x_longtarget_from_seeds) does the rest."""
import ctypes as C
import io
import math

import numpy as np
import pytest

import host_pipeline
from conftest import GOLDEN, golden_table, load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, errors, hmmer, plan7

BGC = "BGC0001090.gbk"
CONTIG = "1390.SAMEA104415756.OFHT01000022.fna"


def _read(name, alphabet):
    with easel.SequenceFile(GOLDEN / "seqs" / name, digital=True, alphabet=alphabet) as f:
        return f.read_block()


def _cut_model(full, lo, hi, name):
    """Nodes lo+1 .. hi of <full> as a model of their own (as tests/test_host_longtarget.py makes one), with a window length."""
    h = plan7.HMM(full.alphabet, hi - lo, name)
    h.transition_probabilities[1:] = full.transition_probabilities[lo + 1:hi + 1]
    h.transition_probabilities[0] = full.transition_probabilities[0]
    h.match_emissions[1:] = full.match_emissions[lo + 1:hi + 1]
    h.insert_emissions[:] = full.insert_emissions[lo:hi + 1]
    t = np.array(h.transition_probabilities[hi - lo])
    t[0], t[2] = t[0] + t[2], 0.0
    t[5], t[6] = 1.0, 0.0
    h.transition_probabilities[hi - lo] = t
    h.composition = full.composition
    h.consensus = full.consensus[lo:hi]
    h._evparam[:] = full._evparam
    # the window length hmmbuild would have written (p7_Builder_MaxLength): a search with an HMM query replaces hmm.max_length by
    # it (reference plan7.pyx:7346-7354), so any other value would make a model's second search differ from its first
    view, keep = h._view()
    w = C.c_int32()
    assert _lib.lib().p7x_hmm_max_length(C.byref(view), 1e-7, C.byref(w)) == 0
    h.max_length = int(w.value)
    return h


_SEEDS = {}          # (model key, target, strand filter, max_length, F1, block_length) -> the oracle's seeds per unit: the slow part, once


def lone(oracle, hmm, seqs, pipeline=None, key=None, unfinished=False):
    """tests/host_pipeline.py::host_nhmmer restated with the oracle's seeds kept between calls; unfinished: the list as one
    part of two that happens to hold every unit (cfg.lt_nparts = 2): no E-values, duplicates or thresholds yet."""
    pipeline = pipeline or plan7.LongTargetsPipeline(hmm.alphabet)
    bg = pipeline.background
    om = plan7.OptimizedProfile(hmm, bg, 400)
    max_length = pipeline.window_length or hmm.max_length
    dsq, offsets, lengths, names, accs, descs = plan7.LongTargetsPipeline._pack(seqs)
    ck = (key or hmm.name, seqs[0].name, pipeline.strand, max_length, pipeline.F1, pipeline.block_length)
    if ck not in _SEEDS:
        op = oracle.OracleProfile(hmm, bg, 400)
        units = []
        for t, s in enumerate(seqs):
            seq = np.asarray(s.sequence, dtype=np.uint8)
            for (i, n) in host_pipeline.blocks_of(len(seq), pipeline.block_length, max_length):
                for strand in (0, 1):
                    if (strand == 0 and pipeline.strand == "crick") or (strand == 1 and pipeline.strand == "watson"):
                        continue
                    blk = seq[i:i + n] if strand == 0 else host_pipeline.DNA_COMP[seq[i:i + n][::-1]]
                    units.append((t, i, strand, list(oracle.ssv_longtarget(op, blk, max_length, pipeline.F1))))
        _SEEDS[ck] = units
    units = _SEEDS[ck]
    cfg = pipeline._cfg()
    if unfinished:
        assert len(units) == 1                      # the one unit goes to part 0 of 2
        cfg.lt_part, cfg.lt_nparts = 0, 2
    st_t, st_b, st_s, seeds = [], [], [], []
    for (t, i, strand, sds) in units:
        for sd in sds:
            st_t.append(t); st_b.append(i); st_s.append(strand); seeds.append(sd)
    a_t = np.array(st_t or [0], dtype=np.int64); a_b = np.array(st_b or [0], dtype=np.int64); a_s = np.array(st_s or [0], dtype=np.int32)
    a_seeds = np.ascontiguousarray(np.array(seeds if seeds else [[0, 0, 0]], dtype=np.int64).reshape(-1, 3))
    out = C.c_void_p()
    st = _lib.lib().p7x_longtarget_from_seeds(C.byref(cfg), om._handle, dsq.ctypes.data, offsets.ctypes.data, lengths.ctypes.data,
                                              len(seqs), names, accs, descs, a_t.ctypes.data, a_b.ctypes.data, a_s.ctypes.data,
                                              a_seeds.ctypes.data, len(seeds), C.byref(out))
    assert st == 0, _lib.last_error()
    hits = plan7.TopHits(hmm, out)
    hits._keep = (om, names, accs, descs, dsq)
    return hits


def collect(per_model, seq, pipeline, total, index=None, handle=None):
    """p7x_scan_collect_longtargets over TopHits objects; returns the handle (total == 0) or the finished TopHits."""
    n = len(per_model)
    arr = (C.c_void_p * max(n, 1))(*[h._handle.value for h in per_model])
    idx = None if index is None else np.array(index, dtype=np.int64)
    cfg = pipeline._cfg()
    inout = C.c_void_p(handle.value if handle is not None else None)
    st = _lib.lib().p7x_scan_collect_longtargets(arr, None if idx is None else idx.ctypes.data, n, total, C.byref(cfg), seq.name.encode(),
                                                 (seq.accession or "").encode(), (seq.description or "").encode(), len(seq), C.byref(inout))
    assert st == 0, _lib.last_error()
    if total == 0:
        return inout
    hits = plan7.TopHits(seq, inout)
    hits._keep = per_model
    return hits


def fields(h):
    d = h.domains[0]
    a = d.alignment
    return (a.hmm_from, a.hmm_to, a.target_from, a.target_to, d.env_from, d.env_to, d.strand, h.score, d.score, d.bias, h.bias, h.duplicate,
            a.hmm_sequence, a.target_sequence, a.identity_sequence)


@pytest.fixture(scope="module")
def library(libp7x):
    full = load_hmms("bmyD")[0]
    return [full, load_hmms("RF00001")[0], _cut_model(full, 400, 440, "bmyD_40"), _cut_model(full, 850, 1193, "bmyD_tail"),
            _cut_model(full, 100, 300, "bmyD_200")]


@pytest.mark.parametrize("target", [BGC, CONTIG])
def test_collect_rule(library, oracle, target):
    """Every model's hits in the collected list are its lone search's -- every coordinate, strand, score, bias and alignment
    string equal --, E-values and lnP times the number of models, named after the model, and the list is sorted by key."""
    seqs = _read(target, library[0].alphabet)
    pli = plan7.LongTargetsPipeline(library[0].alphabet)
    alone = [lone(oracle, m, seqs) for m in library]
    scan = collect(alone, seqs[0], pli, len(library))
    assert scan.mode == "scan" and scan.long_targets and scan.searched_models == len(library) and scan.query is seqs[0]
    assert scan.searched_residues == 2 * len(seqs[0]) and scan.searched_nodes == sum(m.M for m in library)
    assert len(scan) == sum(len(a) for a in alone) and len(scan) >= 3
    assert scan.is_sorted() and [h.evalue for h in scan] == sorted(h.evalue for h in scan)
    for m, a in zip(library, alone):
        mine = [h for h in scan if h.name == m.name]
        assert sorted(map(fields, mine)) == sorted(map(fields, a))
        assert all((h.accession, h.description) == (m.accession, m.description) for h in mine)
        by_pos = {fields(h)[:7]: h for h in a}
        for h in mine:
            w = by_pos[fields(h)[:7]]
            assert h.evalue == pytest.approx(w.evalue * len(library), rel=1e-6)
            assert h.domains[0].i_evalue == pytest.approx(w.domains[0].i_evalue * len(library), rel=1e-6)
            assert h._rec.lnP == pytest.approx(w._rec.lnP + math.log(len(library)), rel=1e-6)
            assert h.domains[0]._rec.lnP == pytest.approx(w.domains[0]._rec.lnP + math.log(len(library)), rel=1e-6)
            # the thresholds acted on the scaled values
            assert h.reported == (not h.duplicate and h.evalue <= 10.0) and h.included == (h.reported and h.evalue <= 0.01)
    # both strands are there on the contig
    if target == CONTIG:
        assert {h.domains[0].strand for h in scan} == {"+", "-"}


def rounds_to(value, text):
    decimals = len(text.split(".")[1]) if "." in text else 0
    return abs(value - float(text)) <= 0.5 * 10.0 ** -decimals + 1e-4


def check_scan_table(hits, rows):
    """tests/test_host_longtarget.py::check_nhmmer_table with the roles exchanged: the hit is the model (the table's query
    column), the sequence is the table's target."""
    reported = [h for h in hits if h.reported]
    assert len(reported) == len(rows)
    for row, hit in zip(rows, reported):
        d = hit.best_domain
        assert hit.name == row[2] and hits.query.name == row[0]
        assert (hit.accession or "-") == row[3]
        assert (d.alignment.hmm_from, d.alignment.hmm_to) == (int(row[4]), int(row[5]))
        assert (d.alignment.target_from, d.alignment.target_to) == (int(row[6]), int(row[7]))
        assert (d.env_from, d.env_to) == (int(row[8]), int(row[9]))
        assert hit.length == int(row[10]) and d.strand == row[11]
        assert rounds_to(d.bias, row[14]), (d.bias, row[14])
        assert rounds_to(d.score, row[13]), (d.score, row[13])
        assert d.i_evalue == pytest.approx(float(row[12]), abs=0.1)
        if float(row[12]) > 0:
            assert float("%.2g" % d.i_evalue) == pytest.approx(float(row[12]), rel=0.045), (d.i_evalue, row[12])


def check_written_rows(hits):
    """TopHits.write("targets") of a long-target scan: nhmmer's columns with the roles exchanged, against the hit objects."""
    buf = io.BytesIO()
    hits.write(buf)
    lines = buf.getvalue().decode().splitlines()
    reported = [h for h in hits if h.reported]
    if not reported:
        assert lines == []
        return
    assert lines[0].split()[1:3] == ["target", "name"] and "modlen" in lines[0] and "strand" in lines[0] and lines[1].startswith("#")
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    assert len(rows) == len(reported)
    for row, h in zip(rows, reported):
        d = h.best_domain
        assert row[:4] == [h.name, h.accession or "-", hits.query.name, hits.query.accession or "-"]
        assert [int(x) for x in row[4:10]] == [d.alignment.hmm_from, d.alignment.hmm_to, d.alignment.target_from, d.alignment.target_to, d.env_from, d.env_to]
        assert int(row[10]) == d.alignment.hmm_length and row[11] == d.strand
        assert row[12] == ("%9.2g" % h.evalue).strip() and row[13] == "%.1f" % h.score and row[14] == "%.1f" % d.bias
    nohead = io.BytesIO()
    hits.write(nohead, header=False)
    assert nohead.getvalue().decode().splitlines() == [ln for ln in lines if not ln.startswith("#")]


def test_one_model_library_reproduces_the_nhmmer_table(library, oracle):
    """log(1) = 0: the scan of a one-model library is the model's nhmmer search with the roles exchanged (bmyD1.tbl); an
    unfinished per-model list (one part of a search) is finished as the lone search finishes it."""
    hmm = library[0]
    seqs = _read(BGC, hmm.alphabet)
    pli = plan7.LongTargetsPipeline(hmm.alphabet)
    scan = collect([lone(oracle, hmm, seqs)], seqs[0], pli, 1)
    check_scan_table(scan, golden_table("bmyD1.tbl"))
    check_written_rows(scan)
    assert [h.evalue for h in scan] == [h.evalue for h in lone(oracle, hmm, seqs)]
    back = plan7.TopHits.from_bytes(scan.to_bytes(), query=seqs[0])
    assert [fields(h) for h in back] == [fields(h) for h in scan] and back.mode == "scan" and back.long_targets
    # an unfinished list: the watson strand as part 0 of 2
    pw = plan7.LongTargetsPipeline(hmm.alphabet, strand="watson")
    part = lone(oracle, hmm, seqs, pw, unfinished=True)
    whole = lone(oracle, hmm, seqs, pw)
    got = collect([part], seqs[0], pw, 1)
    assert [fields(h) + (h.evalue, h.reported, h.included) for h in got] == [fields(h) + (h.evalue, h.reported, h.included) for h in whole]
    assert len(got.reported) == 1 and got.strand == "watson" and got.searched_residues == len(seqs[0])


def test_thresholds_act_on_the_scaled_values(library, oracle):
    """bmyD2.tbl: the third row has E = 1.4 and the second 0.0063.  In a library of 8 models they are 11 and 0.05: the first
    is no longer reported under E = 10 (it is under E = 100), the second no longer included under incE = 0.01 (it is under 0.1)."""
    hmm = library[0]
    seqs = _read(CONTIG, hmm.alphabet)
    rows = golden_table("bmyD2.tbl")
    assert float(rows[2][12]) == 1.4 and float(rows[1][12]) == 0.0063
    alone = lone(oracle, hmm, seqs)
    assert len(alone.reported) == 3 and len(alone.included) == 2
    at = lambda hits, row: next(h for h in hits if (h.domains[0].alignment.target_from, h.domains[0].alignment.target_to) == (int(row[6]), int(row[7])))
    scan = collect([alone], seqs[0], plan7.LongTargetsPipeline(hmm.alphabet), 8)
    third, second = at(scan, rows[2]), at(scan, rows[1])
    assert third.evalue == pytest.approx(8 * at(alone, rows[2]).evalue, rel=1e-6) and 10.0 < third.evalue < 12.0
    assert not third.reported and not third.included and not third.domains[0].reported
    assert second.reported and not second.included and 0.01 < second.evalue < 0.1
    assert len(scan.reported) == 2 and len(scan.included) == 1
    loose = plan7.LongTargetsPipeline(hmm.alphabet, E=100.0, domE=100.0, incE=0.1, incdomE=0.1)
    scan = collect([lone(oracle, hmm, seqs, loose)], seqs[0], loose, 8)
    third, second = at(scan, rows[2]), at(scan, rows[1])
    assert third.reported and third.domains[0].reported and not third.included and second.included and second.domains[0].included
    assert len(scan.reported) >= 3 and len(scan.included) == 2


def test_duplicates_are_removed_within_a_model_only(library, oracle):
    """The same model under two names: both sets of hits stay, although they lie on top of each other."""
    hmm = library[0]
    twin = hmm.copy()
    twin.name = b"bmyD_twin" if isinstance(hmm.name, bytes) else "bmyD_twin"
    seqs = _read(CONTIG, hmm.alphabet)
    a, b = lone(oracle, hmm, seqs), lone(oracle, twin, seqs, key=hmm.name)
    scan = collect([a, b], seqs[0], plan7.LongTargetsPipeline(hmm.alphabet), 2)
    one, two = [h for h in scan if h.name == hmm.name], [h for h in scan if h.name == twin.name]
    assert len(one) == len(two) == len(a) and [fields(h) for h in one] == [fields(h) for h in two]
    assert sum(h.duplicate for h in one) == sum(h.duplicate for h in two) == sum(h.duplicate for h in a)
    assert len(scan.reported) == 2 * len([h for h in a if h.evalue * 2 <= 10.0 and not h.duplicate])


def test_batches_and_model_order_do_not_change_the_result(library, oracle):
    seqs = _read(BGC, library[0].alphabet)
    pli = plan7.LongTargetsPipeline(library[0].alphabet)
    alone = [lone(oracle, m, seqs) for m in library]
    n = len(library)
    image = lambda hits: [(h.name, h.evalue, h.reported, h.included) + fields(h) for h in hits]
    whole = collect(alone, seqs[0], pli, n)
    assert len(whole) >= 3
    # two batches, the size known only at the end
    handle = collect(alone[:2], seqs[0], pli, 0)
    handle = collect(alone[2:], seqs[0], pli, 0, handle=handle)
    two = collect([], seqs[0], pli, -1, handle=handle)
    assert image(two) == image(whole) and two.searched_models == n
    # the size known before: the last batch finishes
    handle = collect(alone[:3], seqs[0], pli, 0)
    assert image(collect(alone[3:], seqs[0], pli, n, handle=handle)) == image(whole)
    # another order of the models, with and without their numbers
    perm = [3, 0, 4, 2, 1]
    assert image(collect([alone[i] for i in perm], seqs[0], pli, n, index=perm)) == image(whole)
    assert image(collect([alone[i] for i in perm], seqs[0], pli, n)) == image(whole)
    # an empty library: an empty finished list
    none = collect([], seqs[0], pli, -1)
    assert len(none) == 0 and none.mode == "scan" and none.searched_models == 0
    # a finished scan list takes no more models, and a scan list is not a per-model list
    cfg = pli._cfg()
    arr = (C.c_void_p * 1)(alone[0]._handle.value)
    inout = C.c_void_p(whole._handle.value)
    assert _lib.lib().p7x_scan_collect_longtargets(arr, None, 1, 0, C.byref(cfg), b"x", b"", b"", 10, C.byref(inout)) != 0
    arr = (C.c_void_p * 1)(whole._handle.value)
    inout = C.c_void_p(None)
    assert _lib.lib().p7x_scan_collect_longtargets(arr, None, 1, 1, C.byref(cfg), b"x", b"", b"", 10, C.byref(inout)) != 0


# ------------------------------------------------------------------------------------------------ the launch plan
TILES = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 20, 24, 32, 48)       # p7x_ssvlong.hip: P7X_SSV_R


def batch_plan(M, slack):
    M = np.ascontiguousarray(M, dtype=np.int32); slack = np.ascontiguousarray(slack, dtype=np.int32)
    n = len(M)
    of = np.full(n, -7, dtype=np.int32)
    R = np.zeros(64, dtype=np.int32); pair = np.zeros(64, dtype=np.int32); lds = np.zeros(64, dtype=np.int64)
    limit = C.c_int64()
    k = _lib.lib().p7x_debug_ssv_batch_plan(M.ctypes.data, slack.ctypes.data, n, of.ctypes.data, R.ctypes.data, pair.ctypes.data, lds.ctypes.data, 64,
                                            C.byref(limit))
    assert k >= 0, _lib.last_error()
    return of, R[:k], pair[:k], lds[:k], limit.value


def tile_of(M, pair):
    """ssvlong_pick_R restated: the smallest tile whose 64 R registers hold cells up to M (+ 1, the virtual node of PAIR)."""
    need = (M + (1 if pair else 0) + 1) // 2 + 1
    return next(r for r in TILES if 64 * r >= need)


@pytest.fixture
def options(libp7x):
    yield _lib.set_debug_option
    for name in ("ssv_kernel", "ssv_parts", "ssv_scan_chunk"):
        _lib.set_debug_option(name, -1)


def test_launch_plan(options):
    """Model lengths at both ends of every register tile for both row flavours, losses per row below and above 16: every
    batchable model is in exactly one launch, a launch's models share (R, PAIR), no launch asks for more LDS than the
    kernel's widest tile; 6,141 nodes are batched, 6,142 go through the chained parts."""
    Ms = sorted({m for r in TILES for m in (128 * r - 3, 128 * r - 2, 128 * (r - 1) - 1 if r > 2 else 1, 128 * (r - 1) if r > 2 else 2) if 1 <= m <= 6142} | {1, 6141, 6142})
    M, slack = [], []
    for m in Ms:
        for s in (9, 16, 17, 80):
            M.append(m); slack.append(s)
    of, R, pair, lds, limit = batch_plan(M, slack)
    assert limit == 2 * 4 * 12 * 64 * 16 <= 160 * 1024 and all(0 < b <= limit for b in lds)
    assert len({(int(r), int(p)) for r, p in zip(R, pair)}) == len(R)              # one launch per group
    seen_tiles = set()
    for m, s, g in zip(M, slack, of):
        if m > 6141:
            assert g == -1
            continue
        assert 0 <= g < len(R)
        want_pair = s <= 16
        assert (int(R[g]), bool(pair[g])) == (tile_of(m, want_pair), want_pair), (m, s)
        assert lds[g] == 2 * 4 * ((R[g] + 3) // 4) * 64 * 16
        seen_tiles.add(int(R[g]))
    assert seen_tiles == set(TILES)
    assert of[M.index(6141)] >= 0 and all(of[i] == -1 for i, m in enumerate(M) if m == 6142)
    # every row (3) and every second row (4) whatever the loss; the int16 flavours 6 and 7 likewise
    for opt, want in ((3, 0), (6, 0), (4, 1), (7, 1)):
        options("ssv_kernel", opt)
        of, R, pair, lds, _ = batch_plan(M, slack)
        assert set(pair.tolist()) == {want} and all((g >= 0) == (m <= 6141) for m, g in zip(M, of))
    options("ssv_kernel", -1)
    # forced parts: whatever has two nodes for each part goes through the chain
    options("ssv_parts", 2)
    of, R, pair, lds, _ = batch_plan([1, 2, 3, 4, 5, 100, 1203, 6141], [9] * 8)
    assert (of >= 0).tolist() == [True, True, True, False, False, False, False, False]
    options("ssv_parts", 0)
    assert (batch_plan([1, 2, 3, 4, 5, 100, 1203, 6141], [9] * 8)[0] >= 0).all()


# ------------------------------------------------------------------------------------------------ API errors, no device
def test_api_errors_need_no_device(libp7x):
    dna, amino = easel.Alphabet.dna(), easel.Alphabet.amino()
    bmyd = load_hmms("bmyD")[0]
    seq = _read(BGC, dna)[0]
    pli = plan7.LongTargetsPipeline(dna)
    protein_seq = easel.DigitalSequence(amino, name="p", sequence=np.arange(20, dtype=np.uint8))
    with pytest.raises(errors.AlphabetMismatch):
        pli.scan_seq(protein_seq, [bmyd])
    with pytest.raises(errors.AlphabetMismatch):
        pli.scan_seq(seq, [bmyd, load_hmms("PF02826")[0]])
    with pytest.raises(errors.AlphabetMismatch):
        next(iter(hmmer.nhmmscan([seq], [load_hmms("PF02826")[0]])))
    with pytest.raises(TypeError):
        pli.scan_seq("ACGT", [bmyd])
    # a Profile / OptimizedProfile that carries no window length
    bare = load_hmms("bmyD")[0]
    bare.max_length = None
    om = plan7.OptimizedProfile(bare, plan7.Background(dna), 400)
    assert (getattr(om, "max_length", None) or -1) <= 0
    with pytest.raises(TypeError, match="max_length"):
        pli.scan_seq(seq, [bmyd, om])
    # ... unless window_length overrides every model's: then only the device is missing
    if _lib.lib().p7x_device_count() < 1:
        with pytest.raises(errors.DeviceUnavailable):
            plan7.LongTargetsPipeline(dna, window_length=2000).scan_seq(seq, [om])
        with pytest.raises(errors.DeviceUnavailable):
            next(iter(hmmer.nhmmscan(seq, [bmyd])))
    # a model beyond the device kernels, by name
    limit = _lib.lib().p7x_max_model_length()
    giant = random_hmm(limit + 1, seed=3, alphabet=dna)
    giant.name = "giant"
    giant.max_length = 4 * limit
    with pytest.raises(ValueError, match="giant.*model too long"):
        pli.scan_seq(seq, [bmyd, giant])
    # an empty library and an empty query list, as hmmscan: a list without hits; nothing
    assert list(hmmer.nhmmscan([], [bmyd])) == []
    empty = list(hmmer.nhmmscan([seq], []))
    assert len(empty) == 1 and len(empty[0]) == 0 and empty[0].mode == "scan" and empty[0].long_targets and empty[0].query is seq
    with pytest.raises(ValueError):
        next(iter(hmmer.nhmmscan([seq], [bmyd], batch=0)))
