"""GPU tests of nhmmscan: the batched long-target SSV scan (ssvlong_multi_kernel, a model per blockIdx.y) against the
single-model scan and the oracle's sequential p7_SSVFilter_longtarget, and hmmer.nhmmscan / LongTargetsPipeline.scan_seq
end to end against hmmer.nhmmer of every model of the library alone."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import host_pipeline
from conftest import GOLDEN, golden_table, load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, hmmer, plan7
from test_host_nhmmscan import BGC, CONTIG, TILES, _cut_model, _read, check_scan_table, check_written_rows, fields, tile_of

pytestmark = pytest.mark.gpu

DNA = easel.Alphabet.dna()


@pytest.fixture
def option():
    yield _lib.set_debug_option
    for name in ("ssv_kernel", "ssv_parts", "ssv_scan_chunk"):
        _lib.set_debug_option(name, -1)


def batch_stats(reset=False):
    out = (C.c_int64 * 8)()
    assert _lib.lib().p7x_debug_ssv_batch_stats(out, int(reset)) == 0
    return [int(v) for v in out]


def single_seeds(om, cfg, residues, complement, cap=1 << 16):
    seeds = np.zeros((cap, 3), dtype=np.int64)
    d = np.ascontiguousarray(residues, dtype=np.uint8)
    n = _lib.lib().p7x_ssv_longtarget_seeds(C.byref(cfg), om._handle, 0, d.ctypes.data, len(d), int(complement), seeds.ctypes.data, cap)
    assert 0 <= n <= cap, _lib.last_error()
    return seeds[:n].tolist()


def batch_seeds(oms, cfg, residues, complement, cap=1 << 18):
    """p7x_ssv_longtarget_seeds_batch: the seeds of every model of the batch, a list per model."""
    seeds = np.zeros((cap, 3), dtype=np.int64)
    count = np.zeros(len(oms), dtype=np.int64)
    d = np.ascontiguousarray(residues, dtype=np.uint8)
    arr = (C.c_void_p * len(oms))(*[om._handle for om in oms])
    n = _lib.lib().p7x_ssv_longtarget_seeds_batch(C.byref(cfg), arr, len(oms), 0, d.ctypes.data, len(d), int(complement), seeds.ctypes.data, cap,
                                                  count.ctypes.data)
    assert 0 <= n <= cap and n == int(count.sum()), _lib.last_error()
    ends = np.cumsum(count)
    return [seeds[int(e - c):int(e)].tolist() for c, e in zip(count, ends)]


class Library:
    """The models of the seeds tests with their references, computed once per (target, strand) and shared."""

    def __init__(self, oracle, hmms):
        self.oracle = oracle
        self.pli = plan7.LongTargetsPipeline(DNA, block_length=1 << 30)
        self.hmms = hmms
        self.oms = [plan7.OptimizedProfile(h, self.pli.background, 400) for h in hmms]
        self.ops = [oracle.OracleProfile(h, self.pli.background, 400) for h in hmms]
        self._single, self._oracle = {}, {}

    def single(self, key, seq, strand):
        # the options stay as the test set them: the single-model scan has no chunk option, and its seeds are the same with
        # every kernel flavour (tests/test_gpu_longtarget.py)
        if (key, strand) not in self._single:
            self._single[(key, strand)] = [single_seeds(om, self.pli._cfg(), seq, strand) for om in self.oms]
        return self._single[(key, strand)]

    def sequential(self, key, seq, strand):
        if (key, strand) not in self._oracle:
            blk = np.ascontiguousarray(seq if strand == 0 else host_pipeline.DNA_COMP[seq[::-1]])
            with ThreadPoolExecutor(max_workers=8) as pool:          # the oracle's scan releases the interpreter
                self._oracle[(key, strand)] = list(pool.map(
                    lambda hp: self.oracle.ssv_longtarget(hp[1], blk, hp[0].max_length, self.pli.F1).tolist(), zip(self.hmms, self.ops)))
        return self._oracle[(key, strand)]


@pytest.fixture(scope="module")
def bgc():
    return np.asarray(_read(BGC, DNA)[0].sequence, dtype=np.uint8)


@pytest.fixture(scope="module")
def tiles_library(oracle):
    """A Dirichlet-sampled model (60-110 units lost per row: the maximum in every row) at the smallest and the largest M of
    every register tile, and on the other side of the PAIR decision the fixtures (9-12 units) and slices of bmyD up to the
    largest paired M of several tiles; a model of one node."""
    full = load_hmms("bmyD")[0]
    hmms = [full, load_hmms("RF00001")[0], random_hmm(1, seed=9001, alphabet=DNA)]
    prev = 0
    for r in TILES:
        lo, hi = max(2, 128 * prev - 1), 128 * r - 2               # need = (M + 1) // 2 + 1 registers of 64 r
        assert tile_of(lo, False) == r == tile_of(hi, False) and (prev == 0 or tile_of(lo - 1, False) == prev) and (r == TILES[-1] or tile_of(hi + 1, False) > r)
        hi = min(hi, 6141)                                          # 6,142 nodes go through the chained parts, whatever their rows
        hmms += [random_hmm(lo, seed=9000 + lo, alphabet=DNA), random_hmm(hi, seed=9000 + hi, alphabet=DNA)]
        prev = r
    for r in (2, 3, 4, 5, 8, 9):                                    # paired: the virtual node M + 1 is the tile's last cell
        hi = 128 * r - 3
        assert tile_of(hi, True) == r and tile_of(hi + 1, True) > r
        hmms.append(_cut_model(full, 20, 20 + hi, f"bmyD_{hi}"))
    return Library(oracle, hmms)


def check_batched(lib, key, seq, strands=(0, 1), sequential=True):
    got_any = 0
    for strand in strands:
        got = batch_seeds(lib.oms, lib.pli._cfg(), seq, strand)
        want = lib.single(key, seq, strand)
        for h, g, w in zip(lib.hmms, got, want):
            assert g == w, (key, strand, h.name, h.M)
        if sequential:
            for h, g, w in zip(lib.hmms, got, lib.sequential(key, seq, strand)):
                assert g == w, (key, strand, h.name, h.M, "oracle")
        got_any += sum(len(g) for g in got)
    return got_any


def test_plan_of_the_tiles_library(tiles_library):
    """The library holds both row flavours at once and every tile; everything in it is batched."""
    slack = []
    for om in tiles_library.oms:
        s = C.c_int32()
        assert _lib.lib().p7x_debug_ssv_tables(om._handle, 0, None, C.byref(s), None, 0) > 0
        slack.append(s.value)
    from test_host_nhmmscan import batch_plan
    of, R, pair, lds, limit = batch_plan([h.M for h in tiles_library.hmms], slack)
    assert (of >= 0).all() and set(R.tolist()) == set(TILES) and set(pair.tolist()) == {0, 1}
    assert min(slack) <= 12 and max(slack) >= 60


@pytest.mark.parametrize("chunk", [64, -1], ids=["chunks of 64", "the library's chunks"])
def test_batched_seeds_on_the_cluster(tiles_library, bgc, option, chunk):
    """BGC0001090 whole, both strands: batched == single-model == the oracle's sequential scan, for every model; with chunks of
    64 rows the 44,660 rows of a strand cross 697 chunk boundaries, and every model is longer than its chunks' warm-up."""
    before = batch_stats()
    option("ssv_scan_chunk", chunk)
    assert check_batched(tiles_library, "bgc", bgc) > 100
    after = batch_stats()
    assert after[3] - before[3] == 2 * len(tiles_library.oms) and after[4] == before[4] and after[2] - before[2] >= 2 * 18


@pytest.mark.parametrize("variant", [5, 3, 4])
def test_batched_seeds_with_every_kernel_flavour(tiles_library, bgc, option, variant):
    """int16 cells (5), the maximum in every row (3) and in every second row whatever the model loses per row (4)."""
    option("ssv_kernel", variant)
    option("ssv_scan_chunk", 192)
    got = [batch_seeds(tiles_library.oms, tiles_library.pli._cfg(), bgc, strand) for strand in (0, 1)]
    option("ssv_kernel", -1)
    for strand in (0, 1):
        for h, g, w in zip(tiles_library.hmms, got[strand], tiles_library.sequential("bgc", bgc, strand)):
            assert g == w, (variant, strand, h.name, h.M)


def test_batched_seeds_on_short_targets(tiles_library, bgc, option):
    """700 residues (shorter than bmyD and most of the library), one residue, and two short records laid end to end with
    the sentinel between them inside a chunk: every diagonal ends there."""
    assert check_batched(tiles_library, "bgc700", bgc[:700]) > 0
    check_batched(tiles_library, "one", bgc[:1])
    two = np.concatenate([bgc[1000:1900], np.array([255], dtype=np.uint8), bgc[30000:31100]])
    for chunk in (-1, 128):
        option("ssv_scan_chunk", chunk)
        # the oracle scans one record at a time: the single-model scan is the reference across the sentinel ...
        assert check_batched(tiles_library, "two", two, sequential=False) > 0
    # ... and per record the seeds of the model of one node are the sequential scan's, shifted
    m1 = next(i for i, h in enumerate(tiles_library.hmms) if h.M == 1)
    got = batch_seeds(tiles_library.oms, tiles_library.pli._cfg(), two, 0)[m1]
    want = [s for s in tiles_library.sequential("two_a", two[:900], 0)[m1]] + \
           [[s[0] + 901, s[1], s[2]] for s in tiles_library.sequential("two_b", two[901:], 0)[m1]]
    assert got == want and len(got) > 10


def test_model_beyond_one_launch_joins_the_batch(oracle, bgc, option):
    """M = 6,142 next to short models: it goes through the chained parts of the single-model scan, the others through the
    batched launch, and every model's seeds are the single-model scan's."""
    hmms = [random_hmm(6142, seed=15142, alphabet=DNA), _cut_model(load_hmms("bmyD")[0], 300, 700, "bmyD_400"), random_hmm(60, seed=9060, alphabet=DNA)]
    lib = Library(oracle, hmms)
    before = batch_stats()
    check_batched(lib, "bgc", bgc, sequential=False)
    after = batch_stats()
    assert after[4] - before[4] == 2 and after[3] - before[3] == 4          # per strand: one model falls back, two are batched


def test_record_buffer_too_small_at_first(oracle, option):
    """200 copies of a 60-node model's consensus in 20 kb: more rows reach the threshold than the first record buffer holds;
    the scan is repeated with room for all of them and the seeds are the single-model scan's."""
    hmm = random_hmm(60, seed=9060, alphabet=DNA)
    rng = np.random.default_rng(60)
    seq = rng.integers(0, 4, size=20_000).astype(np.uint8)
    cons = np.argmax(hmm.match_emissions[1:], axis=1).astype(np.uint8)
    for c in range(200):
        seq[100 * c + 10:100 * c + 70] = cons
    lib = Library(oracle, [hmm, random_hmm(130, seed=9130, alphabet=DNA)])
    before = batch_stats()
    n = check_batched(lib, "planted", seq, strands=(0,))
    after = batch_stats()
    assert n >= 200 and after[5] - before[5] == 1, (n, before, after)


# ------------------------------------------------------------------------------------------------ end to end
def image(h):
    return fields(h) + (h.reported, h.included)


def alone(model, seq, **options):
    """hmmer.nhmmer of one model against one sequence (digitised in the model's own alphabet: DNA and RNA share their codes)."""
    s = easel.DigitalSequence(model.alphabet, name=seq.name, accession=seq.accession, description=seq.description, sequence=np.asarray(seq.sequence))
    return next(hmmer.nhmmer(model, easel.DigitalSequenceBlock(model.alphabet, [s]), **options))


def check_scan_against_lone_searches(scan, library, seq, **options):
    n = len(library)
    assert scan.mode == "scan" and scan.long_targets and scan.query is seq and scan.searched_models == n
    total = 0
    for m in library:
        want = alone(m, seq, **options)
        mine = [h for h in scan if h.name == m.name]
        assert len(mine) == len(want), m.name
        assert sorted(map(fields, mine)) == sorted(map(fields, want)), m.name
        by = {fields(h): h for h in want}
        for h in mine:
            assert h.evalue == pytest.approx(by[fields(h)].evalue * n, rel=1e-6)
            assert (h.accession, h.description) == (m.accession, m.description)
        total += len(mine)
    assert total == len(scan) and scan.is_sorted()
    return total


@pytest.fixture(scope="module")
def e2e_library():
    full = load_hmms("bmyD")[0]
    return [full, load_hmms("RF00001")[0], _cut_model(full, 850, 1193, "bmyD_tail"), _cut_model(full, 100, 300, "bmyD_200"),
            _cut_model(full, 400, 440, "bmyD_40")]


def test_nhmmscan_equals_nhmmer_of_every_model(e2e_library):
    """The tail is nhmmer's own code over the same seeds: every coordinate, strand, score, bias and alignment string of
    every model's hits equal its lone search's, the E-values times the number of models; twice the same list."""
    seq = _read(BGC, DNA)[0]
    scan = next(hmmer.nhmmscan([seq], e2e_library))
    assert check_scan_against_lone_searches(scan, e2e_library, seq) >= 3
    check_written_rows(scan)
    again = next(hmmer.nhmmscan([seq], e2e_library))
    assert [(h.name, h.evalue) + image(h) for h in again] == [(h.name, h.evalue) + image(h) for h in scan]
    # batches of two models: the same list
    split = next(hmmer.nhmmscan([seq], e2e_library, batch=2))
    assert [(h.name, h.evalue) + image(h) for h in split] == [(h.name, h.evalue) + image(h) for h in scan]
    # a library of one: nhmmer's table with the roles exchanged
    check_scan_table(next(hmmer.nhmmscan(seq, e2e_library[:1])), golden_table("bmyD1.tbl"))


def test_nhmmscan_on_the_contig(e2e_library):
    """391 kb: two blocks, hits on both strands (bmyD's own three are all on the reverse strand, bmyD2.tbl; the slices of it
    find copies on the forward strand too)."""
    seq = _read(CONTIG, DNA)[0]
    library = e2e_library
    scan = next(hmmer.nhmmscan([seq], library))
    assert check_scan_against_lone_searches(scan, library, seq) >= 3
    assert {h.domains[0].strand for h in scan} == {"+", "-"} and scan.searched_residues == 2 * len(seq)


def test_several_queries_share_the_library(e2e_library):
    whole = _read(BGC, DNA)[0]
    contig = _read(CONTIG, DNA)[0]
    b = easel.DigitalSequence(DNA, name="contig_part", sequence=np.asarray(contig.sequence)[180_000:190_000])
    c = easel.DigitalSequence(DNA, name="short", sequence=np.asarray(whole.sequence)[:100])       # shorter than every model
    library = e2e_library[:4]
    assert len(c) < min(m.M for m in library)
    seen = []
    before = batch_stats()
    together = list(hmmer.nhmmscan([whole, b, c], library, batch=3, callback=lambda q, n: seen.append((q.name, n))))
    after = batch_stats()
    assert after[0] - before[0] == 2 and after[1] - before[1] == 6            # two batches: their tables once, six scans
    assert seen == [(whole.name, 3), (b.name, 3), (c.name, 3)] and [h.query for h in together] == [whole, b, c]
    for q, hits in zip((whole, b, c), together):
        own = next(hmmer.nhmmscan(q, library))
        assert [(h.name, h.evalue) + image(h) for h in hits] == [(h.name, h.evalue) + image(h) for h in own], q.name
        assert hits.searched_models == len(library)
    assert len(together[0]) >= 2 and len(together[1]) >= 1 and len(together[2]) == 0
    # from a block and from a file
    block = easel.DigitalSequenceBlock(DNA, [whole, b])
    assert [len(h) for h in hmmer.nhmmscan(block, library)] == [len(together[0]), len(together[1])]
    with easel.SequenceFile(GOLDEN / "seqs" / BGC, digital=True, alphabet=DNA) as f:
        from_file = list(hmmer.nhmmscan(f, library))
    assert len(from_file) == 1 and [image(h) for h in from_file[0]] == [image(h) for h in together[0]]
    # an empty library and an empty query list, as hmmscan
    assert list(hmmer.nhmmscan([], library)) == []
    empty = list(hmmer.nhmmscan([whole], []))
    assert len(empty) == 1 and len(empty[0]) == 0 and empty[0].mode == "scan"
    # a query without residues: nothing is scanned, the list is empty and counts the library like the others
    nothing = easel.DigitalSequence(DNA, name="nothing", sequence=np.zeros(0, dtype=np.uint8))
    got = list(hmmer.nhmmscan([nothing, c], library, batch=3))
    assert [len(h) for h in got] == [0, 0] and [h.searched_models for h in got] == [len(library)] * 2


def test_scan_seq_and_serialisation(e2e_library):
    import pickle
    seq = _read(BGC, DNA)[0]
    library = e2e_library[:4]
    ref = next(hmmer.nhmmscan(seq, library))
    hits = plan7.LongTargetsPipeline(DNA).scan_seq(seq, library)
    assert [(h.name, h.evalue) + image(h) for h in hits] == [(h.name, h.evalue) + image(h) for h in ref] and len(hits) >= 2
    from_block = plan7.LongTargetsPipeline(DNA).scan_seq(seq, plan7.OptimizedProfileBlock(DNA, [lib_om for lib_om in hits._library[0].profiles[:1]]))
    assert [fields(h) for h in from_block] == [fields(h) for h in hits if h.name == library[0].name]
    for strand, sign in (("watson", "+"), ("crick", "-")):
        one = plan7.LongTargetsPipeline(DNA, strand=strand).scan_seq(seq, library)
        assert one.strand == strand and one.searched_residues == len(seq) and {h.domains[0].strand for h in one} == {sign}
        check_scan_against_lone_searches(one, library, seq, strand=strand)
    wide = plan7.LongTargetsPipeline(DNA, window_length=2000).scan_seq(seq, library)
    check_scan_against_lone_searches(wide, library, seq, window_length=2000)
    for back in (plan7.TopHits.from_bytes(hits.to_bytes(), query=seq), pickle.loads(pickle.dumps(hits))):
        assert [(h.name, h.evalue) + image(h) for h in back] == [(h.name, h.evalue) + image(h) for h in hits]
        assert back.mode == "scan" and back.long_targets and back.searched_models == len(library)
    check_written_rows(hits)
