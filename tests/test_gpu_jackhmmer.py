"""jackhmmer on the device: the reference's two recorded runs through `Pipeline.iterate_seq` / `iterate_hmm` (what
tests/test_host_jackhmmer.py asserts of the CPU seams, and no more: its docstring says which rounds this project's builder
reproduces), the reference's `TestJackhmmer` cases (test_hmmer.py:497-624), `hmmer.jackhmmer`'s rounds for a batch of
queries against every query's own loop, and `Pipeline.search_msa`."""
import itertools

import pytest

import jackhmmer_cases as jc
from conftest import GOLDEN, golden_table, synthetic_block
from pyhmmer_amd import easel, hmmer, plan7
from test_gpu_phmmer import flat
from test_host_tomsa import stockholm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pksi(libp7x):
    with easel.SequenceFile(GOLDEN / "seqs" / "PKSI.faa", digital=True, alphabet=easel.Alphabet.amino()) as sf:
        return sf.read_block()


def jackhmmer_pipeline(alphabet):
    return plan7.Pipeline(alphabet, incE=jc.INC, incdomE=jc.INC)


# ------------------------------------------------------------------------------------------------ the recorded rounds
def test_iterate_seq_p12748(proteome):
    search = jackhmmer_pipeline(proteome.alphabet).iterate_seq(jc.p12748(), proteome)
    for n in range(1, jc.P12748_ROUNDS + 1):
        assert search.iteration == n - 1
        result = next(search)
        assert search.iteration == n == result.iteration
        columns, rows, name, names = jc.recorded("p12748", n)
        assert (len(result.msa), len(result.msa.sequences), result.msa.name) == (columns, rows, name)
        assert {nm.split("/")[0] for nm in result.msa.names} == {nm.split("/")[0] for nm in names}
        if n == 1:                                            # round 2: tests/test_host_jackhmmer.py's docstring
            assert set(result.msa.names) == set(names)
        jc.assert_codes_kept(result.msa)
    assert result.converged and search.converged
    with pytest.raises(StopIteration):
        next(search)


def test_iterate_hmm_kr(proteome, models):
    search = jackhmmer_pipeline(proteome.alphabet).iterate_hmm(models["KR"][0], proteome)
    for n in (1, 2):                                          # round 3: tests/test_host_jackhmmer.py's docstring
        result = next(search)
        columns, rows, name, _ = jc.recorded("KR", n)
        assert (len(result.msa), len(result.msa.sequences), result.msa.name) == (columns, rows, name)
        assert result.iteration == n and not result.converged
        jc.assert_codes_kept(result.msa)


# ------------------------------------------------------------------------------------------------ the reference's TestJackhmmer
def test_pksi(pksi):
    """test_hmmer.py:543-571: one round is phmmer; `A0A089QRB9.domtbl` at that test's deltas."""
    seen = []
    result = next(hmmer.jackhmmer(pksi[-1:], pksi, cpus=1, max_iterations=1, callback=lambda q, total: seen.append((q.name, total))))
    assert result.iteration == 1 and seen == [(pksi[len(pksi) - 1].name, 1)]
    result.hits.sort()
    rows = golden_table("A0A089QRB9.domtbl", kind="domtbl")
    pairs = [(hit, dom) for hit in result.hits for dom in hit.domains]
    for r, pair in itertools.zip_longest(rows, pairs):
        assert r is not None and pair is not None
        hit, dom = pair
        assert hit.name == r[0]
        assert abs(hit.score - float(r[7])) <= 0.1 and abs(hit.bias - float(r[8])) <= 0.1 and abs(hit.evalue - float(r[6])) <= 0.1
        assert abs(dom.i_evalue - float(r[12])) <= 0.1 and abs(dom.score - float(r[13])) <= 0.1
        a = dom.alignment
        assert (a.hmm_from, a.hmm_to, a.target_from, a.target_to, dom.env_from, dom.env_to) == tuple(int(v) for v in r[15:21])


def test_pksi_checkpoint(pksi):
    """test_hmmer.py:573-587: the jackhmmer CLI converges in 3 iterations, 5 hits, 17 sequences in the alignment."""
    iterations = next(hmmer.jackhmmer(pksi[len(pksi) - 1], pksi, cpus=1, checkpoints=True))
    print([(len(r.hits), len(r.msa.sequences), r.converged) for r in iterations])
    assert len(iterations) == 3
    assert iterations[-1].converged
    assert len(iterations[-1].hits) == 5
    assert len(iterations[-1].msa.sequences) == 17
    assert [r.iteration for r in iterations] == [1, 2, 3]


def test_thioesterase(proteome, models):
    """test_hmmer.py:589-624."""
    result = next(hmmer.jackhmmer(models["Thioesterase"][0], proteome, cpus=1, max_iterations=1, incE=0.1, incdomE=0.1))
    _, hits, _, _, it = result
    assert it == 1 and len(hits) == 1
    hits.sort()
    hit = hits[0]
    assert hit.name == "938293.PRJEB85.HG003687_113"
    assert abs(hit.score - 8.6) <= 0.1 and abs(hit.bias - 1.5) <= 0.1 and abs(hit.evalue - 0.096) <= 0.01
    assert len(hit.domains) == 1
    domain = hit.domains[0]
    assert abs(domain.score - 8.1) <= 0.1 and abs(domain.bias - 1.5) <= 0.1
    assert round(domain.i_evalue - 0.14, 2) == 0 and round(domain.c_evalue - 6.5e-05, 2) == 0
    a = domain.alignment
    assert (a.target_from, a.target_to, a.hmm_from, a.hmm_to, domain.env_from, domain.env_to) == (115, 129, 79, 93, 115, 129)


def test_no_queries_and_callback_error(pksi):
    assert next(hmmer.jackhmmer([], pksi, cpus=1, max_iterations=1), None) is None

    class Oops(Exception):
        pass

    def callback(query, total):
        raise Oops("oopsie")

    for cpus in (1, 2):
        with pytest.raises(Oops):
            next(hmmer.jackhmmer(pksi[-1:], pksi, cpus=cpus, max_iterations=1, callback=callback))


# ------------------------------------------------------------------------------------------------ rounds against the single-query loop
def included(hits):
    return [(h.name, [(d.env_from, d.env_to, d.alignment.hmm_from, d.alignment.hmm_to, d.alignment.target_from, d.alignment.target_to)
                      for d in h.domains]) for h in hits.included]


def test_rounds_of_a_batch_equal_every_query_alone(proteome, models):
    """Four queries advance round by round in one `jackhmmer` call -- a sequence query that converges in round 3, another
    sequence of LuxC.faa, an HMM query that is still going when `max_iterations` = 6 stops it (the recorded run of KR.hmm
    converges in round 6, this one does not: tests/test_host_jackhmmer.py) and a sequence query without a hit, done after
    round 1 -- and each is compared with its own `iterate_seq` / `iterate_hmm`: the same number of rounds; per round the
    included names in order, the domain coordinates, the Stockholm text of the alignment, and the scores as exactly as
    test_gpu_phmmer.py::test_five_queries_in_one_call_equal_five_calls compares a batched search with a single one (`flat`:
    hit score and bias to four decimals, everything else equal)."""
    luxc = jc.luxc_queries()
    lonely = synthetic_block(1, 90, seed=11)[0]
    lonely.name = "lonely"
    queries = [jc.p12748(), next(s for s in luxc if "P12748" not in s.name), models["KR"][0], lonely]
    seen = []
    together = list(hmmer.jackhmmer(queries, proteome, checkpoints=True, max_iterations=6,
                                    callback=lambda q, total: seen.append((q.name, total))))
    assert len(together) == 4 and seen == [(q.name, 4) for q in queries]
    rounds = hmmer.jackhmmer_rounds()
    assert [r["round"] for r in rounds] == list(range(7))                 # round 0: the models of the sequence queries; one search per round
    assert [r["queries"] for r in rounds[1:]] == [sum(len(b) >= n for b in together) for n in range(1, 7)]
    for query, batched in zip(queries, together):
        pipeline = jackhmmer_pipeline(proteome.alphabet)
        search = pipeline.iterate_hmm(query, proteome) if isinstance(query, plan7.HMM) else pipeline.iterate_seq(query, proteome)
        alone = []
        for result in itertools.islice(search, 6):
            alone.append(result)
            if result.converged:
                break
        assert len(batched) == len(alone), query.name
        for b, a in zip(batched, alone):
            assert (b.iteration, b.converged) == (a.iteration, a.converged)
            assert included(b.hits) == included(a.hits), (query.name, a.iteration)
            assert stockholm(b.msa) == stockholm(a.msa), (query.name, a.iteration)
            assert flat(b.hits) == flat(a.hits), (query.name, a.iteration)
            assert b.hmm.evalue_parameters == a.hmm.evalue_parameters and b.hmm.name == a.hmm.name
            jc.assert_codes_kept(b.msa)
    assert [len(r) for r in together][0] == 3 and together[0][-1].converged
    assert len(together[2]) == 6 and len(together[3]) == 1 and together[3][0].converged
    assert list(together[3][0].msa.names) == ["lonely"]


# ------------------------------------------------------------------------------------------------ search_msa
def test_search_msa_is_build_msa_then_search_hmm(proteome):
    abc = proteome.alphabet
    with easel.MSAFile(GOLDEN / "msa" / "LuxC.sto", digital=True, alphabet=abc) as f:
        msa = f.read()
    pipeline = plan7.Pipeline(abc)
    hits = pipeline.search_msa(msa, proteome)
    assert hits.query is msa and len(hits) > 0
    hmm, _, om = plan7.Builder(abc, seed=pipeline.seed).build_msa(msa, pipeline.background)
    assert flat(hits) == flat(pipeline.search_hmm(hmm, proteome)) == flat(pipeline.search_hmm(om, proteome))
