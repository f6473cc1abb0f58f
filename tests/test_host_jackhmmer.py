"""jackhmmer without a device: `easel.KeyHash`, `TopHits.compare_ranking`, the loop of `plan7.IterativeSearch`
(`Pipeline.iterate_seq` / `iterate_hmm`) with its two device steps replaced by their CPU seams (tests/jackhmmer_cases.py), the
argument checks of `Pipeline.search_msa` / `iterate_*` / `hmmer.jackhmmer`, and the code matrix an alignment keeps.

The recorded rounds are the reference's (test_pipeline.py:267-328): P12748 of LuxC.faa and KR.hmm against the fixture
proteome with incE = incdomE = 0.001, written by HMMER 3.3.2.

What this project's builder reproduces of them, and what it does not:

* P12748: every round has the fixture's number of columns, rows, its name and its TARGETS, and the search has converged after
  round 3.  Round 1 also has the fixture's row names.  From round 2 on one row is named `...HG003689_22/134-316` where the
  fixture has `/134-317` (round 3: `/133-318` for `/133-319`, `HG003690_243/95-282` for `/95-281`): the alignment of that domain
  (E = 3.0e-14, far from 0.001) ends one residue earlier.  The residue the fixture adds carries the posterior digit 5 --
  optimal accuracy weighs it as a match against the same residue left to the C state, a near tie that the model of round 2,
  the first one `Builder.build_msa` makes here, decides the other way.  The rows are otherwise the fixture's, column by column.
* KR.hmm: rounds 1 and 2 have the fixture's columns, rows and name (270 x 6, 273 x 11).  Round 3 includes two targets that the
  fixture includes one round later: `HG003686_375` with E = 3.8e-4 and `HG003687_15` with E = 8.3e-4 against the threshold
  0.001, giving 281 x 15 where the fixture has 275 x 13; from there the runs part, and this one has not converged after round 7
  (the fixture's after round 6).

So the rounds before the first that differs are asserted in full, and of the later ones what is listed above."""
import itertools

import numpy as np
import pytest

import jackhmmer_cases as jc
from conftest import GOLDEN, synthetic_block
from pyhmmer_amd import easel, errors, hmmer, plan7
from test_host_tomsa import DOM_A, DOM_B, DOM_C, handmade_hits

INCLUDED, REPORTED, NEW, DROPPED = 1, 2, 4, 8          # P7X_IS_*


@pytest.fixture(scope="module")
def amino(libp7x):
    return easel.Alphabet.amino()


# ------------------------------------------------------------------------------------------------ KeyHash
def test_keyhash_surface():
    kh = easel.KeyHash()
    assert len(kh) == 0 and list(kh) == [] and "a" not in kh
    assert kh.add("first") == 0 and kh.add("second") == 1 and kh.add("first") == 0        # a key again: its index, no new entry
    assert len(kh) == 2 and list(kh) == ["first", "second"]
    assert "first" in kh and "third" not in kh and 3 not in kh
    assert kh["second"] == 1
    with pytest.raises(KeyError):
        kh["third"]
    with pytest.raises(TypeError):
        kh.add(3)
    other = kh.copy()
    assert other == kh and other is not kh
    other.add("third")
    assert len(kh) == 2 and len(other) == 3 and other != kh
    kh.clear()
    assert len(kh) == 0 and "first" not in kh and kh.add("second") == 0


# ------------------------------------------------------------------------------------------------ compare_ranking
def hits_of(amino, *flagged):
    """One hit of one domain per (name, flags)."""
    doms = itertools.cycle([DOM_A, DOM_B, DOM_C])
    return handmade_hits("q5", amino, 5, [(name, None, None, flags, [next(doms)]) for name, flags in flagged])


def flags_of(hits):
    return [(h.name, h.included, h.new, h.dropped) for h in hits]


def test_compare_ranking_new_kept_dropped(amino):
    hits = hits_of(amino, ("t1", INCLUDED | REPORTED), ("t2", INCLUDED | REPORTED), ("t3", REPORTED), ("t4", REPORTED))
    ranking = easel.KeyHash()
    for name in ("t3", "t1", "gone"):                 # the round before included t3, t1 and a target this round does not report
        ranking.add(name)
    assert hits.compare_ranking(ranking) == 1
    assert flags_of(hits) == [("t1", True, False, False),          # kept: included before and now
                              ("t2", True, True, False),           # new
                              ("t3", False, False, True),          # dropped: included before, not now
                              ("t4", False, False, False)]         # never included
    assert list(ranking) == ["t1", "t2"] and ranking["t2"] == 1    # refilled with the included hits, in list order
    # the flags are part of the list: they travel with its image, and a second comparison finds nothing new
    back = plan7.TopHits.from_bytes(hits.to_bytes())
    assert flags_of(back) == flags_of(hits)
    assert [h._rec.flags for h in back] == [INCLUDED | REPORTED, INCLUDED | REPORTED | NEW, REPORTED | DROPPED, REPORTED]
    assert back.compare_ranking(ranking) == 0 and list(ranking) == ["t1", "t2"]
    with pytest.raises(TypeError):
        hits.compare_ranking({"t1": 0})


def test_compare_ranking_empty_ranking_and_duplicate_names(amino):
    hits = hits_of(amino, ("t1", INCLUDED | REPORTED), ("t2", REPORTED), ("t1", INCLUDED | REPORTED))
    ranking = easel.KeyHash()
    assert hits.compare_ranking(ranking) == 2          # an empty ranking: every included hit is new, nothing is dropped
    assert flags_of(hits) == [("t1", True, True, False), ("t2", False, False, False), ("t1", True, True, False)]
    assert list(ranking) == ["t1"]                     # the same name twice is one key, not an error
    # the walk follows the list's current order
    hits = hits_of(amino, ("b", INCLUDED | REPORTED), ("a", INCLUDED | REPORTED))
    assert hits.compare_ranking(ranking) == 2 and list(ranking) == [h.name for h in hits]
    empty = handmade_hits("q5", amino, 5, [])
    assert empty.compare_ranking(ranking) == 0 and len(ranking) == 0


# ------------------------------------------------------------------------------------------------ the recorded rounds
@pytest.fixture(scope="module")
def p12748_rounds(oracle, proteome):
    search = jc.host_iterate(oracle, jc.p12748(), proteome)
    rounds = []
    for n in range(jc.P12748_ROUNDS):
        assert search.iteration == n and not search.converged
        rounds.append(next(search))
        assert search.iteration == n + 1 == rounds[-1].iteration
    return search, rounds


def test_p12748_rounds(p12748_rounds):
    search, rounds = p12748_rounds
    for n, result in enumerate(rounds, 1):
        hmm, hits, msa, converged, iteration = result                   # unpacks like the reference's
        assert isinstance(hmm, plan7.HMM) and isinstance(hits, plan7.TopHits) and isinstance(msa, easel.DigitalMSA)
        columns, rows, name, names = jc.recorded("p12748", n)
        assert (len(msa), len(msa.sequences), msa.name) == (columns, rows, name)
        assert {nm.split("/")[0] for nm in msa.names} == {nm.split("/")[0] for nm in names}
        assert msa.names[0] == search.query.name and msa.author and msa.description == search.query.description
        assert converged == (n == 3) and iteration == n
        jc.assert_codes_kept(msa)
    assert set(rounds[0].msa.names) == set(jc.recorded("p12748", 1)[3])         # round 2: see the module's docstring
    assert search.converged and search.msa is rounds[-1].msa and list(search.ranking) == [h.name for h in rounds[-1].hits.included]
    with pytest.raises(StopIteration):
        next(search)
    assert search.iteration == 3
    # round 1 searches with the query's own model, the later ones with models of the alignments
    assert [r.hmm.M for r in rounds] == [len(search.query)] * 3 and [r.hmm.nseq for r in rounds] == [1, 2, 3]
    assert [r.hmm.name for r in rounds] == [search.query.name, search.query.name + "-i1", search.query.name + "-i2"]
    assert [[h.new for h in r.hits.included] for r in rounds] == [[True], [False, True], [False, False]]


def test_kr_rounds(oracle, proteome, models):
    search = jc.host_iterate(oracle, models["KR"][0], proteome)
    for n in (1, 2):                                                              # round 3: see the module's docstring
        result = next(search)
        columns, rows, name, _ = jc.recorded("KR", n)
        assert (len(result.msa), len(result.msa.sequences), result.msa.name) == (columns, rows, name)
        assert result.iteration == n and not result.converged
        jc.assert_codes_kept(result.msa)
    assert result.hmm.name == "KR-i1" and search.msa is result.msa


# ------------------------------------------------------------------------------------------------ the loop's corners
def test_select_hits_changes_the_next_alignment(oracle, proteome, p12748_rounds):
    seen = []

    def drop_all(hits):
        assert hits.is_sorted(by="key")
        for hit in hits:
            seen.append(hit.name)
            hit.dropped = True

    search = jc.host_iterate(oracle, jc.p12748(), proteome, select_hits=drop_all)
    result = next(search)
    assert seen == [h.name for h in p12748_rounds[1][0].hits]
    assert len(p12748_rounds[1][0].msa.names) == 2 and list(result.msa.names) == [search.query.name]
    assert result.converged and len(search.ranking) == 0 and not any(h.included for h in result.hits)


def test_sequence_query_without_hits_converges_at_once(oracle):
    targets = synthetic_block(40, 120, seed=7)
    query = synthetic_block(1, 90, seed=11)[0]
    query.name = "lonely"
    search = jc.host_iterate(oracle, query, targets)
    result = next(search)
    assert len(result.hits.included) == 0 and result.converged and result.iteration == 1
    assert list(result.msa.names) == ["lonely"] and len(result.msa) == 90 and result.msa.name == "lonely-i1"
    with pytest.raises(StopIteration):
        next(search)


def test_hmm_query_without_included_hits_is_an_error(oracle, models):
    search = jc.host_iterate(oracle, models["KR"][0], synthetic_block(40, 120, seed=7))
    with pytest.raises(ValueError, match="No included domains found"):
        next(search)


def test_one_round_is_not_convergence(p12748_rounds):
    first = p12748_rounds[1][0]
    assert first.iteration == 1 and not first.converged and [h.new for h in first.hits.included] == [True]


# ------------------------------------------------------------------------------------------------ argument checks
def test_iterate_checks(amino, proteome, models):
    pipeline = plan7.Pipeline(amino, seed=7)
    query = jc.p12748()
    search = pipeline.iterate_seq(query, proteome)
    assert isinstance(search, plan7.IterativeSearch) and iter(search) is search
    assert (search.pipeline, search.query, search.targets) == (pipeline, query, proteome)
    assert (search.converged, search.msa, search.iteration, len(search.ranking)) == (False, None, 0, 0)
    assert search.builder.architecture == "hand" and search.builder.seed == 7
    assert pipeline.iterate_hmm(models["KR"][0], proteome).query is models["KR"][0]
    hand = plan7.Builder(amino, architecture="hand")
    assert pipeline.iterate_seq(query, proteome, hand).builder is hand
    for method, q in ((pipeline.iterate_seq, query), (pipeline.iterate_hmm, models["KR"][0])):
        with pytest.raises(ValueError, match="only supports a builder with 'hand' architecture"):
            method(q, proteome, plan7.Builder(amino))                   # the default architecture is "fast"
        with pytest.raises(errors.AlphabetMismatch):
            method(q, easel.DigitalSequenceBlock(easel.Alphabet.dna(), []))
    dna = easel.Alphabet.dna()
    with pytest.raises(errors.AlphabetMismatch):
        pipeline.iterate_seq(easel.DigitalSequence(dna, name="n", sequence=np.zeros(8, np.uint8)), proteome)
    with pytest.raises(errors.AlphabetMismatch):
        plan7.Pipeline(dna).iterate_hmm(models["KR"][0], proteome)
    with pytest.raises(TypeError):
        pipeline.iterate_seq(models["KR"][0], proteome)
    with pytest.raises(TypeError):
        pipeline.iterate_hmm(query, proteome)


def test_search_msa_checks(amino, proteome):
    with easel.MSAFile(GOLDEN / "msa" / "LuxC.sto", digital=True, alphabet=amino) as f:
        msa = f.read()
    with pytest.raises(errors.AlphabetMismatch):
        plan7.Pipeline(easel.Alphabet.dna()).search_msa(msa, proteome)
    with pytest.raises(TypeError):
        plan7.Pipeline(amino).search_msa(msa.textize(), proteome)


def test_long_targets_refuse_alignments_and_rounds(models):
    dna = easel.Alphabet.dna()
    pipeline = plan7.LongTargetsPipeline(dna)
    block = easel.DigitalSequenceBlock(dna, [])
    for call in (lambda: pipeline.search_msa(None, block), lambda: pipeline.iterate_seq(None, block), lambda: pipeline.iterate_hmm(None, block)):
        with pytest.raises(NotImplementedError, match="no DNA builder"):
            call()


def test_jackhmmer_checks(amino, proteome):
    assert next(hmmer.jackhmmer([], proteome, max_iterations=1), None) is None          # no queries: nothing, and no device asked for
    assert hmmer.jackhmmer_rounds() == []
    with pytest.raises(TypeError, match="Unsupported query type"):
        next(hmmer.jackhmmer(3, proteome))
    with pytest.raises(ValueError, match="backend"):
        next(hmmer.jackhmmer([], proteome, backend="fork"))
    with easel.SequenceFile(GOLDEN / "seqs" / "LuxC.faa") as text_file:
        with pytest.raises(ValueError, match="digital"):
            next(hmmer.jackhmmer([], text_file))


# ------------------------------------------------------------------------------------------------ the code matrix
def test_alignment_keeps_its_code_matrix(amino, p12748_rounds):
    msa = p12748_rounds[1][1].msa
    jc.assert_codes_kept(msa)
    assert not msa._codes().flags.writeable
    # a subset is another alignment: it starts without a matrix and encodes its own rows
    part = msa.select(sequences=[0, 2], columns=range(100, 300))
    assert getattr(part, "_code_matrix", None) is None
    assert np.array_equal(part._codes(), msa._codes()[[0, 2], 100:300])
    # rows replaced behind the alignment's back: the matrix is dropped, not handed out
    changed = msa.select()
    changed._keep_codes(changed._encode_rows())
    changed._rows[1] = changed._rows[0]
    assert np.array_equal(changed._codes()[1], changed._codes()[0]) and changed._code_matrix is None
    # text alignments and alignments made without the flag have none; the seam turns it off
    hits = handmade_hits("q5", amino, 5, [("t1", None, None, INCLUDED | REPORTED, [DOM_A]), ("t2", None, None, INCLUDED | REPORTED, [DOM_B])])
    assert getattr(hits.to_msa(amino), "_code_matrix", None) is None
    kept = hits.to_msa(amino, digitize=True)
    jc.assert_codes_kept(kept)
    assert kept._codes().tolist() == [[0, 20, 1, 2, 3, 4], [0, 5, 1, 2, 20, 20]]         # A.CDEF / AgCD--
    from pyhmmer_amd import _lib
    _lib.set_debug_option("msa_codes", 0)
    try:
        plain = hits.to_msa(amino, digitize=True)
    finally:
        _lib.set_debug_option("msa_codes", -1)
    assert getattr(plain, "_code_matrix", None) is None and np.array_equal(plain._codes(), kept._codes())
