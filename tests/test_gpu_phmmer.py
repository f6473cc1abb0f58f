"""phmmer end to end on the device: hmmer.phmmer and Pipeline.search_seq against HMMER's own `phmmer --domtblout` of the last
sequence of PKSI.faa against that file (the reference's test_hmmer.py:464-493), batches of queries, and the error paths."""
import itertools
import math

import numpy as np
import pytest

from conftest import GOLDEN, golden_table
from pyhmmer_amd import easel, errors, hmmer, plan7

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pksi(libp7x):
    abc = easel.Alphabet.amino()
    with easel.SequenceFile(GOLDEN / "seqs" / "PKSI.faa", digital=True, alphabet=abc) as sf:
        return sf.read_block()


def flat(hits):
    return [(h.name, round(h.score, 4), round(h.bias, 4), h.evalue,
             [(d.score, d.i_evalue, d.c_evalue, d.env_from, d.env_to, d.alignment.hmm_from, d.alignment.hmm_to,
               d.alignment.target_from, d.alignment.target_to) for d in h.domains]) for h in hits]


@pytest.fixture(scope="module")
def last_query_hits(pksi):
    return next(hmmer.phmmer(pksi[-1:], pksi, cpus=1))


def test_pksi_reproduces_the_phmmer_table(last_query_hits, pksi):
    """Every field the reference test checks, at its tolerances, and |ln E - ln E(table)| <= 0.06 for the non-zero E-values
    (two printed digits: ln 1.05 = 0.049 plus formatting slack)."""
    assert last_query_hits.query is pksi[len(pksi) - 1]
    hits = last_query_hits.copy()                 # the fixture is shared: sort a copy
    hits.sort()
    rows = golden_table("A0A089QRB9.domtbl", kind="domtbl")
    pairs = [(hit, dom) for hit in hits for dom in hit.domains]
    for r, pair in itertools.zip_longest(rows, pairs):
        assert r is not None and pair is not None
        hit, dom = pair
        assert hit.name == r[0]
        assert abs(hit.score - float(r[7])) <= 0.1 and abs(hit.bias - float(r[8])) <= 0.1 and abs(hit.evalue - float(r[6])) <= 0.1
        assert abs(dom.i_evalue - float(r[12])) <= 0.1 and abs(dom.score - float(r[13])) <= 0.1
        a = dom.alignment
        assert (a.hmm_from, a.hmm_to, a.target_from, a.target_to, dom.env_from, dom.env_to) == tuple(int(v) for v in r[15:21])
        for got, want in ((hit.evalue, float(r[6])), (dom.c_evalue, float(r[11])), (dom.i_evalue, float(r[12]))):
            if want > 0:
                assert got > 0 and abs(math.log(got) - math.log(want)) <= 0.06, (r[0], r[9], got, want)


def test_search_seq_gives_the_same_hits(last_query_hits, pksi):
    hits = plan7.Pipeline(pksi.alphabet).search_seq(pksi[len(pksi) - 1], pksi)
    assert hits.query is pksi[len(pksi) - 1]
    assert flat(hits) == flat(last_query_hits)
    hmm, profile, om = plan7.Builder(pksi.alphabet).build(pksi[len(pksi) - 1], plan7.Background(pksi.alphabet))
    assert hmm.M == profile.M == om.M == 2085 and hmm.evalue_parameters == om.evalue_parameters
    assert hmm.evalue_parameters.f_tau is not None
    assert flat(plan7.Pipeline(pksi.alphabet).search_hmm(hmm, pksi)) == flat(last_query_hits)


def test_five_queries_in_one_call_equal_five_calls(pksi, last_query_hits):
    """Batch calibration plus batched search: hit for hit what the queries give one by one; the callback sees every query."""
    seen = []
    together = list(hmmer.phmmer(pksi[-5:], pksi, callback=lambda q, total: seen.append((q.name, total))))
    assert len(together) == 5 and seen == [(s.name, 5) for s in pksi[-5:]]
    for q, hits in zip(pksi[-5:], together):
        assert hits.query is q
        alone = next(hmmer.phmmer([q], pksi))
        assert flat(hits) == flat(alone), q.name
    assert flat(together[-1]) == flat(last_query_hits)


def test_error_paths(pksi):
    abc = pksi.alphabet
    assert next(hmmer.phmmer([], pksi, cpus=1), None) is None
    dna = easel.Alphabet.dna()
    dseq = easel.DigitalSequence(dna, name="d", sequence=np.array([0, 1, 2, 3] * 10, np.uint8))
    with pytest.raises(errors.AlphabetMismatch):
        next(hmmer.phmmer([dseq], pksi))
    with pytest.raises(errors.AlphabetMismatch):
        plan7.Pipeline(abc).search_seq(dseq, pksi)
    with pytest.raises(errors.AlphabetMismatch):
        plan7.Pipeline(abc).search_seq(pksi[0], easel.DigitalSequenceBlock(dna, [dseq]))
    with pytest.raises(TypeError):
        plan7.Pipeline(abc).search_seq(plan7.HMM(abc, 3, "x"), pksi)
    with pytest.raises(TypeError):
        plan7.Pipeline(abc).search_seq(pksi[0], [pksi[1]])
    with pytest.raises(TypeError):
        next(hmmer.phmmer(["MKV"], pksi))
    with pytest.raises(TypeError):
        next(hmmer.phmmer(pksi[-1:], "targets"))

    class Oops(Exception):
        pass

    def callback(query, total):
        raise Oops("oopsie")

    with pytest.raises(Oops):
        next(hmmer.phmmer(pksi[-1:], pksi, cpus=1, callback=callback))
