"""TopHits.to_msa of device searches (`hmmer.hmmsearch`, library defaults): the alignment of the included domains, held to
HMMER's recorded alignment (tests/golden/msa/KR-1.sto, see tests/test_host_tomsa.py) and to the host twin of the search
(tests/host_pipeline.py: the oracle's filters and parsers, the product's host stage), string for string.  No DP runs in
to_msa itself: what is checked is that the alignment displays the device search leaves are the ones HMMER's would be."""
import pytest

import host_pipeline
from pyhmmer_amd import easel, hmmer, plan7
from test_host_tomsa import assert_equals_fixture, stockholm

pytestmark = pytest.mark.gpu

INC = dict(incE=1e-3, incdomE=1e-3)          # the thresholds the fixture was made with


@pytest.fixture(scope="module")
def amino(libp7x):
    return easel.Alphabet.amino()


@pytest.fixture(scope="module")
def kr_device(models, proteome):
    hits, = hmmer.hmmsearch(models["KR"][0], proteome, **INC)
    return hits


def test_kr_alignment_equals_hmmer_and_the_host_twin(models, oracle, proteome, kr_device, amino):
    msa = kr_device.to_msa(amino, all_consensus_cols=True)       # hmmsearch -A passes p7_ALL_CONSENSUS_COLS
    assert isinstance(msa, easel.TextMSA) and msa.name == "KR"
    assert_equals_fixture(msa)
    hmm = models["KR"][0]
    twin = host_pipeline.host_search(oracle, hmm, proteome, pipeline=plan7.Pipeline(hmm.alphabet, **INC))
    for flags in (dict(all_consensus_cols=True), dict(), dict(trim=True, digitize=True)):
        assert stockholm(kr_device.to_msa(amino, **flags)) == stockholm(twin.to_msa(amino, **flags)), flags


def test_pf02826_alignment_equals_the_host_twin(models, oracle, proteome, amino):
    hmm = models["PF02826"][0]
    hits, = hmmer.hmmsearch(hmm, proteome)
    twin = host_pipeline.host_search(oracle, hmm, proteome)
    msa = hits.to_msa(amino)
    assert stockholm(msa) == stockholm(twin.to_msa(amino))
    nincluded = sum(1 for h in hits if h.included for d in h.domains if d.included)
    assert len(msa.sequences) == nincluded > 1
    assert msa.names == tuple(f"{h.name}/{d.alignment.target_from}-{d.alignment.target_to}"
                              for h in hits if h.included for d in h.domains if d.included)


def test_alignment_after_serialisation_and_merge(models, proteome, kr_device, amino):
    want = stockholm(kr_device.to_msa(amino))
    back = plan7.TopHits.from_bytes(kr_device.to_bytes())
    assert back.query is None and stockholm(back.to_msa(amino)) == want
    # two halves of the proteome, Z fixed to the whole so that inclusion does not move
    hmm = models["KR"][0]
    half = len(proteome) // 2
    parts = [list(hmmer.hmmsearch(hmm, proteome[a:b], Z=len(proteome), **INC))[0] for a, b in ((0, half), (half, len(proteome)))]
    merged = parts[0].merge(parts[1])
    assert stockholm(merged.to_msa(amino)) == want
    assert stockholm(plan7.TopHits.from_bytes(merged.to_bytes()).to_msa(amino)) == want


def test_extra_sequences_and_traces_come_first(models, proteome, kr_device, amino):
    hmm = models["KR"][0]
    extras = [proteome[kr_device[r].seqidx] for r in range(2)]
    traces = plan7.TraceAligner().compute_traces(hmm, easel.DigitalSequenceBlock(amino, extras))
    plain = kr_device.to_msa(amino)
    msa = kr_device.to_msa(amino, sequences=extras, traces=list(traces))
    assert msa.names == tuple(s.name for s in extras) + plain.names
    assert len(msa) >= len(plain)
    strip = lambda row: row.replace("-", "").replace(".", "").upper()
    assert [strip(r) for r in msa.alignment[:2]] == [amino.decode(s.sequence) for s in extras]       # whole sequences, flanks included
    assert [strip(r) for r in msa.alignment[2:]] == [strip(r) for r in plain.alignment]
    trimmed = kr_device.to_msa(amino, sequences=extras, traces=list(traces), trim=True)
    assert trimmed.names == msa.names and len(trimmed) <= len(msa)
