"""hmmalign on the host: TraceAligner / hmmer.hmmalign through the host twin (test seam "host_align" = 1: upstream's
Forward / Backward / decoding / optimal accuracy in upstream's summation order), the MSA built from the traces
(p7_tracealign_Seqs) and Easel's Stockholm text, pinned byte for byte by the reference's recorded
`hmmalign --trim LuxC.hmm LuxC.faa` (tests/golden/msa/LuxC.hmmalign.sto).  Trace / Traces semantics follow the
reference's test_traces.py and test_tracealigner.py."""
import io

import numpy as np
import pytest

from conftest import GOLDEN
from pyhmmer_amd import _lib, easel, errors, hmmer, plan7


@pytest.fixture
def host_align(libp7x):
    _lib.set_debug_option("host_align", 1)
    yield
    _lib.set_debug_option("host_align", -1)


@pytest.fixture(scope="module")
def luxc(libp7x):
    with plan7.HMMFile(GOLDEN / "hmms" / "LuxC.hmm") as f:
        hmm = f.read()
    with easel.SequenceFile(GOLDEN / "seqs" / "LuxC.faa", digital=True, alphabet=hmm.alphabet) as sf:
        seqs = sf.read_block()
    return hmm, seqs


def _stockholm(msa) -> bytes:
    buf = io.BytesIO()
    msa.write(buf, "stockholm")
    return buf.getvalue()


def test_hmmalign_trim_reproduces_hmmer_byte_for_byte(luxc, host_align):
    hmm, seqs = luxc
    msa = hmmer.hmmalign(hmm, seqs, trim=True)
    assert isinstance(msa, easel.TextMSA)
    assert _stockholm(msa) == (GOLDEN / "msa" / "LuxC.hmmalign.sto").read_bytes()


def test_hmmalign_text_stream(luxc, host_align):
    hmm, seqs = luxc
    msa = hmmer.hmmalign(hmm, list(seqs), trim=True)           # any iterable of sequences, as the reference
    out = io.StringIO()
    msa.write(out, "stockholm")
    assert out.getvalue() == (GOLDEN / "msa" / "LuxC.hmmalign.sto").read_text()


@pytest.mark.parametrize("trim,alen", [(False, 567), (True, 429)])
def test_align_traces_columns(luxc, host_align, trim, alen):
    hmm, seqs = luxc
    aligner = plan7.TraceAligner()
    traces = aligner.compute_traces(hmm, seqs)
    assert len(traces) == len(seqs)
    msa = aligner.align_traces(hmm, seqs, traces, all_consensus_cols=True, trim=trim)
    assert len(msa.sequences) == len(seqs) and len(msa) == alen
    assert msa.names == tuple(s.name for s in seqs)
    assert all(len(row) == alen for row in msa.alignment)
    # every residue of a sequence is in its row (trim drops only the flanks)
    for row, seq in zip(msa.alignment, seqs):
        residues = "".join(c for c in row if c.isalpha()).upper()
        text = seq.textize().sequence.upper()
        assert residues == text if not trim else residues in text


def test_traces_of_the_aligner(luxc, host_align):
    hmm, seqs = luxc
    traces = plan7.TraceAligner().compute_traces(hmm, seqs)
    for trace, seq in zip(traces, seqs):
        assert trace.M == hmm.M == 400
        assert trace.L == len(seq)
        pp = trace.posterior_probabilities
        assert pp is not None and pp.dtype == np.float32 and pp.shape == trace.st.shape
        assert ((pp >= 0) & (pp <= 1.0 + 1e-4)).all()       # (float posteriors: a few ulps above 1 is upstream's arithmetic)
        emitted = np.isin(trace.st, (1, 3)) | (np.isin(trace.st, (5, 8)) & (trace.i > 0))
        assert sorted(trace.i[emitted].tolist()) == list(range(1, len(seq) + 1))     # each residue exactly once
        assert 0.0 < trace.expected_accuracy() <= len(seq)
    assert traces.nflagged == 0
    assert traces == plan7.TraceAligner().compute_traces(hmm, seqs)                  # deterministic


def test_all_consensus_cols_off_drops_unused_columns(luxc, host_align):
    hmm, seqs = luxc
    aligner = plan7.TraceAligner()
    traces = aligner.compute_traces(hmm, seqs[:2])
    full = aligner.align_traces(hmm, seqs[:2], traces, all_consensus_cols=True)
    used = aligner.align_traces(hmm, seqs[:2], traces)
    assert len(used) <= len(full)
    assert used.reference.count("x") == sum(1 for k in range(1, hmm.M + 1)
                                            if any(((t.st == 1) & (t.k == k)).any() for t in traces))


def test_digitize(luxc, host_align):
    hmm, seqs = luxc
    msa = hmmer.hmmalign(hmm, seqs, trim=True, digitize=True)
    assert isinstance(msa, easel.DigitalMSA) and msa.alphabet == hmm.alphabet
    assert _stockholm(msa) == (GOLDEN / "msa" / "LuxC.hmmalign.sto").read_bytes()
    dseqs = msa.sequences
    assert len(dseqs) == len(seqs) and all(len(s) == len(msa) for s in dseqs)
    assert msa.textize() == hmmer.hmmalign(hmm, seqs, trim=True)


def test_align_traces_mismatch(luxc):
    hmm, seqs = luxc
    with pytest.raises(ValueError):
        plan7.TraceAligner().align_traces(hmm, seqs, plan7.Traces())


def test_align_traces_msa_type(luxc):
    hmm, _ = luxc
    aligner = plan7.TraceAligner()
    seqs = easel.DigitalSequenceBlock(hmm.alphabet)
    msa = aligner.align_traces(hmm, seqs, plan7.Traces())
    assert isinstance(msa, easel.TextMSA) and len(msa) == 0
    msa_d = aligner.align_traces(hmm, seqs, plan7.Traces(), digitize=True)
    assert isinstance(msa_d, easel.DigitalMSA)
    assert len(aligner.compute_traces(hmm, seqs)) == 0


def test_alphabet_mismatch(luxc):
    hmm, _ = luxc
    dna = easel.Alphabet.dna()
    block = easel.DigitalSequenceBlock(dna, [easel.TextSequence(name="s", sequence="ACGT").digitize(dna)])
    with pytest.raises(errors.AlphabetMismatch):
        plan7.TraceAligner().compute_traces(hmm, block)
    with pytest.raises(errors.AlphabetMismatch):
        plan7.TraceAligner().align_traces(hmm, block, plan7.Traces([plan7.Trace.from_sequence(block[0])]))


def test_invalid_hmm_is_refused(luxc):
    hmm, seqs = luxc
    bad = hmm.copy()
    bad.transition_probabilities[3, 0] += 0.1
    with pytest.raises(ValueError):
        plan7.TraceAligner().compute_traces(bad, seqs)


def test_empty_sequence_gets_an_empty_trace(luxc, host_align):
    hmm, seqs = luxc
    block = easel.DigitalSequenceBlock(hmm.alphabet, [seqs[0], easel.DigitalSequence(hmm.alphabet, name="empty")])
    traces = plan7.TraceAligner().compute_traces(hmm, block)
    assert len(traces[1].st) == 0 and traces[1].L == 0
    msa = plan7.TraceAligner().align_traces(hmm, block, traces, all_consensus_cols=True)
    assert set(msa.alignment[1]) <= {"-", "."}


def test_without_a_device_the_compute_call_fails(luxc, libp7x):
    """No CPU fallback: outside the test seam the traces come from the device or not at all."""
    hmm, seqs = luxc
    device = 0 if libp7x.p7x_device_count() == 0 else libp7x.p7x_device_count()     # on a GPU machine: a device that is not there
    with pytest.raises(errors.DeviceUnavailable):
        plan7.TraceAligner(device=device).compute_traces(hmm, seqs)
    with pytest.raises(errors.DeviceUnavailable):
        hmmer.hmmalign(hmm, seqs, device=device)


def test_hmmalign_is_exported():
    assert "hmmalign" in hmmer.__all__
    assert {"Trace", "Traces", "TraceAligner"} <= set(plan7.__all__)
    assert {"MSA", "TextMSA", "DigitalMSA"} <= set(easel.__all__)


def test_stockholm_writer_annotation():
    """Easel's layout: names padded to the longest, #=GS AC / DE, #=GR PP per row, #=GC lines after the rows."""
    rows = [easel.TextSequence(name="a", accession="AC1", description="first", sequence="AC-d."),
            easel.TextSequence(name="bbbb", sequence="ACGD.")]
    msa = easel.TextMSA(sequences=rows)
    msa.posterior_probabilities = ["**.9.", "9*98."]
    msa.pp_consensus, msa.reference = "**.9.", "xx.x."
    assert len(msa) == 5
    assert _stockholm(msa).decode() == (
        "# STOCKHOLM 1.0\n\n"
        "#=GS a    AC AC1\n"
        "#=GS a    DE first\n\n"
        "a            AC-d.\n"
        "#=GR a    PP **.9.\n"
        "bbbb         ACGD.\n"
        "#=GR bbbb PP 9*98.\n"
        "#=GC PP_cons **.9.\n"
        "#=GC RF      xx.x.\n"
        "//\n")


# ---- Traces container semantics (reference tests/test_plan7/test_traces.py)
def _trace(n=3):
    return plan7.Trace.from_sequence(easel.TextSequence(sequence="N" * n))


def test_trace_from_sequence():
    t = _trace(4)
    assert t.M == t.L == 4 and t.posterior_probabilities is None
    assert t.st.tolist() == [6, 1, 1, 1, 1, 7] and t.k.tolist() == [0, 1, 2, 3, 4, 0]
    assert t == _trace(4) and t != _trace(3)
    with pytest.raises(ValueError):
        t.expected_accuracy()


def test_traces_bool_len_identity():
    assert not plan7.Traces()
    assert plan7.Traces([_trace()])
    assert plan7.Traces() is not plan7.Traces()
    assert len(plan7.Traces([_trace(1), _trace(2), _trace(3)])) == 3


def test_traces_append_iter_getitem_setitem():
    t1, t2, t3 = _trace(1), _trace(2), _trace(3)
    block = plan7.Traces()
    block.append(t1)
    block.append(t2)
    assert block[0] == t1 and block[1] == t2 and block[-1] is t2 and block[-2] is t1
    it = iter(plan7.Traces([t1, t2, t3]))
    assert next(it) is t1 and next(it) is t2 and next(it) is t3
    with pytest.raises(StopIteration):
        next(it)
    with pytest.raises(IndexError):
        block[3]
    with pytest.raises(IndexError):
        block[-5]
    block[0] = t3
    assert block[0] is t3 and block[1] is t2
    block[:] = [t1, t2, t3]
    block[2:5] = [t3, t3, t3]
    assert len(block) == 5 and block[4] is t3
    assert isinstance(block[1:3], plan7.Traces)


def test_traces_clear_remove_index_pop_contains():
    t1, t2, t3 = _trace(1), _trace(2), _trace(3)
    block = plan7.Traces([t1, t2])
    block.remove(t1)
    assert len(block) == 1 and block[0] is t2
    block = plan7.Traces([t1, t2])
    assert block.index(t1) == 0 and block.index(t2) == 1
    with pytest.raises(ValueError):
        block.index(t3)
    with pytest.raises(ValueError):
        block.index(t1, start=1)
    assert t1 in block and t2 in block and t3 not in block and 42 not in block and object() not in block
    block = plan7.Traces([t1, t2, t3])
    assert block.pop() is t3 and block.pop(0) is t1 and block.pop(-1) is t2
    with pytest.raises(IndexError):
        block.pop()
    block = plan7.Traces([t1, t2])
    block.clear()
    block.clear()
    assert len(block) == 0


def test_stockholm_refuses_lines_of_another_length():
    msa = easel.TextMSA(sequences=[easel.TextSequence(name="a", sequence="ACDE")])
    for attr, value in (("reference", "x"), ("pp_consensus", "*****"), ("secondary_structure", "<<")):
        bad = easel.TextMSA(sequences=[easel.TextSequence(name="a", sequence="ACDE")])
        setattr(bad, attr, value)
        with pytest.raises(ValueError):
            _stockholm(bad)
    msa.posterior_probabilities = ["9"]
    with pytest.raises(ValueError):
        _stockholm(msa)


def test_align_traces_refuses_invalid_traces(luxc):
    """Traces are user-constructible: a match without a residue, or flank emissions the column map does not count, are
    refused instead of being placed outside the sequence or the alignment."""
    hmm, seqs = luxc
    block = seqs[:1]
    n = len(block[0])
    no_residue = plan7.Trace()
    no_residue.st = np.array([4, 5, 6, 1, 7, 8, 9], dtype=np.int8)     # S N B M1 E C T with the match on residue 0
    no_residue.k = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.int32)
    no_residue.i = np.zeros(7, dtype=np.int32)
    stray = plan7.Trace()
    stray.st = np.array([4, 6, 5, 5, 5, 7, 9], dtype=np.int8)           # S B N N N E T: N emits without following N
    stray.k = np.zeros(7, dtype=np.int32)
    stray.i = np.array([0, 0, 1, 2, 3, 0, 0], dtype=np.int32)
    for bad in (no_residue, stray):
        bad._M, bad._L = hmm.M, n
        with pytest.raises(ValueError, match="not a valid alignment"):
            plan7.TraceAligner().align_traces(hmm, block, plan7.Traces([bad]))
