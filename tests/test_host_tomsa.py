"""TopHits.to_msa on the host: the alignment of the included domains of a search (upstream p7_tophits_Alignment, what
`hmmsearch -A` writes), built from the hit list alone -- every alignment display converted back to a trace
(p7_alidisplay_Backconvert; `Trace.from_alignment`), the traces aligned by p7_tracealign_Seqs (tests/test_host_align.py).

The hits come from the CPU seam of the search (tests/host_pipeline.py: the oracle's filters and parsers, the product's
host stage).  The recorded answer is the reference's tests/golden/msa/KR-1.sto: `KR.hmm` against the proteome with
incE = incdomE = 0.001, written by HMMER 3.3.2.  The file holds two Stockholm records; the first one, six rows, is the
alignment of that search (the reference's own test reads only the first as well) and is what "the fixture" means here."""
import ctypes as C
import io
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import host_pipeline
from conftest import GOLDEN
from pyhmmer_amd import _lib, easel, errors, plan7

INCLUDED, REPORTED = 1, 2            # P7X_IS_INCLUDED, P7X_IS_REPORTED
S, N, B, E, CC, T, M, D, I = 4, 5, 6, 7, 8, 9, 1, 2, 3      # p7T_*


# ------------------------------------------------------------------------------------------------ helpers (shared with the GPU tests)
def stockholm(msa) -> str:
    buf = io.BytesIO()
    msa.write(buf, "stockholm")
    return buf.getvalue().decode()


def parse_stockholm(text: str):
    """The records of a Stockholm text: for each, the #=GF lines, {(name, tag): text} of #=GS, the rows in order of first
    appearance {name: aligned text}, {name: PP text} of #=GR ... PP, {tag: text} of #=GC; blocks are joined."""
    records, rec = [], None
    for line in text.splitlines():
        if line.startswith("# STOCKHOLM"):
            rec = SimpleNamespace(gf=[], gs={}, rows={}, gr={}, gc={})
            continue
        if rec is None or not line.strip():
            continue
        if line == "//":
            records.append(rec)
            rec = None
        elif line.startswith("#=GF "):
            rec.gf.append(line)
        elif line.startswith("#=GS "):
            _, name, tag, value = line.split(None, 3)
            rec.gs[(name, tag)] = value
        elif line.startswith("#=GR "):
            _, name, tag, value = line.split()
            assert tag == "PP", line
            rec.gr[name] = rec.gr.get(name, "") + value
        elif line.startswith("#=GC "):
            _, tag, value = line.split()
            rec.gc[tag] = rec.gc.get(tag, "") + value
        else:
            assert not line.startswith("#"), line
            name, value = line.split()
            rec.rows[name] = rec.rows.get(name, "") + value
    assert rec is None, "unterminated Stockholm record"
    return records


def fixture_text() -> str:
    """The first record of the fixture, as text."""
    text = (GOLDEN / "msa" / "KR-1.sto").read_text()
    return text[:text.index("//\n") + 3]


def without_gf(text: str) -> str:
    return "".join(line for line in text.splitlines(keepends=True) if not line.startswith("#=GF "))


def assert_equals_fixture(msa):
    """Identity with HMMER's recorded alignment: the parsed content -- row names in order, every row, every PP line, RF and
    PP_cons, every #=GS line -- and then the bytes.  The only line class left out of the byte comparison is `#=GF`: the
    fixture's two (`ID KR-i1`, `AU hmmsearch (HMMER 3.3.2)`) are what the program that wrote it says about its own run (the
    model it searched with was named KR-i1), ours is `ID KR`, the name of tests/golden/hmms/KR.hmm."""
    text = stockholm(msa)
    ours, = parse_stockholm(text)
    want, = parse_stockholm(fixture_text())
    assert list(ours.rows) == list(want.rows)
    assert tuple(ours.rows) == msa.names
    for name in want.rows:
        assert ours.rows[name] == want.rows[name], name
        assert ours.gr[name] == want.gr[name], name
    assert set(ours.gr) == set(want.gr)
    assert ours.gc == want.gc and set(want.gc) == {"RF", "PP_cons"}
    assert ours.gs == want.gs and {tag for _, tag in want.gs} == {"DE"}
    assert ours.gf == ["#=GF ID KR"]
    assert without_gf(text) == without_gf(fixture_text())


def handmade_hits(qname, alphabet, M_, hits):
    """A hit list of hand-written displays (test seam p7x_debug_tophits_from_displays).  hits: (name, accession, description,
    flags, [domain dict: model, aseq, pp, hmm (from, to), sq (from, to), L, included])."""
    nh = len(hits)
    arr = lambda xs: (C.c_char_p * max(nh, 1))(*[x.encode() if x else None for x in xs])
    doms = [d for h in hits for d in h[4]]
    recs = (_lib.DomainRec * max(len(doms), 1))()
    for r, d in zip(recs, doms):
        r.model, r.aseq, r.ppline = d["model"].encode(), d["aseq"].encode(), d["pp"].encode() if d.get("pp") else None
        r.hmmfrom, r.hmmto = d["hmm"]
        r.sqfrom, r.sqto = d["sq"]
        r.L, r.is_included, r.is_reported = d["L"], int(d.get("included", True)), 1
    flags = (C.c_uint32 * max(nh, 1))(*[h[3] for h in hits])
    ndom = (C.c_int32 * max(nh, 1))(*[len(h[4]) for h in hits])
    out = C.c_void_p()
    st = _lib.lib().p7x_debug_tophits_from_displays(qname.encode(), alphabet.type_code, M_, nh, arr(h[0] for h in hits),
                                                    arr(h[1] for h in hits), arr(h[2] for h in hits), flags, ndom, recs, C.byref(out))
    assert st == 0, _lib.last_error()
    return plan7.TopHits(qname, out)


# three displays against a model of five nodes, worked out by hand below
DOM_A = dict(model="acdef", aseq="ACDEF", pp="98765", hmm=(1, 5), sq=(1, 5), L=5)          # starts at residue 1, ends at L: no flanks
DOM_B = dict(model="a.cd", aseq="AgCD", pp="9876", hmm=(1, 3), sq=(2, 5), L=6)             # an insert right after the first match
DOM_C = dict(model="acde", aseq="AC-E", pp="98.7", hmm=(2, 5), sq=(1, 3), L=3)             # a delete before the last match


def as_alignment(d, M_=5):
    return SimpleNamespace(hmm_sequence=d["model"], target_sequence=d["aseq"], posterior_probabilities=d.get("pp"),
                           hmm_from=d["hmm"][0], hmm_to=d["hmm"][1], hmm_length=M_, target_from=d["sq"][0], target_to=d["sq"][1],
                           target_length=d["L"])


@pytest.fixture(scope="module")
def amino(libp7x):
    return easel.Alphabet.amino()


@pytest.fixture(scope="module")
def kr_hits(models, oracle, proteome):
    hmm = models["KR"][0]
    return host_pipeline.host_search(oracle, hmm, proteome, pipeline=plan7.Pipeline(hmm.alphabet, incE=1e-3, incdomE=1e-3))


# ------------------------------------------------------------------------------------------------ back-conversion
@pytest.mark.parametrize("name", ["KR", "PF02826"])
def test_backconversion_round_trip(models, oracle, proteome, name):
    """Every domain of the host-pipeline hits: display -> trace of the whole target -> display again, rendered by the code
    that made the first one (make_alidisplay through the seam p7x_debug_tophits_from_trace).  Model, match, sequence and
    posterior lines and all coordinates come back as they were (a PP digit d decodes to d / 10, the middle of the values
    [d / 10 - 0.05, d / 10 + 0.05) that print as d, and so encodes to d again)."""
    hmm = models[name][0]
    hits = host_pipeline.host_search(oracle, hmm, proteome)
    om = hits._keep[0]
    ndom = 0
    for hit in hits:
        seq = proteome[hit.seqidx]
        assert seq.name == hit.name
        dsq1 = np.concatenate([[255], seq.sequence, [255]]).astype(np.uint8)
        for dom in hit.domains:
            a = dom.alignment
            tr = plan7.Trace.from_alignment(a)
            assert (tr.M, tr.L) == (hmm.M, len(seq)) and len(tr.st) == len(a) + 6 + (a.target_from - 1) + (len(seq) - a.target_to)
            assert list(tr.st[:2]) == [S, N] and list(tr.st[-2:]) == [CC, T]
            emitted = tr.i[np.isin(tr.st, (M, I)) | (((tr.st == N) | (tr.st == CC)) & (tr.i > 0))]
            assert np.array_equal(emitted, np.arange(1, len(seq) + 1))                    # every residue exactly once, in order
            flank = ((tr.st == N) | (tr.st == CC)) & (tr.i > 0)
            assert np.all(tr.posterior_probabilities[flank] == 1.0)
            assert np.all(tr.posterior_probabilities[~flank & ~np.isin(tr.st, (M, I))] == 0.0)
            out = C.c_void_p()
            st = _lib.lib().p7x_debug_tophits_from_trace(om._handle, dsq1.ctypes.data, len(seq), len(tr.st), tr.st.ctypes.data,
                                                         tr.k.ctypes.data, tr.i.ctypes.data, tr.posterior_probabilities.ctypes.data,
                                                         hit.name.encode(), C.byref(out))
            assert st == 0, _lib.last_error()
            b = plan7.TopHits(hmm, out)[0].domains[0].alignment
            for attr in ("hmm_sequence", "identity_sequence", "target_sequence", "posterior_probabilities", "hmm_from", "hmm_to",
                         "hmm_length", "target_from", "target_to", "target_length", "hmm_name", "target_name"):
                assert getattr(a, attr) == getattr(b, attr), (hit.name, attr)
            # upstream's own form: the subsequence alone
            sub = plan7.Trace.from_alignment(a, whole=False)
            assert len(sub.st) == len(a) + 6 and list(sub.st[:3]) == [S, N, B] and list(sub.st[-3:]) == [E, CC, T]
            assert sub.L == a.target_to - a.target_from + 1 and sub.M == hmm.M
            core = slice(3, 3 + len(a))
            assert np.array_equal(sub.st[core], tr.st[np.isin(tr.st, (M, D, I))]) and np.array_equal(sub.k[core], tr.k[np.isin(tr.st, (M, D, I))])
            assert np.array_equal(sub.i[core][sub.st[core] != D], np.arange(1, sub.L + 1))
            ndom += 1
    assert ndom >= 10


def test_backconversion_of_handmade_displays(amino):
    pp = lambda *digits: [np.float32(d / 10.0) for d in digits]
    # no flanks: the trace of the whole target is upstream's trace of the subsequence
    for whole in (True, False):
        tr = plan7.Trace.from_alignment(as_alignment(DOM_A), amino, whole=whole)
        assert list(tr.st) == [S, N, B, M, M, M, M, M, E, CC, T] and (tr.M, tr.L) == (5, 5)
        assert list(tr.k) == [0, 0, 0, 1, 2, 3, 4, 5, 0, 0, 0] and list(tr.i) == [0, 0, 0, 1, 2, 3, 4, 5, 0, 0, 0]
        assert list(tr.posterior_probabilities) == [0, 0, 0] + pp(9, 8, 7, 6, 5) + [0, 0, 0]
    # an insert right after the first match; one flank residue on either side
    tr = plan7.Trace.from_alignment(as_alignment(DOM_B), amino)
    assert list(tr.st) == [S, N, N, B, M, I, M, M, E, CC, CC, T] and (tr.M, tr.L) == (5, 6)
    assert list(tr.k) == [0, 0, 0, 0, 1, 1, 2, 3, 0, 0, 0, 0] and list(tr.i) == [0, 0, 1, 0, 2, 3, 4, 5, 0, 0, 6, 0]
    assert list(tr.posterior_probabilities) == [0, 0, 1, 0] + pp(9, 8, 7, 6) + [0, 0, 1, 0]
    sub = plan7.Trace.from_alignment(as_alignment(DOM_B), amino, whole=False)
    assert list(sub.st) == [S, N, B, M, I, M, M, E, CC, T] and list(sub.i) == [0, 0, 0, 1, 2, 3, 4, 0, 0, 0] and sub.L == 4
    # a delete before the last match: no residue, no posterior
    tr = plan7.Trace.from_alignment(as_alignment(DOM_C), amino)
    assert list(tr.st) == [S, N, B, M, M, D, M, E, CC, T] and list(tr.k) == [0, 0, 0, 2, 3, 4, 5, 0, 0, 0]
    assert list(tr.i) == [0, 0, 0, 1, 2, 0, 3, 0, 0, 0]
    assert list(tr.posterior_probabilities) == [0, 0, 0] + pp(9, 8) + [0] + pp(7) + [0, 0, 0]
    # '*' is 1.0; without a PP line the trace has no posteriors
    star = plan7.Trace.from_alignment(as_alignment(dict(DOM_A, pp="*9*9*")), amino)
    assert list(star.posterior_probabilities[3:8]) == [1.0] + pp(9) + [1.0] + pp(9) + [1.0]
    assert plan7.Trace.from_alignment(as_alignment(dict(DOM_A, pp=None)), amino).posterior_probabilities is None
    # what is not a display is refused
    for bad in (dict(DOM_A, hmm=(1, 4)), dict(DOM_A, sq=(1, 4)), dict(DOM_A, aseq="ACDE"), dict(DOM_A, aseq="AC1EF"),
                dict(DOM_A, pp="9876x"), dict(DOM_A, sq=(2, 6)), dict(DOM_B, aseq="A-CD", sq=(2, 4))):
        with pytest.raises(ValueError):
            plan7.Trace.from_alignment(as_alignment(bad), amino)
    with pytest.raises(ValueError, match="alphabet"):
        plan7.Trace.from_alignment(as_alignment(DOM_A))


# ------------------------------------------------------------------------------------------------ to_msa on hand-made hit lists
def test_to_msa_of_handmade_displays(amino):
    """Three hits of one domain each.  Columns: node 1, the insert after it (DOM_B's g), nodes 2..5.  DOM_B ends at node 3
    (nodes 4, 5: '-'), DOM_C starts at node 2 and deletes node 4.  PP_cons is the mean over the rows with a residue in a
    match column: node 1 (.9 + .9) / 2, node 2 (.8 + .7 + .9) / 3, node 3 (.7 + .6 + .8) / 3, node 4 .6, node 5 (.5 + .7) / 2."""
    hits = handmade_hits("q5", amino, 5, [("t1", "ACC1", "first target", INCLUDED | REPORTED, [DOM_A]),
                                          ("t2", None, None, INCLUDED | REPORTED, [DOM_B]),
                                          ("t3", None, "third", INCLUDED | REPORTED, [DOM_C])])
    assert hits.alphabet == amino
    msa = hits.to_msa(amino)
    assert isinstance(msa, easel.TextMSA) and msa.name == "q5"
    assert msa.names == ("t1/1-5", "t2/2-5", "t3/1-3")
    assert msa.alignment == ("A.CDEF", "AgCD--", "-.AC-E")
    assert msa.posterior_probabilities == ["9.8765", "9876..", "..98.7"]
    assert msa.reference == "x.xxxx" and msa.pp_consensus == "9.8766" and msa.secondary_structure is None
    assert [s.description for s in msa.sequences] == ["[subseq from] first target", "[subseq from] t2", "[subseq from] third"]
    assert [s.accession for s in msa.sequences] == ["ACC1", "", ""]
    assert stockholm(msa) == ("# STOCKHOLM 1.0\n#=GF ID q5\n\n"
                              "#=GS t1/1-5 AC ACC1\n#=GS t1/1-5 DE [subseq from] first target\n#=GS t2/2-5 DE [subseq from] t2\n"
                              "#=GS t3/1-3 DE [subseq from] third\n\n"
                              "t1/1-5         A.CDEF\n#=GR t1/1-5 PP 9.8765\nt2/2-5         AgCD--\n#=GR t2/2-5 PP 9876..\n"
                              "t3/1-3         -.AC-E\n#=GR t3/1-3 PP ..98.7\n#=GC PP_cons   9.8766\n#=GC RF        x.xxxx\n//\n")
    # without DOM_A only the nodes somebody uses get a column, unless all are asked for
    two = handmade_hits("q5", amino, 5, [("t2", None, None, INCLUDED, [DOM_B]), ("t3", None, None, INCLUDED, [DOM_C])])
    assert two.to_msa(amino).reference == "x.xxx" and two.to_msa(amino).alignment == ("AgCD-", "-.ACE")
    assert two.to_msa(amino, all_consensus_cols=True).alignment == ("AgCD--", "-.AC-E")


def test_to_msa_takes_included_domains_of_included_hits(amino):
    second = dict(DOM_B, sq=(12, 15), L=20)
    hits = handmade_hits("q5", amino, 5, [
        ("multi", None, None, INCLUDED | REPORTED, [DOM_A, dict(DOM_C, sq=(7, 9), L=20, included=False), second]),
        ("reported_only", None, None, REPORTED, [DOM_A]),               # an included domain of a hit that is not included
        ("last", None, None, INCLUDED | REPORTED, [DOM_C])])
    msa = hits.to_msa(amino)
    assert msa.names == ("multi/1-5", "multi/12-15", "last/1-3")
    assert msa.alignment == ("A.CDEF", "AgCD--", "-.AC-E")
    hits[2].included = False                                            # the flags are read at the time of the call
    assert hits.to_msa(amino).names == ("multi/1-5", "multi/12-15")


def test_to_msa_extra_sequences_trim_and_digitize(amino):
    """`sequences` / `traces` come first.  The extra one is GG ACDEF GG with the trace of the whole sequence, so it has two
    flank residues on either side: they get columns of their own unless the alignment is trimmed."""
    hits = handmade_hits("q5", amino, 5, [("t1", None, None, INCLUDED, [DOM_A])])
    extra = easel.TextSequence(name="extra", description="brought along", sequence="GGACDEFGG").digitize(amino)
    trace = plan7.Trace.from_alignment(as_alignment(dict(DOM_A, sq=(3, 7), L=9)), amino)
    full = hits.to_msa(amino, sequences=[extra], traces=[trace])
    assert full.names == ("extra", "t1/1-5")
    assert full.alignment == ("ggACDEFgg", "..ACDEF..") and full.reference == "..xxxxx.."
    assert full.posterior_probabilities == ["**98765**", "..98765.."] and full.pp_consensus == "..98765.."
    assert [s.description for s in full.sequences] == ["brought along", "[subseq from] t1"]
    trimmed = hits.to_msa(amino, sequences=[extra], traces=[trace], trim=True)
    assert trimmed.alignment == ("ACDEF", "ACDEF") and trimmed.reference == "xxxxx" and trimmed.names == full.names
    assert len(full) >= len(hits.to_msa(amino)) == 5
    # only extras: still an alignment (upstream fails only when there is nothing at all)
    none = handmade_hits("q5", amino, 5, [])
    assert none.to_msa(amino, sequences=[extra], traces=[trace], trim=True).alignment == ("ACDEF",)
    # digital round trip
    digital = hits.to_msa(amino, sequences=[extra], traces=[trace], digitize=True)
    assert isinstance(digital, easel.DigitalMSA) and digital.alphabet == amino and digital.name == "q5"
    assert digital.textize() == full and full.digitize(amino) == digital
    gap = amino.K
    assert [list(s.sequence) for s in digital.sequences] == [list(amino.encode("GGACDEFGG")), [gap, gap] + list(amino.encode("ACDEF")) + [gap, gap]]


def test_to_msa_nucleotide_and_reverse_strand(libp7x):
    """Long-target lists take the same path; a reverse-strand domain has sqfrom > sqto and its subsequence is the display's
    own text (already the reverse complement), as upstream takes it."""
    dna = easel.Alphabet.dna()
    fwd = dict(model="acgu", aseq="ACGT", pp="9999", hmm=(1, 4), sq=(7, 10), L=50)
    rev = dict(model="ac.gu", aseq="ACtGT", pp="99899", hmm=(1, 4), sq=(31, 27), L=50)
    hits = handmade_hits("nuc", dna, 4, [("chr", None, None, INCLUDED, [fwd]), ("chr", None, None, INCLUDED, [rev])])
    msa = hits.to_msa(dna)
    assert msa.names == ("chr/7-10", "chr/31-27") and msa.alignment == ("AC.GT", "ACtGT")
    with pytest.raises(ValueError, match="sqfrom <= sqto"):
        plan7.Trace.from_alignment(as_alignment(rev, 4), dna)
    assert list(plan7.Trace.from_alignment(as_alignment(rev, 4), dna, whole=False).st) == [S, N, B, M, M, I, M, M, E, CC, T]


def test_to_msa_errors(amino):
    hits = handmade_hits("q5", amino, 5, [("t1", None, None, INCLUDED, [DOM_A])])
    with pytest.raises(errors.AlphabetMismatch):
        hits.to_msa(easel.Alphabet.dna())
    extra = easel.TextSequence(name="extra", sequence="ACDEF").digitize(amino)
    with pytest.raises(ValueError, match="same length"):
        hits.to_msa(amino, sequences=[extra], traces=[])
    with pytest.raises(ValueError, match="same length"):
        hits.to_msa(amino, traces=[plan7.Trace.from_sequence(extra)])
    with pytest.raises(errors.AlphabetMismatch):
        hits.to_msa(amino, sequences=[easel.TextSequence(name="n", sequence="ACGT").digitize(easel.Alphabet.dna())],
                    traces=[plan7.Trace.from_sequence(extra)])
    for nothing in (handmade_hits("q5", amino, 5, []),
                    handmade_hits("q5", amino, 5, [("t1", None, None, REPORTED, [DOM_A])]),
                    handmade_hits("q5", amino, 5, [("t1", None, None, INCLUDED, [dict(DOM_A, included=False)])])):
        with pytest.raises(ValueError, match="No included domains"):
            nothing.to_msa(amino)
    with pytest.raises(ValueError):                                       # a trace of another model
        hits.to_msa(amino, sequences=[extra], traces=[plan7.Trace.from_sequence(easel.TextSequence(sequence="ACD").digitize(amino))])


# ------------------------------------------------------------------------------------------------ identity with HMMER
def test_included_set_is_the_fixtures(kr_hits):
    """The premise of the identity test: at incE = incdomE = 0.001 the included domains are exactly the fixture's rows."""
    want, = parse_stockholm(fixture_text())
    ours = [f"{h.name}/{d.alignment.target_from}-{d.alignment.target_to}" for h in kr_hits if h.included for d in h.domains if d.included]
    assert ours == list(want.rows) and len(ours) == 6
    assert any(h.included and len(h.domains.included) < len(h.domains) for h in kr_hits)      # ... and not simply all domains


def test_to_msa_reproduces_hmmer(kr_hits, amino):
    msa = kr_hits.to_msa(amino, all_consensus_cols=True)         # hmmsearch -A passes p7_ALL_CONSENSUS_COLS (hmmsearch.c)
    assert isinstance(msa, easel.TextMSA) and msa.name == "KR" and len(msa.sequences) == 6
    assert_equals_fixture(msa)
    assert msa.reference.count("x") == 262
    # by default only the nodes some row uses get a column; the rows hold the same residues
    default = kr_hits.to_msa(amino)
    assert default.names == msa.names and len(default) == len(msa) - (262 - default.reference.count("x")) < len(msa)
    strip = lambda row: row.replace("-", "").replace(".", "")
    assert [strip(r) for r in default.alignment] == [strip(r) for r in msa.alignment]
    # the reference's own checks (test_tophits.py::test_to_msa)
    assert len({s.name.split("/")[0] for s in msa.sequences}) == len(kr_hits.included)
    digital = kr_hits.to_msa(amino, trim=True, digitize=True, all_consensus_cols=True)
    assert isinstance(digital, easel.DigitalMSA) and len(digital) >= 262 and digital.names == msa.names
    assert len({s.name.split("/")[0] for s in digital.sequences}) == len(kr_hits.included)


def test_to_msa_survives_serialisation_and_merge(models, oracle, proteome, kr_hits, amino):
    want = stockholm(kr_hits.to_msa(amino))
    back = plan7.TopHits.from_bytes(kr_hits.to_bytes())
    assert back.query is None and back.alphabet == amino
    assert stockholm(back.to_msa(amino)) == want
    assert stockholm(pickle.loads(pickle.dumps(kr_hits)).to_msa(amino)) == want
    assert stockholm(kr_hits.copy().to_msa(amino)) == want
    with pytest.raises(errors.AlphabetMismatch):
        back.to_msa(easel.Alphabet.rna())
    # two halves of the proteome with Z fixed to the whole, so that inclusion does not move
    hmm = models["KR"][0]
    pli = lambda: plan7.Pipeline(hmm.alphabet, incE=1e-3, incdomE=1e-3, Z=len(proteome))
    half = len(proteome) // 2
    parts = [host_pipeline.host_search(oracle, hmm, proteome[a:b], pipeline=pli()) for a, b in ((0, half), (half, len(proteome)))]
    merged = parts[0].merge(parts[1])
    assert stockholm(merged.to_msa(amino)) == want
    assert stockholm(plan7.TopHits.from_bytes(merged.to_bytes()).to_msa(amino)) == want
