"""Translation on the host twin (test seam ``host_translate``): the reference's recorded cases, every codon of every table
and the six-frame ORFs against the plain-Python restatement of tests/translate_cases.py, and the ten annotated CDS of
BGC0001090.gbk.  tests/test_gpu_translate.py runs the same cases on the device."""
import ctypes as C
import itertools
import pickle
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import translate_cases as tc
from conftest import GOLDEN
from pyhmmer_amd import _lib, easel
from pyhmmer_amd.errors import AlphabetMismatch, InvalidParameter

DNA, RNA, AMINO = easel.Alphabet.dna(), easel.Alphabet.rna(), easel.Alphabet.amino()
GBK = GOLDEN / "seqs" / "BGC0001090.gbk"


@pytest.fixture(autouse=True)
def host_twin(libp7x):
    _lib.set_debug_option("host_translate", 1)
    _lib.set_debug_option("orf_chunk", -1)
    yield
    _lib.set_debug_option("host_translate", -1)


def dna(text, **kw):
    return easel.TextSequence(sequence=text, **kw).digitize(DNA)


def make_block(seqs, alphabet="dna"):
    abc = DNA if alphabet == "dna" else RNA
    return easel.DigitalSequenceBlock(abc, [easel.TextSequence(name=f"s{i}", sequence=s).digitize(abc) for i, s in enumerate(seqs)])


def expected_arrays(want):
    """The arrays of a TranslatedBlock that holds the ORFs <want> of the restatement."""
    dsq = [255]
    offsets = []
    for o in want:
        offsets.append(len(dsq))
        dsq.extend(tc.AMINO.index(c) for c in o["residues"])
        dsq.append(255)
    return dict(dsq=np.array(dsq, dtype=np.uint8), offsets=np.array(offsets, dtype=np.int64),
                lengths=np.array([len(o["residues"]) for o in want], dtype=np.int32),
                source=np.array([o["source"] for o in want], dtype=np.int64), frame=np.array([o["frame"] for o in want], dtype=np.int8),
                start=np.array([o["start"] for o in want], dtype=np.int64), end=np.array([o["end"] for o in want], dtype=np.int64))


def block_arrays(orfs):
    pk = orfs.packed()
    return dict(dsq=pk.dsq, offsets=pk.offsets, lengths=pk.lengths, source=orfs.source_index, frame=orfs.frame, start=orfs.start, end=orfs.end)


def assert_same_arrays(got, want, label):
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (label, key)


_expected = {}


def expected_of(case):
    """The restatement's ORFs of a case, computed once for the host and the device tests."""
    label, seqs, alphabet, table, min_length, strand = case
    if label not in _expected:
        _expected[label] = tc.orfs([s.replace("U", "T") for s in seqs], table, min_length, strand)
    return _expected[label]


CASES = tc.orf_cases()


# ------------------------------------------------------------------------------------------- 1. the reference's recorded cases
def test_translate_sequence_recorded_cases():
    gencode = easel.GeneticCode()
    seq = dna("ATGCTGCCCGGTTTGGCACTGCTCCTGCTGGCCGCC")
    assert seq.translate(gencode).textize().sequence == "MLPGLALLLLAA"
    assert seq.translate().textize().sequence == "MLPGLALLLLAA"
    prot = dna("ATGCTGCCCGGT", name="seq", source="source", description="d", accession="a").translate(gencode)
    assert (prot.name, prot.source, prot.description, prot.accession) == ("seq", "source", "d", "a") and prot.alphabet == AMINO
    assert easel.DigitalSequence(DNA).translate(gencode).textize().sequence == ""
    with pytest.raises(AlphabetMismatch):
        easel.DigitalSequence(AMINO).translate(gencode)
    with pytest.raises(ValueError):
        dna("ATGCT").translate(gencode)
    with pytest.raises(ValueError):
        dna("ATGC-T").translate(gencode)            # a codon with a gap: the stated deviation, translate refuses it


def test_translate_block_recorded_cases():
    block = easel.DigitalSequenceBlock(DNA, [dna("ATGCTG", name="seq1", description="one", source="some_source"),
                                             dna("ATGCCC", name="seq2", description="two", source="other_source"),
                                             dna("ATTCTGATGATA", name="seq3")])
    prots = block.translate()
    assert prots.alphabet == AMINO and len(prots) == 3
    assert [p.textize().sequence for p in prots] == ["ML", "MP", "ILMI"]
    assert [p.name for p in prots] == ["seq1", "seq2", "seq3"]
    assert [p.description for p in prots] == ["one", "two", ""] and [p.source for p in prots] == ["some_source", "other_source", ""]
    gencode = easel.GeneticCode()
    assert len(easel.DigitalSequenceBlock(DNA).translate(gencode)) == 0
    with pytest.raises(AlphabetMismatch):
        easel.DigitalSequenceBlock(AMINO).translate(gencode)
    with pytest.raises(AlphabetMismatch):
        easel.DigitalSequenceBlock(AMINO).translate_orfs(gencode)
    with pytest.raises(ValueError, match="index 1"):
        easel.DigitalSequenceBlock(DNA, [dna("ATG"), dna("ATGC")]).translate()
    with pytest.raises(ValueError, match="index 2"):
        easel.DigitalSequenceBlock(DNA, [dna("ATG"), dna(""), dna("ATGAT~")]).translate()
    stops = easel.DigitalSequenceBlock(DNA, [dna("ATGTAAGGR")]).translate()
    assert stops[0].textize().sequence == "M*G"


def test_genetic_code_recorded_cases():
    with pytest.raises(ValueError):
        easel.GeneticCode(42)
    with pytest.raises(InvalidParameter):
        easel.GeneticCode(42)
    gencode = easel.GeneticCode()
    prot = gencode.translate(bytearray())
    assert len(prot) == 0 and prot.dtype == np.uint8
    with pytest.raises(ValueError):
        gencode.translate(bytearray([0, 0, 0, 1, 1]))
    g11 = easel.GeneticCode(11)
    g2 = pickle.loads(pickle.dumps(g11))
    assert (g2.translation_table, g2.nucleotide_alphabet, g2.amino_alphabet) == (11, g11.nucleotide_alphabet, g11.amino_alphabet)
    assert repr(g11) == "GeneticCode(11)" and repr(easel.GeneticCode(4, nucleotide_alphabet=RNA)) == "GeneticCode(4, nucleotide_alphabet=Alphabet.rna())"
    assert gencode.description == "Standard" and g11.description == "Bacterial, Archaeal and Plant Plastid"
    gencode.translation_table = 4
    assert gencode.translation_table == 4 and AMINO.decode(gencode.translate(DNA.encode("TGA"))) == "W"
    with pytest.raises(InvalidParameter):
        gencode.translation_table = 7
    with pytest.raises(InvalidParameter):
        easel.GeneticCode(nucleotide_alphabet=AMINO)
    with pytest.raises(InvalidParameter):
        easel.GeneticCode(amino_alphabet=DNA)


def test_reverse_complement_recorded_cases():
    seq = dna("ATGC")
    assert seq.reverse_complement().textize().sequence == "GCAT" and seq.textize().sequence == "ATGC"
    assert seq.reverse_complement(inplace=True) is None and seq.textize().sequence == "GCAT"
    assert dna("ACGTRYMKSWHBVDN-*~").reverse_complement().textize().sequence == "~*-NHBVDWSMKRYACGT"
    prot = easel.TextSequence(sequence="MEMLP").digitize(AMINO)
    with pytest.raises(ValueError):
        prot.reverse_complement()
    with pytest.raises(ValueError):
        prot.reverse_complement(inplace=True)
    text = easel.TextSequence(sequence="ATGC")
    assert text.reverse_complement().sequence == "GCAT" and text.sequence == "ATGC"
    assert text.reverse_complement(inplace=True) is None and text.sequence == "GCAT"
    assert easel.TextSequence(sequence="acgTRy").reverse_complement().sequence == "rYAcgt"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(Warning):
            easel.TextSequence(sequence="MEMLP").reverse_complement()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert easel.TextSequence(sequence="MEMLP").reverse_complement().sequence == "NNKNK"


def test_msa_reverse_complement_recorded_case():
    rows = ["..TTAAAACC", "AAAAGGAATT", "CCCCGGGG..", "GGGGGGGGGG"]
    msa = easel.TextMSA(sequences=[easel.TextSequence(name=f"seq{i + 1}", sequence=r) for i, r in enumerate(rows)]).digitize(DNA)
    want = ["GGTTTTAA--", "AATTCCTTTT", "--CCCCGGGG", "CCCCCCCCCC"]
    rc = msa.reverse_complement()
    assert [DNA.decode(s.sequence) for s in rc.sequences] == want and rc.names == msa.names
    assert [DNA.decode(s.sequence) for s in msa.sequences] == [r.replace(".", "-") for r in rows]
    assert msa.reverse_complement(inplace=True) is None
    assert [DNA.decode(s.sequence) for s in msa.sequences] == want
    with pytest.raises(ValueError):
        easel.TextMSA(sequences=[easel.TextSequence(name="p", sequence="MEMLP")]).digitize(AMINO).reverse_complement()


# ------------------------------------------------------------------------------------------- 2. every codon
@pytest.mark.parametrize("table", sorted(tc.DIFFERENCES))
def test_every_codon_of_every_table(table):
    letters = "ACGTRYMKSWHBVDN"
    codons = ["".join(c) for c in itertools.product(letters, repeat=3)]
    assert len(codons) == 15 ** 3                                       # the codes 0..3 and 5..15
    got = AMINO.decode(easel.GeneticCode(table).translate(DNA.encode("".join(codons))))
    want = "".join(tc.translate_codon(table, c) for c in codons)
    assert got == want
    assert not set(got) & set("JBZ")
    aa64, lut = easel.GeneticCode(table)._tables()
    assert AMINO.decode(aa64) == "".join(tc.code_table(table)["".join(c)] for c in itertools.product("TCAG", repeat=3))
    assert lut.shape == (18 ** 3,)
    for c1, c2, c3 in itertools.product(range(18), repeat=3):
        cell = int(lut[(c1 * 18 + c2) * 18 + c3])
        want1 = tc.translate_codon(table, tc.NT[c1] + tc.NT[c2] + tc.NT[c3])
        assert cell == (tc.AMINO.index("X") | 0x80 if want1 is None else tc.AMINO.index(want1)), (c1, c2, c3)


def test_named_codons():
    def t(table, codon, alphabet=DNA):
        return AMINO.decode(easel.GeneticCode(table, nucleotide_alphabet=alphabet).translate(alphabet.encode(codon)))
    assert t(1, "GGR") == "G" and t(1, "TTY") == "F" and t(1, "UUY", RNA) == "F"
    assert t(1, "TAR") == "*" and t(1, "TRA") == "*"
    assert t(1, "TGR") == "X" and t(4, "TGR") == "W"
    assert t(1, "NNN") == "X"


# ------------------------------------------------------------------------------------------- 3. ORFs, twin = restatement
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_orfs_equal_the_restatement(case):
    label, seqs, alphabet, table, min_length, strand = case
    code = easel.GeneticCode(table, nucleotide_alphabet=DNA if alphabet == "dna" else RNA)
    orfs = make_block(seqs, alphabet).translate_orfs(code, min_length=min_length, strand=strand)
    assert not orfs.on_device and orfs.alphabet == AMINO
    want = expected_of(case)
    assert label.startswith("lengths") or label.startswith("stops") or len(want) > 10
    assert_same_arrays(block_arrays(orfs), expected_arrays(want), label)
    assert len(orfs) == len(want)


def test_orf_case_properties():
    """The cases hold what they are there for."""
    by = {c[0]: c for c in CASES}
    for m in (1, 20):
        want = expected_of(by[f"stops, min_length {m}"])
        lens = sorted(len(o["residues"]) for o in want if o["source"] == 4 and o["frame"] == 1)
        assert lens == [m, m]                                   # the run of min_length - 1 is not reported
        assert any(o["source"] == 5 and o["frame"] == 2 and len(o["residues"]) == m for o in want)
    mixed = expected_of(by["mixed block"])
    assert {o["frame"] for o in mixed} == {1, 2, 3, -1, -2, -3} and max(o["source"] for o in mixed) == 301
    assert any("X" in o["residues"] for o in expected_of(by["degenerate, table 1"]))
    with pytest.raises(InvalidParameter):
        make_block(["ACGT"]).translate_orfs(min_length=0)
    with pytest.raises(InvalidParameter):
        make_block(["ACGT"]).translate_orfs(strand="both")


def test_translated_block_sequences():
    seqs = ["", "CC" + "GCT" * 30 + "TAA" + "GCA" * 25, "ACGT"]
    block = make_block(seqs)
    orfs = block.translate_orfs(min_length=20, strand="watson")
    assert len(orfs) == 4 and list(orfs.source_index) == [1, 1, 1, 1] and list(orfs.frame) == [1, 2, 3, 3]
    first = orfs[0]
    assert (first.name, first.source, first.alphabet) == ("orf1", "s1", AMINO)
    assert first.description == f"source=s1 coords={orfs.start[0]}..{orfs.end[0]} length={len(first)} frame={orfs.frame[0]}"
    assert orfs[-1].name == "orf4" and [s.name for s in orfs] == ["orf1", "orf2", "orf3", "orf4"]
    # the tables a search reads: NUL-terminated names and descriptions
    tab = bytes(orfs._strtab)
    for i in range(4):
        assert tab[int(orfs._name_off[i]):].split(b"\0")[0] == f"orf{i + 1}".encode()
        assert tab[int(orfs._desc_off[i]):].split(b"\0")[0] == orfs[i].description.encode()


# ------------------------------------------------------------------------------------------- 4. coordinates
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_coordinates_give_back_the_residues(case):
    label, seqs, alphabet, table, min_length, strand = case
    code = easel.GeneticCode(table, nucleotide_alphabet=DNA if alphabet == "dna" else RNA)
    block = make_block(seqs, alphabet)
    orfs = block.translate_orfs(code, min_length=min_length, strand=strand)
    pk = orfs.packed()
    for n in range(len(orfs)):
        src = seqs[int(orfs.source_index[n])].replace("U", "T")
        start, end, frame = int(orfs.start[n]), int(orfs.end[n]), int(orfs.frame[n])
        nt = src[start - 1:end] if frame > 0 else tc.reverse_complement(src[end - 1:start])
        residues = AMINO.decode(pk.dsq[pk.offsets[n]:pk.offsets[n] + pk.lengths[n]])
        assert "".join(tc.translate_codon(table, nt[i:i + 3]) or "X" for i in range(0, len(nt), 3)) == residues, (label, n)
        assert len(nt) == 3 * len(residues)
        # locate: an amino range back to nucleotides
        i, j = 1 + len(residues) // 3, len(residues) - len(residues) // 4
        dom = SimpleNamespace(hit=SimpleNamespace(name=f"orf{n + 1}"), alignment=SimpleNamespace(target_from=i, target_to=j))
        name, k, a, b, fr = orfs.locate(dom)
        assert (name, k, fr) == (f"s{k}", int(orfs.source_index[n]), frame)
        part = src[a - 1:b] if frame > 0 else tc.reverse_complement(src[b - 1:a])
        assert "".join(tc.translate_codon(table, part[x:x + 3]) or "X" for x in range(0, len(part), 3)) == residues[i - 1:j], (label, n)
        assert orfs.locate(SimpleNamespace(best_domain=dom)) == (name, k, a, b, fr)
    with pytest.raises(ValueError):
        orfs.locate(SimpleNamespace(hit=SimpleNamespace(name="s0"), alignment=SimpleNamespace(target_from=1, target_to=1)))


# ------------------------------------------------------------------------------------------- 5. real data
def check_genbank_cds(orfs_crick, orfs_watson, L):
    """The ten CDS of BGC0001090 (all on the complement strand) among the crick ORFs of the record, and among the watson
    ORFs of its reverse complement with mirrored coordinates."""
    cds = tc.genbank_cds(GBK)
    assert len(cds) == 10 and all(c[2] for c in cds) and max(b - a + 1 for a, b, _, _ in cds) == 16092
    for orfs, mirrored in ((orfs_crick, False), (orfs_watson, True)):
        pk = orfs.packed()
        ends = {int(e): n for n, e in enumerate(orfs.end) if (orfs.frame[n] > 0) == mirrored}
        for a, b, _, translation in cds:
            end = L + 1 - (a + 3) if mirrored else a + 3            # the stop codon is not part of the ORF
            assert end in ends, (a, b, mirrored)
            n = ends[end]
            assert (orfs.start[n] <= L + 1 - b) if mirrored else (orfs.start[n] >= b)
            residues = AMINO.decode(pk.dsq[pk.offsets[n]:pk.offsets[n] + pk.lengths[n]])
            assert len(residues) >= len(translation) == (b - a + 1) // 3 - 1
            assert residues[-len(translation) + 1:] == translation[1:], (a, b, mirrored)      # the start codon reads M whatever it encodes


def test_genbank_cds_are_among_the_orfs():
    with easel.SequenceFile(GBK, format="genbank", digital=True, alphabet=DNA) as sf:
        rec = sf.read()
    assert len(rec) == 44660
    code = easel.GeneticCode(11)
    crick = easel.DigitalSequenceBlock(DNA, [rec]).translate_orfs(code, min_length=20)
    watson = easel.DigitalSequenceBlock(DNA, [rec.reverse_complement()]).translate_orfs(code, min_length=20)
    check_genbank_cds(crick, watson, len(rec))


# ------------------------------------------------------------------------------------------- 6. the plan
@pytest.mark.parametrize("chunk", [4, 64, 65, -1])
def test_chunks_do_not_depend_on_the_split(chunk):
    """The units of work are cut from the packed array: their number follows from the nucleotides, the chunk length and
    at most one more per sequence boundary, whatever the lengths of the sequences."""
    _lib.set_debug_option("orf_chunk", chunk)
    rng = np.random.default_rng(3)
    nt = "".join("ACGT"[i] for i in rng.integers(0, 4, size=6000))
    splits = [[nt[:5997], nt[5997:5998], nt[5998:5999], nt[5999:]], [nt[:1500], nt[1500:3000], nt[3000:4500], nt[4500:]],
              ["", nt, "", ""]]
    used, chunks = C.c_int32(), C.c_int64()
    assert _lib.lib().p7x_orfs_plan(6000, 4, C.byref(used), C.byref(chunks)) == 0
    c = used.value
    assert c == (196 if chunk < 0 else chunk)
    assert -(-6000 // c) <= chunks.value <= -(-6000 // c) + 4 + 1
    for split in splits:
        orfs = make_block(split).translate_orfs(min_length=20)
        assert (orfs.chunks, orfs.orf_chunk) == (chunks.value, c)
    one = make_block([nt]).translate_orfs(min_length=20)
    assert -(-6000 // c) <= one.chunks <= -(-6000 // c) + 1 + 1
    _lib.set_debug_option("orf_chunk", -1)
