"""Translation on the device (p7x_translate.hip): the ORF finder and the in-frame translation give the bytes of the host
twin at every chunk length, twice over; the ten CDS of BGC0001090.gbk with the longest spread over some 250 chunks; and a
planted protein found by hmmsearch in the ORFs of both strands and located on its contig."""
import numpy as np
import pytest

import translate_cases as tc
from conftest import GOLDEN
from pyhmmer_amd import _lib, easel, hmmer
from test_gpu_search import _hit_fields
from test_host_translate import CASES, GBK, assert_same_arrays, block_arrays, check_genbank_cds, expected_arrays, expected_of, make_block

pytestmark = pytest.mark.gpu

DNA, RNA, AMINO = easel.Alphabet.dna(), easel.Alphabet.rna(), easel.Alphabet.amino()
CHUNKS = [4, 7, 64, 65, -1]                 # -1: the default


@pytest.fixture(autouse=True)
def options(libp7x):
    _lib.set_debug_option("host_translate", -1)
    _lib.set_debug_option("orf_chunk", -1)
    yield
    _lib.set_debug_option("host_translate", -1)
    _lib.set_debug_option("orf_chunk", -1)


def twin(fn):
    _lib.set_debug_option("host_translate", 1)
    try:
        return fn()
    finally:
        _lib.set_debug_option("host_translate", -1)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_orfs_equal_the_twin(case):
    label, seqs, alphabet, table, min_length, strand = case
    code = easel.GeneticCode(table, nucleotide_alphabet=DNA if alphabet == "dna" else RNA)
    block = make_block(seqs, alphabet)
    find = lambda: block.translate_orfs(code, min_length=min_length, strand=strand)
    host = twin(find)
    assert not host.on_device
    want = block_arrays(host)
    assert_same_arrays(want, expected_arrays(expected_of(case)), label)
    for chunk in CHUNKS:
        _lib.set_debug_option("orf_chunk", chunk)
        first, second = find(), find()
        assert first.on_device and second.on_device and first.orf_chunk == (196 if chunk < 0 else chunk)
        assert_same_arrays(block_arrays(first), want, (label, chunk))
        assert_same_arrays(block_arrays(second), block_arrays(first), (label, chunk, "second run"))


def test_device_block_translation_equals_the_twin():
    seqs = [s[:len(s) // 3 * 3] for s in tc.mixed_block()]
    block = make_block(seqs)
    for table in (1, 11):
        code = easel.GeneticCode(table)
        host, dev = twin(lambda: block.translate(code)), block.translate(code)
        assert len(dev) == len(host) == len(seqs)
        for a, b, s in zip(dev, host, seqs):
            assert np.array_equal(a.sequence, b.sequence) and (a.name, a.alphabet) == (b.name, AMINO)
            assert AMINO.decode(a.sequence) == tc.translate(table, s)
    # the error case reports the same sequence and codon
    bad = list(seqs)
    bad[200] = bad[200][:3] + "A-C" + bad[200][6:] if len(bad[200]) >= 6 else "A-C"
    bad[301] = bad[301][:600] + "~" + bad[301][601:]
    messages = []
    for run in (lambda: make_block(bad).translate(), lambda: twin(lambda: make_block(bad).translate())):
        with pytest.raises(ValueError) as err:
            run()
        messages.append(str(err.value))
    assert messages[0] == messages[1] and "index 200" in messages[0]
    short = list(seqs)
    short[17] = "ACGT"
    with pytest.raises(ValueError, match="index 17"):
        make_block(short).translate()


def test_genbank_cds_on_the_device_across_chunks():
    with easel.SequenceFile(GBK, format="genbank", digital=True, alphabet=DNA) as sf:
        rec = sf.read()
    code = easel.GeneticCode(11)
    _lib.set_debug_option("orf_chunk", 64)
    crick = easel.DigitalSequenceBlock(DNA, [rec]).translate_orfs(code, min_length=20)
    watson = easel.DigitalSequenceBlock(DNA, [rec.reverse_complement()]).translate_orfs(code, min_length=20)
    assert crick.on_device and watson.on_device and crick.orf_chunk == 64 and crick.chunks == -(-(len(rec) + 2) // 64)
    check_genbank_cds(crick, watson, len(rec))
    assert max(crick.packed().lengths) * 3 // 64 >= 250          # the longest ORF spans that many chunks


def test_planted_protein_is_found_and_located(models):
    hmm = models["PF02826"][0]
    P = hmm.emit_sequence(easel.Randomness(42))
    protein = AMINO.decode(P.sequence)
    assert len(protein) >= 20 and set(protein) <= set(tc.AMINO[:20])
    first_codon = {}
    for codon, aa in zip(("".join(c) for c in __import__("itertools").product("TCAG", repeat=3)), tc.STANDARD):
        first_codon.setdefault(aa, codon)
    cds = "".join(first_codon[a] for a in protein)
    insert = "TAA" + cds + "TAA"
    rng = np.random.default_rng(9)
    rand = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))
    off0, off1 = 1000, 2345
    contig0 = rand(off0) + insert + rand(1500)
    contig1 = rand(off1) + tc.reverse_complement(insert) + rand(777)
    block = make_block([contig0, contig1])
    orfs = block.translate_orfs(min_length=20)
    assert orfs.on_device
    pk = orfs.packed()
    # the expected records: watson of contig 0, crick of contig 1
    n = len(protein)
    L1 = len(contig1)
    want = {0: (off0 + 4, off0 + 3 + 3 * n, (off0 + 3) % 3 + 1),
            1: (off1 + 3 + 3 * n, off1 + 4, -((L1 - (off1 + 3 + 3 * n)) % 3 + 1))}
    found = {}
    for k, (start, end, frame) in want.items():
        hit = [i for i in range(len(orfs)) if (orfs.source_index[i], orfs.start[i], orfs.end[i], orfs.frame[i]) == (k, start, end, frame)]
        assert len(hit) == 1, (k, start, end, frame)
        i = hit[0]
        assert np.array_equal(pk.dsq[pk.offsets[i]:pk.offsets[i] + pk.lengths[i]], P.sequence)
        found[f"orf{i + 1}"] = k
    Z = 1000.0
    direct = next(hmmer.hmmsearch([hmm], easel.DigitalSequenceBlock(AMINO, [easel.DigitalSequence(AMINO, name="P", sequence=P.sequence)]), Z=Z))
    hits = next(hmmer.hmmsearch([hmm], orfs, Z=Z))
    assert len(direct) == 1
    mine = [h for h in hits if h.name in found]
    assert sorted(h.name for h in mine) == sorted(found)
    for h in mine:
        # one search against another of the same device path: field by field, as tests/test_gpu_search.py compares them
        assert _hit_fields([h])[0][1:] == _hit_fields(direct)[0][1:]
        k = found[h.name]
        name, index, a, b, frame = orfs.locate(h)
        assert (name, index, frame) == (f"s{k}", k, want[k][2]) and orfs.locate(h.best_domain) == (name, index, a, b, frame)
        lo, hi = min(want[k][:2]), max(want[k][:2])
        assert lo <= min(a, b) and max(a, b) <= hi and (a < b) == (k == 0)
        assert h.description.startswith(f"source=s{k} coords={want[k][0]}..{want[k][1]} ")
