"""Translation and six-frame ORFs restated in plain Python, sharing nothing with the product: the tables
are built from the standard code's string and NCBI's differences, sequences are text, codons are slices mapped through a
dict, ORFs are what is left when a frame's translation is split at its stops.  Also the case generators of the translate
tests and a small parser of the CDS features of a GenBank record."""
import itertools
import random
import re

NT = "ACGT-RYMKSWHBVDN*~"
AMINO = "ACDEFGHIKLMNPQRSTVWY-BJZOUX*~"
STANDARD = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"      # NCBI order: TCAG, first base slowest
DIFFERENCES = {
    1: "", 2: "AGA* AGG* ATAM TGAW", 3: "ATAM CTTT CTCT CTAT CTGT TGAW", 4: "TGAW", 5: "AGAS AGGS ATAM TGAW", 6: "TAAQ TAGQ",
    9: "AAAN AGAS AGGS TGAW", 10: "TGAC", 11: "", 12: "CTGS", 13: "AGAG AGGG ATAM TGAW", 14: "AAAN AGAS AGGS TAAY TGAW",
    16: "TAGL", 21: "TGAW ATAM AGAS AGGS AAAN", 22: "TCA* TAGL", 23: "TTA*", 24: "AGAS AGGK TGAW", 25: "TGAG",
}
EXPANSION = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "M": "AC", "K": "GT", "S": "CG", "W": "AT",
             "H": "ACT", "B": "CGT", "V": "ACG", "D": "AGT", "N": "ACGT"}
COMPLEMENT = dict(zip("ACGTURYMKSWHBVDN-*~", "TGCAAYRKMSWDVBHN-*~"))
_tables = {}


def code_table(table):
    """{codon of ACGT: amino letter} of an NCBI table."""
    if table not in _tables:
        t = {"".join(c): STANDARD[i] for i, c in enumerate(itertools.product("TCAG", repeat=3))}
        for change in DIFFERENCES[table].split():
            t[change[:3]] = change[3]
        _tables[table] = t
    return _tables[table]


def translate_codon(table, codon, _seen={}):
    """The amino letter of a codon of text; None when it holds a gap, * or ~."""
    if (table, codon) not in _seen:
        if any(c not in EXPANSION for c in codon):
            _seen[table, codon] = None
        else:
            t = code_table(table)
            got = {t["".join(c)] for c in itertools.product(*(EXPANSION[c] for c in codon))}
            _seen[table, codon] = got.pop() if len(got) == 1 else "X"
    return _seen[table, codon]


def reverse_complement(seq):
    return "".join(COMPLEMENT[c] for c in reversed(seq))


def translate(table, seq):
    return "".join(translate_codon(table, seq[i:i + 3]) for i in range(0, len(seq), 3))


def orfs(seqs, table=1, min_length=20, strand=None):
    """The ORFs of a list of text sequences, in output order: dicts of residues, source, frame, start, end."""
    out = []
    for k, seq in enumerate(seqs):
        L = len(seq)
        for which in ("watson", "crick"):
            if strand not in (None, which):
                continue
            S = seq if which == "watson" else reverse_complement(seq)
            found = []
            for f in (1, 2, 3):
                codons = [S[i:i + 3] for i in range(f - 1, L - 2, 3)]
                aa = "".join(translate_codon(table, c) or "X" for c in codons)
                a = 0
                for run in aa.split("*"):
                    b = a + len(run)
                    if run and b - a >= min_length:
                        if which == "watson":
                            found.append((f + 3 * a, dict(residues=run, source=k, frame=f, start=f + 3 * a, end=f + 3 * b - 1)))
                        else:
                            found.append((f + 3 * a, dict(residues=run, source=k, frame=-f, start=L + 1 - (f + 3 * a), end=L + 2 - (f + 3 * b))))
                    a = b + 1
            out.extend(o for _, o in sorted(found, key=lambda x: x[0]))
    return out


# ---------------------------------------------------------------------------------------------------------- cases
def _random_dna(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def mixed_block(seed=5):
    """300 random reads of 0..200 nt, one random contig of 20,000 nt, empty sequences at both ends."""
    rng = random.Random(seed)
    return [""] + [_random_dna(rng, rng.randint(0, 200)) for _ in range(300)] + [_random_dna(rng, 20000)] + ["", ""]


def orf_cases():
    """(label, sequences, alphabet, table, min_length, strand)."""
    rng = random.Random(11)
    A, stop = "GCT", "TAA"
    cases = [("lengths 0..6", [_random_dna(rng, n, "ACG") for n in range(7)], "dna", 1, 1, None)]
    for m in (1, 20):
        stops = [
            stop + A * (m + 2),                                     # a stop as the first codon
            A * (m + 2) + stop,                                     # as the last codon
            A * m + stop + stop + A * (m + 1),                      # two adjacent stops
            A * (2 * m + 3),                                        # no stop at all
            stop + A * m + stop + A * (m - 1) + stop + A * m,       # runs of exactly min_length and of one less
            "C" + A * m + stop + "GG" + A * (m - 1) + "TAG",        # the same out of frame 1
        ]
        cases.append((f"stops, min_length {m}", stops, "dna", 1, m, None))
    reads = [_random_dna(rng, rng.randint(0, 400)) for _ in range(40)]
    for strand in (None, "watson", "crick"):
        cases.append((f"strand {strand}", reads, "dna", 1, 5, strand))
    degenerate = [_random_dna(rng, 300, "ACGTRYMKSWHBVDN"), "N" * 90 + _random_dna(rng, 100) + "N" * 31, "GGRTTYTARTRATGR" * 9,
                  _random_dna(rng, 60) + "A-C" + _random_dna(rng, 61) + "*~" + _random_dna(rng, 30)]
    for table in (1, 4, 11):
        cases.append((f"degenerate, table {table}", degenerate, "dna", table, 3, None))
    cases.append(("rna", [s.replace("T", "U") for s in reads[:12]], "rna", 1, 5, None))
    cases.append(("mixed block", mixed_block(), "dna", 1, 20, None))
    cases.append(("mixed block, min_length 1", mixed_block(7)[280:], "dna", 11, 1, None))
    return cases


# ---------------------------------------------------------------------------------------------------------- GenBank
def genbank_cds(path):
    """[(a, b, complement, translation)] of the CDS features of the first record."""
    out, lines = [], open(path).read().splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^     CDS\s+(complement\()?(\d+)\.\.(\d+)\)?\s*$", lines[i])
        i += 1
        if not m:
            continue
        text = None
        while i < len(lines) and lines[i].startswith(" " * 21):
            if lines[i].strip().startswith("/translation="):
                text = lines[i].strip()[len("/translation="):]
                while text.count('"') < 2:
                    i += 1
                    text += lines[i].strip()
            i += 1
        out.append((int(m.group(2)), int(m.group(3)), bool(m.group(1)), text.strip('"')))
    return out
