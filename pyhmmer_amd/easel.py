"""Minimal host-side mirror of the parts of ``pyhmmer.easel`` that sit on the
``p7_Pipeline`` hot path: the digital alphabets, digital sequences, the
``DigitalSequenceBlock`` input container and a FASTA ``SequenceFile`` reader.

Reference: ``src/pyhmmer/easel.pyx`` -- ``Alphabet`` (:183-528), ``TextSequence``
(:7483), ``DigitalSequence`` (:7741), ``DigitalSequenceBlock`` (:8629-8665),
``SequenceFile`` (read / read_block), ``MSA`` / ``TextMSA`` / ``DigitalMSA`` as far as hmmalign needs them, and
``Randomness`` (:7006-7161), the generator the emitters of ``plan7`` draw from.  Everything else in ``pyhmmer.easel``
(SSI, matrices, ...) is out of scope.

The one deliberate difference from the reference: a ``DigitalSequenceBlock`` here can
be *packed* once (``block.packed()``) into the flat ``dsq_concat + offsets + lengths``
arrays the C-ABI consumes (``include/p7x.h``), instead of an array of ``ESL_SQ*``.
"""
from __future__ import annotations

import io
import os
from typing import Iterable, Iterator, List, Optional, Sequence as _Seq

import numpy as np

__all__ = [
    "Alphabet", "GeneticCode", "Sequence", "TextSequence", "DigitalSequence",
    "TextSequenceBlock", "DigitalSequenceBlock", "TranslatedBlock", "ShuffledBlock", "SequenceFile", "MSA", "TextMSA", "DigitalMSA", "MSAFile", "Randomness", "KeyHash",
]

_AMINO = "ACDEFGHIKLMNPQRSTVWY-BJZOUX*~"
_DNA = "ACGT-RYMKSWHBVDN*~"
_RNA = "ACGU-RYMKSWHBVDN*~"

eslRNA, eslDNA, eslAMINO = 1, 2, 3   # libeasel/alphabet.pxd type codes
DSQ_SENTINEL = 255                   # libeasel/__init__.pxd:21 (eslDSQ_SENTINEL)
_MSA_WEIGHT_PREFERENCES = ("conscover", "origorder", "random")      # easel.pyx:175-179
_SHUFFLE_MODES = ("mono", "di", "window", "reverse")                # P7X_SHUFFLE_*: the index is the mode of the C-ABI


class Alphabet:
    """A biological alphabet (reference ``easel.pyx:183-528``)."""

    __slots__ = ("type_code", "symbols", "K", "Kp", "_lut")

    def __init__(self, type_code: int):
        if type_code == eslAMINO:
            self.symbols, self.K = _AMINO, 20
        elif type_code == eslDNA:
            self.symbols, self.K = _DNA, 4
        elif type_code == eslRNA:
            self.symbols, self.K = _RNA, 4
        else:
            raise ValueError(f"unsupported alphabet type {type_code}")
        self.type_code = type_code
        self.Kp = len(self.symbols)
        lut = np.full(256, 255, dtype=np.uint8)
        for i, c in enumerate(self.symbols):
            lut[ord(c)] = i
            lut[ord(c.lower())] = i
        if type_code != eslAMINO:          # Easel synonyms: U<->T, X -> N, I->A? (only the common ones)
            lut[ord("U")] = lut[ord("u")] = 3
            lut[ord("T")] = lut[ord("t")] = 3
            lut[ord("X")] = lut[ord("x")] = self.symbols.index("N")
        lut[ord("_")] = lut[ord(".")] = self.K   # gap synonyms
        self._lut = lut

    # -- constructors mirroring the reference class methods
    @classmethod
    def amino(cls) -> "Alphabet":
        return cls(eslAMINO)

    @classmethod
    def dna(cls) -> "Alphabet":
        return cls(eslDNA)

    @classmethod
    def rna(cls) -> "Alphabet":
        return cls(eslRNA)

    @property
    def type(self) -> str:
        return {eslAMINO: "amino", eslDNA: "DNA", eslRNA: "RNA"}[self.type_code]

    @property
    def gap_symbol(self) -> str:
        return self.symbols[self.K]

    @property
    def gap_index(self) -> int:
        return self.K

    def is_amino(self) -> bool:
        return self.type_code == eslAMINO

    def is_dna(self) -> bool:
        return self.type_code == eslDNA

    def is_rna(self) -> bool:
        return self.type_code == eslRNA

    def is_nucleotide(self) -> bool:
        return self.type_code in (eslDNA, eslRNA)

    def __eq__(self, other) -> bool:
        return isinstance(other, Alphabet) and other.type_code == self.type_code

    def __hash__(self) -> int:
        return hash(self.type_code)

    def __repr__(self) -> str:
        return f"Alphabet.{ {eslAMINO: 'amino', eslDNA: 'dna', eslRNA: 'rna'}[self.type_code] }()"

    def encode(self, sequence: str) -> np.ndarray:
        raw = np.frombuffer(sequence.encode("ascii"), dtype=np.uint8)
        enc = self._lut[raw]
        if (enc == 255).any():
            bad = sequence[int(np.argmax(enc == 255))]
            raise ValueError(f"Invalid symbol {bad!r} for alphabet {self!r}")
        return enc

    def decode(self, sequence) -> str:
        arr = np.asarray(sequence, dtype=np.uint8)
        if arr.size and int(arr.max()) >= self.Kp:
            raise ValueError("invalid digital code in sequence")
        return "".join(self.symbols[i] for i in arr.tolist())


# reverse complement over Easel's nucleotide codes: A<->T C<->G R<->Y M<->K H<->D B<->V; S W N - * ~ stay
_NT_COMPLEMENT = np.array([3, 2, 1, 0, 4, 6, 5, 8, 7, 9, 10, 14, 13, 12, 11, 15, 16, 17], dtype=np.uint8)
_STRANDS = {None: 0, "watson": 1, "crick": 2}           # P7X_STRAND_*


def _text_complement_table() -> bytes:
    """IUPAC complement of a text sequence, case kept; any other byte maps to 0 (the caller writes N and warns)."""
    tab = bytearray(256)
    for a, b in zip("ACGTURYMKSWHBVDN", "TGCAAYRKMSWDVBHN"):
        tab[ord(a)], tab[ord(a.lower())] = ord(b), ord(b.lower())
    return bytes(tab)


_TEXT_COMPLEMENT = _text_complement_table()
# the same for the rows of an alignment: whatever is no IUPAC letter (gaps, *, ~) stays
_TEXT_COMPLEMENT_KEEP = bytes(c or i for i, c in enumerate(_TEXT_COMPLEMENT))


class GeneticCode:
    """A genetic code table for translation (reference ``easel.pyx:557-716``).  The tables are NCBI's, written from the
    standard code and the published differences; ``description`` is this package's own wording."""

    __slots__ = ("nucleotide_alphabet", "amino_alphabet", "_table", "_description")

    def __init__(self, translation_table: int = 1, *, nucleotide_alphabet: Optional[Alphabet] = None,
                 amino_alphabet: Optional[Alphabet] = None):
        from .errors import InvalidParameter
        nucleotide_alphabet = Alphabet.dna() if nucleotide_alphabet is None else nucleotide_alphabet
        amino_alphabet = Alphabet.amino() if amino_alphabet is None else amino_alphabet
        if not nucleotide_alphabet.is_nucleotide():
            raise InvalidParameter("nucleotide_alphabet", nucleotide_alphabet, hint="nucleotide alphabet")
        if not amino_alphabet.is_amino():
            raise InvalidParameter("amino_alphabet", amino_alphabet, hint="amino alphabet")
        self.nucleotide_alphabet, self.amino_alphabet = nucleotide_alphabet, amino_alphabet
        self.translation_table = translation_table

    def __repr__(self) -> str:
        ty = type(self).__name__
        if self.nucleotide_alphabet.is_dna():
            return f"{ty}({self.translation_table!r})"
        return f"{ty}({self.translation_table!r}, nucleotide_alphabet={self.nucleotide_alphabet!r})"

    def __reduce__(self):
        import functools
        return functools.partial(type(self), translation_table=self.translation_table,
                                 nucleotide_alphabet=self.nucleotide_alphabet, amino_alphabet=self.amino_alphabet), ()

    @property
    def translation_table(self) -> int:
        return self._table

    @translation_table.setter
    def translation_table(self, translation_table: int) -> None:
        import ctypes as C
        from . import _lib
        from .errors import InvalidParameter
        table = int(translation_table)
        desc = C.create_string_buffer(128)
        if not -2 ** 31 <= table < 2 ** 31 or _lib.lib().p7x_gencode_table(table, None, desc, 128, None) != 0:
            raise InvalidParameter("translation_table", translation_table, hint="translation table code")
        self._table, self._description = table, desc.value.decode("ascii")

    @property
    def description(self) -> str:
        return self._description

    def _tables(self):
        """``(aa64, lut)``: the 64 amino codes in NCBI order and the Kp^3 codon lookup the library translates with."""
        from . import _lib
        aa64, lut = np.empty(64, dtype=np.uint8), np.empty(18 ** 3, dtype=np.uint8)
        _lib.lib().p7x_gencode_table(self._table, aa64.ctypes.data, None, 0, lut.ctypes.data)
        return aa64, lut

    def translate(self, sequence) -> np.ndarray:
        """Translate a raw digital nucleotide sequence (any buffer of codes) in frame: a ``uint8`` array of amino codes
        (a numpy array where the reference returns a ``VectorU8``).  Degenerate codons whose expansions agree translate
        to what they give (``GGR`` -> ``G``), the others to ``X``; `ValueError` for a length that is no multiple of three
        and for a codon that holds a gap, ``*`` or ``~``."""
        import ctypes as C
        from . import _lib
        seq = np.ascontiguousarray(np.frombuffer(sequence, dtype=np.uint8) if not isinstance(sequence, np.ndarray) else sequence, dtype=np.uint8)
        if seq.shape[0] % 3 != 0:
            raise ValueError(f"Invalid sequence of length {seq.shape[0]!r}")
        out = np.empty(seq.shape[0] // 3, dtype=np.uint8)
        bad = C.c_int64(-1)
        if _lib.lib().p7x_translate_codons(self._table, seq.ctypes.data, seq.shape[0], out.ctypes.data, C.byref(bad)) != 0:
            raise ValueError(_lib.last_error())
        return out


class Sequence:
    """Abstract biological sequence with metadata (reference ``easel.pyx`` ``Sequence``)."""

    __slots__ = ("name", "description", "accession", "source")

    def __init__(self, name: str = "", description: str = "", accession: str = "", source: str = ""):
        self.name = name
        self.description = description
        self.accession = accession
        self.source = source


class TextSequence(Sequence):
    """A sequence stored as text (reference ``easel.pyx:7483``)."""

    __slots__ = ("sequence",)

    def __init__(self, name: str = "", description: str = "", accession: str = "",
                 sequence: str = "", source: str = ""):
        super().__init__(name, description, accession, source)
        self.sequence = sequence

    def __len__(self) -> int:
        return len(self.sequence)

    def digitize(self, alphabet: Alphabet) -> "DigitalSequence":
        return DigitalSequence(alphabet, name=self.name, description=self.description,
                               accession=self.accession, sequence=alphabet.encode(self.sequence),
                               source=self.source)

    def copy(self) -> "TextSequence":
        return TextSequence(self.name, self.description, self.accession, self.sequence, self.source)

    def reverse_complement(self, inplace: bool = False) -> Optional["TextSequence"]:
        """The reverse complement, IUPAC letters complemented with their case kept; any other letter becomes ``N``, with a
        `UserWarning` (reference ``easel.pyx:7688-7738``)."""
        import warnings
        raw = self.sequence.encode("ascii", "replace")[::-1]
        rc = raw.translate(_TEXT_COMPLEMENT)
        if 0 in rc:
            rc = rc.replace(b"\0", b"N")
            warnings.warn("reverse-complementing a text sequence with non-DNA characters", UserWarning, stacklevel=2)
        if inplace:
            self.sequence = rc.decode("ascii")
            return None
        out = self.copy()
        out.sequence = rc.decode("ascii")
        return out


class DigitalSequence(Sequence):
    """A sequence stored as digital residue codes 0..Kp-1 (reference ``easel.pyx:7741``)."""

    __slots__ = ("alphabet", "sequence")

    def __init__(self, alphabet: Alphabet, name: str = "", description: str = "", accession: str = "",
                 sequence=None, source: str = ""):
        super().__init__(name, description, accession, source)
        self.alphabet = alphabet
        seq = np.zeros(0, dtype=np.uint8) if sequence is None else np.ascontiguousarray(sequence, dtype=np.uint8)
        if seq.size and int(seq.max()) >= alphabet.Kp:
            raise ValueError("invalid digital code in sequence")
        self.sequence = seq

    def __len__(self) -> int:
        return int(self.sequence.shape[0])

    def textize(self) -> TextSequence:
        return TextSequence(self.name, self.description, self.accession,
                            self.alphabet.decode(self.sequence), self.source)

    def copy(self) -> "DigitalSequence":
        return DigitalSequence(self.alphabet, self.name, self.description, self.accession,
                               self.sequence.copy(), self.source)

    def translate(self, genetic_code: Optional["GeneticCode"] = None) -> "DigitalSequence":
        """Translate the whole sequence in frame (reference ``easel.pyx:7996-8068``); the metadata is carried over."""
        from .errors import AlphabetMismatch
        genetic_code = GeneticCode() if genetic_code is None else genetic_code
        if self.alphabet != genetic_code.nucleotide_alphabet:
            raise AlphabetMismatch(genetic_code.nucleotide_alphabet, self.alphabet)
        if len(self) % 3 != 0:
            raise ValueError(f"Incomplete sequence of length {len(self)!r}")
        return DigitalSequence(genetic_code.amino_alphabet, self.name, self.description, self.accession,
                               genetic_code.translate(self.sequence), self.source)

    def shuffle(self, seed: int = 42, mode: str = "mono", window: int = 0) -> "DigitalSequence":
        """A decoy of this sequence (an extension), shuffled on the host: what sequence 0 of
        ``DigitalSequenceBlock(alphabet, [self]).shuffle(seed, mode, window)`` is."""
        mode_code = _check_shuffle_arguments(seed, mode, window)
        pk = PackedBlock([self])
        dsq, _ = _shuffle_packed(self.alphabet, pk, mode_code, int(window), int(seed), host=True, threads=1)
        return DigitalSequence(self.alphabet, f"{self.name}-shuffled", self.description, self.accession, dsq[1:1 + len(self)], self.source)

    def reverse_complement(self, inplace: bool = False) -> Optional["DigitalSequence"]:
        """The reverse complement (reference ``easel.pyx:8070-8110``); `ValueError` for an alphabet without complements."""
        if not self.alphabet.is_nucleotide():
            raise ValueError(f"{self.alphabet} has no defined complement")
        rc = _NT_COMPLEMENT[self.sequence[::-1]]
        if inplace:
            self.sequence = rc
            return None
        out = self.copy()
        out.sequence = rc
        return out


class PackedBlock:
    """Flat, device-friendly image of a ``DigitalSequenceBlock``.

    ``dsq`` holds ``255 x1..xL 255 x1..xL 255 ...`` (Easel sentinels, ``plan7.pyx:7615-7616``);
    ``offsets[t]`` indexes ``x1`` of target ``t``; ``lengths[t]`` is ``L_t``.
    """

    __slots__ = ("dsq", "offsets", "lengths", "n", "total_residues", "_resident_token", "__weakref__")

    def __init__(self, seqs: _Seq[DigitalSequence]):
        n = len(seqs)
        lengths = np.fromiter((len(s) for s in seqs), dtype=np.int32, count=n)
        offsets = np.empty(n, dtype=np.int64)
        total = int(lengths.sum(dtype=np.int64))
        dsq = np.full(total + n + 1, DSQ_SENTINEL, dtype=np.uint8)
        pos = 1
        for t, s in enumerate(seqs):
            L = int(lengths[t])
            offsets[t] = pos
            dsq[pos:pos + L] = s.sequence
            pos += L + 1
        self.dsq, self.offsets, self.lengths = dsq, offsets, lengths
        self.n, self.total_residues = n, total

    @classmethod
    def from_arrays(cls, dsq: np.ndarray, offsets: np.ndarray, lengths: np.ndarray) -> "PackedBlock":
        self = cls.__new__(cls)
        self.dsq, self.offsets, self.lengths = dsq, offsets, lengths
        self.n, self.total_residues = int(lengths.shape[0]), int(lengths.sum(dtype=np.int64))
        return self


def _check_shuffle_arguments(seed, mode, window) -> int:
    """The argument checks of both ``shuffle`` methods; returns the mode of the C-ABI."""
    from .errors import InvalidParameter
    if mode not in _SHUFFLE_MODES:
        raise InvalidParameter("mode", mode, choices=list(_SHUFFLE_MODES))
    if int(window) < 0:
        raise InvalidParameter("window", window, hint="a number of residues, 0 or more")
    if mode == "window" and int(window) == 0:
        raise InvalidParameter("window", window, hint="mode 'window' needs a window of at least one residue")
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise InvalidParameter("seed", seed, hint="an integer from 0 to 2**32 - 1")
    return _SHUFFLE_MODES.index(mode)


def _shuffle_packed(alphabet: "Alphabet", pk: "PackedBlock", mode_code: int, window: int, seed: int, *, host: bool, device: int = 0,
                    threads: int = 0):
    """``p7x_shuffle_block`` / ``p7x_shuffle_host`` over a packed block: the shuffled ``dsq`` and the five statistics."""
    from . import _lib
    from .errors import status_to_exception
    dsq = np.empty(pk.dsq.shape[0], dtype=np.uint8)
    stats = np.zeros(5, dtype=np.int64)
    common = (pk.dsq.ctypes.data, pk.offsets.ctypes.data, pk.lengths.ctypes.data, pk.n, int(pk.dsq.shape[0]), mode_code, window, seed)
    if host:
        st, fn = _lib.lib().p7x_shuffle_host(alphabet.type_code, *common, int(threads), dsq.ctypes.data, stats.ctypes.data), "p7x_shuffle_host"
    else:
        st, fn = _lib.lib().p7x_shuffle_block(alphabet.type_code, int(device), *common, dsq.ctypes.data, stats.ctypes.data), "p7x_shuffle_block"
    if st != 0:
        raise status_to_exception(st, fn, _lib.last_error())
    return dsq, stats


class _SequenceBlock:
    __slots__ = ("_seqs", "_packed", "_version")

    def __init__(self, iterable: Iterable = ()):
        self._seqs: List = list(iterable)
        self._packed = None
        self._version = 0           # bumped by every mutation: caches of the packed / resident copy key on it

    def _touch(self) -> None:
        self._packed = None
        self._version += 1

    def __len__(self) -> int:
        return len(self._seqs)

    def __iter__(self) -> Iterator:
        return iter(self._seqs)

    def __getitem__(self, index):
        if isinstance(index, slice):
            return type(self)._from_list(self, self._seqs[index])
        return self._seqs[index]

    def __setitem__(self, index, value) -> None:
        self._seqs[index] = value
        self._touch()

    def __delitem__(self, index) -> None:
        del self._seqs[index]
        self._touch()

    def __contains__(self, item) -> bool:
        return item in self._seqs

    def append(self, seq) -> None:
        self._seqs.append(seq)
        self._touch()

    def extend(self, iterable) -> None:
        self._seqs.extend(iterable)
        self._touch()

    def insert(self, index: int, seq) -> None:
        self._seqs.insert(index, seq)
        self._touch()

    def pop(self, index: int = -1):
        seq = self._seqs.pop(index)
        self._touch()
        return seq

    def remove(self, seq) -> None:
        self._seqs.remove(seq)
        self._touch()

    def index(self, seq, start: int = 0, stop: Optional[int] = None) -> int:
        return self._seqs.index(seq, start, len(self._seqs) if stop is None else stop)

    def clear(self) -> None:
        self._seqs.clear()
        self._touch()

    def largest(self):
        if not self._seqs:
            raise ValueError("block is empty")
        return max(self._seqs, key=len)

    def total_length(self) -> int:
        return sum(len(s) for s in self._seqs)


class TextSequenceBlock(_SequenceBlock):
    """Reference ``easel.pyx:8501``."""

    @staticmethod
    def _from_list(parent, lst):
        return TextSequenceBlock(lst)

    def digitize(self, alphabet: Alphabet) -> "DigitalSequenceBlock":
        return DigitalSequenceBlock(alphabet, (s.digitize(alphabet) for s in self._seqs))


class DigitalSequenceBlock(_SequenceBlock):
    """A list of digital sequences searched as one batch (reference ``easel.pyx:8629-8665``)."""

    __slots__ = ("alphabet",)

    def __init__(self, alphabet: Alphabet, iterable: Iterable = ()):
        super().__init__(iterable)
        self.alphabet = alphabet
        for s in self._seqs:
            if not isinstance(s, DigitalSequence):
                raise TypeError(f"expected DigitalSequence, found {type(s).__name__}")
            if s.alphabet != alphabet:
                raise ValueError("alphabet mismatch in DigitalSequenceBlock")

    @staticmethod
    def _from_list(parent, lst):
        return DigitalSequenceBlock(parent.alphabet, lst)

    def copy(self) -> "DigitalSequenceBlock":
        return DigitalSequenceBlock(self.alphabet, (s.copy() for s in self._seqs))

    def packed(self) -> PackedBlock:
        """Pack once into the flat arrays of the C-ABI (cached until the block is mutated)."""
        if self._packed is None or self._packed.n != len(self._seqs):
            self._packed = PackedBlock(self._seqs)
        return self._packed

    def _check_translatable(self, genetic_code: "GeneticCode") -> None:
        from .errors import AlphabetMismatch
        if self.alphabet != genetic_code.nucleotide_alphabet:
            raise AlphabetMismatch(genetic_code.nucleotide_alphabet, self.alphabet)

    def translate(self, genetic_code: Optional["GeneticCode"] = None, device: int = 0) -> "DigitalSequenceBlock":
        """Translate every sequence whole and in frame, stops kept as ``*`` (reference ``easel.pyx:8765``), the whole block
        at once on ``device`` (``p7x_translate.hip``; test seam ``host_translate``: the host twin).  Names, descriptions,
        accessions and sources are carried over.  `ValueError` for a sequence whose length is no multiple of three or
        that holds a codon with a gap, ``*`` or ``~``."""
        import ctypes as C
        from . import _lib
        from .errors import status_to_exception
        genetic_code = GeneticCode() if genetic_code is None else genetic_code
        self._check_translatable(genetic_code)
        pk = self.packed()
        if pk.n == 0:
            return DigitalSequenceBlock(genetic_code.amino_alphabet)
        bad = np.flatnonzero(pk.lengths % 3)
        if bad.size:
            raise ValueError(f"Incomplete sequence of length {int(pk.lengths[bad[0]])!r} at index {int(bad[0])!r}")
        dsq = np.empty(pk.total_residues // 3 + pk.n + 1, dtype=np.uint8)
        offsets, lengths = np.empty(pk.n, dtype=np.int64), np.empty(pk.n, dtype=np.int32)
        eseq, epos = C.c_int64(-1), C.c_int64(-1)
        st = _lib.lib().p7x_translate_block(genetic_code.translation_table, int(device), pk.dsq.ctypes.data, pk.offsets.ctypes.data,
                                            pk.lengths.ctypes.data, pk.n, pk.total_residues, dsq.ctypes.data, offsets.ctypes.data,
                                            lengths.ctypes.data, C.byref(eseq), C.byref(epos))
        if st == 11 and eseq.value >= 0:
            raise ValueError(f"Failed to translate codon at index {epos.value!r} of the sequence at index {eseq.value!r}")
        if st != 0:
            raise status_to_exception(st, "p7x_translate_block", _lib.last_error())
        abc = genetic_code.amino_alphabet
        return DigitalSequenceBlock(abc, (DigitalSequence(abc, s.name, s.description, s.accession, dsq[o:o + L], s.source)
                                          for s, o, L in zip(self, offsets.tolist(), lengths.tolist())))

    def translate_orfs(self, genetic_code: Optional["GeneticCode"] = None, *, min_length: int = 20, strand: Optional[str] = None,
                       device: int = 0) -> "TranslatedBlock":
        """The open reading frames of the block (an extension): every maximal run of at least
        ``min_length`` codons without a stop, in the three frames of both strands (``strand``: `None`, ``"watson"`` or
        ``"crick"``), found on ``device`` for the whole block at once.  No start codon is asked for.  The result is an
        amino `TranslatedBlock` for `hmmsearch` / `hmmscan` / `phmmer` / `hmmalign`, ordered by source sequence, watson
        before crick, then by the first base along the translated strand."""
        import ctypes as C
        from . import _lib
        from .errors import InvalidParameter, status_to_exception
        genetic_code = GeneticCode() if genetic_code is None else genetic_code
        self._check_translatable(genetic_code)
        if strand not in _STRANDS:
            raise InvalidParameter("strand", strand, choices=["watson", "crick", None])
        if int(min_length) < 1:
            raise InvalidParameter("min_length", min_length, hint="at least one codon")
        pk = self.packed()
        h = C.c_void_p()
        st = _lib.lib().p7x_orfs_find(genetic_code.translation_table, int(device), pk.dsq.ctypes.data, pk.offsets.ctypes.data,
                                      pk.lengths.ctypes.data, pk.n, pk.total_residues, int(min_length), _STRANDS[strand], C.byref(h))
        if st != 0:
            raise status_to_exception(st, "p7x_orfs_find", _lib.last_error())
        try:
            return TranslatedBlock(genetic_code.amino_alphabet, self, h)
        finally:
            _lib.lib().p7x_orfs_destroy(h)

    def shuffle(self, seed: int = 42, mode: str = "mono", window: int = 0, device: int = 0) -> "ShuffledBlock":
        """A decoy of every sequence (an extension): the same lengths and the same residues with the
        homology destroyed, the whole block at once on ``device`` (``p7x_shuffle.hip``; test seam ``host_shuffle``: the host
        twin, the same bytes).  ``mode``: ``"mono"`` a uniform permutation; ``"di"`` a uniform draw among the sequences
        with the same first residue, last residue and count of every adjacent pair (Altschul & Erickson 1985; fewer than
        three residues stay as they are); ``"window"`` a permutation within consecutive windows of ``window`` residues;
        ``"reverse"`` the sequence backwards.  Every digital code is a symbol like any other.  Decoy ``i`` depends on
        sequence ``i``, its index and ``seed`` (0 to 2**32 - 1; 0 is a seed like any other) only, so ``block[:k].shuffle(...)``
        gives the first ``k`` decoys of ``block.shuffle(...)``."""
        mode_code = _check_shuffle_arguments(seed, mode, window)
        dsq, stats = _shuffle_packed(self.alphabet, self.packed(), mode_code, int(window), int(seed), host=False, device=device)
        return ShuffledBlock(self, dsq, stats, mode, int(seed), int(window))


class _LazyDigitalSequenceBlock(DigitalSequenceBlock):
    """A block that exists only as the packed arrays the native FASTA parser produced (``p7x_fasta_parse``): a
    million-record file becomes a searchable block without a million Python objects.  ``DigitalSequence`` objects are
    built on demand (indexing) or all at once when the block is iterated or mutated."""

    __slots__ = ("_list", "_pk", "_strtab", "_name_off", "_desc_off")

    def __init__(self, alphabet: Alphabet, pk: PackedBlock, strtab: np.ndarray, name_off: np.ndarray, desc_off: np.ndarray):
        self._list = None
        self._pk, self._strtab, self._name_off, self._desc_off = pk, strtab, name_off, desc_off
        self.alphabet = alphabet
        self._packed = pk
        self._version = 0

    def _cstr(self, off: int) -> str:
        buf = self._strtab
        end = off
        n = buf.shape[0]
        while end < n and buf[end] != 0:
            end += 1
        return bytes(buf[off:end]).decode("utf-8", "replace")

    def _make(self, t: int) -> DigitalSequence:
        pk = self._pk
        o, L = int(pk.offsets[t]), int(pk.lengths[t])
        return DigitalSequence(self.alphabet, name=self._cstr(int(self._name_off[t])),
                               description=self._cstr(int(self._desc_off[t])), sequence=pk.dsq[o:o + L])

    @property
    def _seqs(self):
        if self._list is None:
            self._list = [self._make(t) for t in range(self._pk.n)]
        return self._list

    @_seqs.setter
    def _seqs(self, value):
        self._list = value

    def __len__(self) -> int:
        return self._pk.n if self._list is None else len(self._list)

    def __getitem__(self, index):
        if self._list is None and not isinstance(index, slice):
            n = self._pk.n
            i = index + n if index < 0 else index
            if not 0 <= i < n:
                raise IndexError("block index out of range")
            return self._make(i)
        return super().__getitem__(index)

    def total_length(self) -> int:
        return self._pk.total_residues if self._list is None else super().total_length()

    def packed(self) -> PackedBlock:
        return self._pk if self._list is None else super().packed()


def _string_table_of(names, descs):
    """Names and descriptions (bytes, one of each per sequence) as the NUL-terminated string table of a packed-only block and
    the offsets of the names and of the descriptions into it."""
    n = len(names)
    sizes = np.fromiter((len(b) + 1 for pair in zip(names, descs) for b in pair), dtype=np.int64, count=2 * n)
    at = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(sizes, out=at[1:])
    strtab = np.frombuffer(b"".join(b + b"\0" for pair in zip(names, descs) for b in pair) + b"\0", dtype=np.uint8)
    return strtab, at[0:2 * n:2].copy(), at[1:2 * n:2].copy()


class TranslatedBlock(_LazyDigitalSequenceBlock):
    """What `DigitalSequenceBlock.translate_orfs` returns: an amino block kept as packed arrays, and where every ORF
    came from.  ``source_index`` (the sequence of the source block), ``frame`` (int8: 1..3 watson, -1..-3 crick), ``start``
    and ``end`` (int64, in the source's own numbering from 1; ``start > end`` on crick) are numpy arrays with one entry per
    ORF.  ORF ``n`` (from 1) is the `DigitalSequence` ``orf{n}``, made on demand, with the description
    ``source={name} coords={start}..{end} length={aa} frame={frame}`` and ``source`` the source sequence's name; the name
    and description tables a search reads are built when first asked for."""

    __slots__ = ("source_block", "source_index", "frame", "start", "end", "on_device", "chunks", "orf_chunk", "kernel_us",
                 "pass_us", "stitch_us", "_tables")

    def __init__(self, alphabet: Alphabet, source: DigitalSequenceBlock, handle):
        from . import _lib
        from .errors import status_to_exception
        lib = _lib.lib()
        n, nres = int(lib.p7x_orfs_info(handle, 0)), int(lib.p7x_orfs_info(handle, 1))
        self.chunks, self.kernel_us = int(lib.p7x_orfs_info(handle, 2)), int(lib.p7x_orfs_info(handle, 3))
        self.on_device, self.orf_chunk = bool(lib.p7x_orfs_info(handle, 4)), int(lib.p7x_orfs_info(handle, 5))
        self.pass_us = tuple(int(lib.p7x_orfs_info(handle, k)) for k in (6, 7, 8, 9))
        self.stitch_us = int(lib.p7x_orfs_info(handle, 10))
        dsq = np.empty(nres + n + 1, dtype=np.uint8)
        offsets, lengths = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32)
        self.source_index, self.frame = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int8)
        self.start, self.end = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        st = lib.p7x_orfs_copy(handle, dsq.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, self.source_index.ctypes.data,
                               self.frame.ctypes.data, self.start.ctypes.data, self.end.ctypes.data)
        if st != 0:
            raise status_to_exception(st, "p7x_orfs_copy", _lib.last_error())
        self.source_block = source
        self._tables = None
        self._list = None
        self._pk = PackedBlock.from_arrays(dsq, offsets, lengths)
        self.alphabet = alphabet
        self._packed = self._pk
        self._version = 0

    def _source_name(self, i: int) -> str:
        return self.source_block[int(self.source_index[i])].name

    def _description(self, i: int) -> str:
        return (f"source={self._source_name(i)} coords={int(self.start[i])}..{int(self.end[i])} "
                f"length={int(self._pk.lengths[i])} frame={int(self.frame[i])}")

    def _make(self, t: int) -> DigitalSequence:
        o, L = int(self._pk.offsets[t]), int(self._pk.lengths[t])
        return DigitalSequence(self.alphabet, name=f"orf{t + 1}", description=self._description(t), sequence=self._pk.dsq[o:o + L],
                               source=self._source_name(t))

    def _string_tables(self):
        """The NUL-terminated string table of names and descriptions and the offsets into it, as the native FASTA parser
        lays them out (`SequenceDatabase` hands pointers into it to the library)."""
        if self._tables is None:
            n = self._pk.n
            names = [f"orf{i + 1}".encode() for i in range(n)]
            src = [s.name for s in self.source_block]
            descs = [f"source={src[k]} coords={a}..{b} length={L} frame={f}".encode()
                     for k, a, b, L, f in zip(self.source_index.tolist(), self.start.tolist(), self.end.tolist(),
                                              self._pk.lengths.tolist(), self.frame.tolist())]
            self._tables = _string_table_of(names, descs)
        return self._tables

    _strtab = property(lambda self: self._string_tables()[0])
    _name_off = property(lambda self: self._string_tables()[1])
    _desc_off = property(lambda self: self._string_tables()[2])

    def locate(self, x):
        """Where a `Domain` (or the best domain of a `Hit`) of a search against this block lies on its source sequence:
        ``(source_name, source_index, nt_from, nt_to, frame)``, nucleotides in the source's own numbering, ``nt_from >
        nt_to`` on crick.  The ORF is found from the hit's name."""
        dom = x.best_domain if hasattr(x, "best_domain") else x
        name = dom.hit.name
        if not name.startswith("orf") or not name[3:].isdigit() or not 1 <= int(name[3:]) <= self._pk.n:
            raise ValueError(f"{name!r} is not an ORF of this block")
        t = int(name[3:]) - 1
        i, j = int(dom.alignment.target_from), int(dom.alignment.target_to)
        start, frame = int(self.start[t]), int(self.frame[t])
        if frame > 0:
            nt = (start + 3 * (i - 1), start + 3 * j - 1)
        else:
            nt = (start - 3 * (i - 1), start - 3 * j + 1)
        k = int(self.source_index[t])
        return (self.source_block[k].name, k, nt[0], nt[1], frame)


def _block_strings(block: DigitalSequenceBlock):
    """The names and descriptions (bytes) of a block, without making the sequences of one that is kept packed."""
    if getattr(block, "_list", 0) is None:
        buf = block._strtab.tobytes()
        cut = lambda offs: [buf[o:buf.index(b"\0", o)] for o in offs.tolist()]
        return cut(block._name_off), cut(block._desc_off)
    return [s.name.encode() for s in block], [(s.description or "").encode() for s in block]


class ShuffledBlock(_LazyDigitalSequenceBlock):
    """What `DigitalSequenceBlock.shuffle` returns: the decoys of ``source_block``, kept as packed arrays with the offsets and
    lengths of the source's packed block.  Decoy ``i`` is the `DigitalSequence` ``{source name}-shuffled`` with the source's
    description, accession and source, made on demand; the name and description tables a search reads are built when
    first asked for.  ``mode``, ``seed`` and ``window`` are the arguments; ``on_device`` tells whether the kernels made the
    block (or the host twin), ``kernel_us`` their time from device events, ``long_sequences`` how many sequences were too long
    for a workgroup's slab and took the second launch, ``runs`` the workgroups of the first."""

    __slots__ = ("source_block", "mode", "seed", "window", "on_device", "kernel_us", "upload_us", "runs", "long_sequences", "_tables")

    def __init__(self, source: DigitalSequenceBlock, dsq: np.ndarray, stats, mode: str, seed: int, window: int):
        pk = source.packed()
        self.source_block, self.mode, self.seed, self.window = source, mode, seed, window
        self.kernel_us, self.upload_us = int(stats[0]) // 1000, int(stats[1]) // 1000
        self.runs, self.long_sequences, self.on_device = int(stats[2]), int(stats[3]), bool(stats[4])
        self._tables = None
        self._list = None
        self._pk = PackedBlock.from_arrays(dsq, pk.offsets, pk.lengths)
        self.alphabet = source.alphabet
        self._packed = self._pk
        self._version = 0

    def _make(self, t: int) -> DigitalSequence:
        src = self.source_block[t]
        o, L = int(self._pk.offsets[t]), int(self._pk.lengths[t])
        return DigitalSequence(self.alphabet, name=f"{src.name}-shuffled", description=src.description, accession=src.accession,
                               sequence=self._pk.dsq[o:o + L], source=src.source)

    def _string_tables(self):
        """The NUL-terminated string table of names and descriptions and the offsets into it, as the native FASTA parser
        lays them out (`SequenceDatabase` hands pointers into it to the library)."""
        if self._tables is None:
            names, descs = _block_strings(self.source_block)
            names = [b + b"-shuffled" for b in names]
            self._tables = _string_table_of(names, descs)
        return self._tables

    _strtab = property(lambda self: self._string_tables()[0])
    _name_off = property(lambda self: self._string_tables()[1])
    _desc_off = property(lambda self: self._string_tables()[2])


class SequenceFile:
    """Sequence reader with the reference's ``SequenceFile`` surface (``read``, ``read_block``, iteration, context
    manager).  FASTA, and the sequence records of GenBank flat files (LOCUS / DEFINITION / VERSION / ORIGIN: what the
    reference's nhmmer fixtures need); the format is recognised from the first line when it is not given."""

    def __init__(self, file, format: Optional[str] = None, *, digital: bool = False,
                 alphabet: Optional[Alphabet] = None):
        if format not in (None, "fasta", "afa", "genbank"):
            raise ValueError(f"unsupported sequence format: {format!r}")
        if isinstance(file, (str, bytes, os.PathLike)):
            self._fh = open(file, "r")
            self._own = True
            self.name = os.fspath(file)
        else:
            self._fh = file
            self._own = False
            self.name = getattr(file, "name", None)
        self.digital = digital
        self.alphabet = alphabet
        self._pending: Optional[str] = None
        self._touched = False
        self._chunk_pos = 0
        self._chunking = False                                # read_chunk() is walking the file
        if format is None:
            try:
                pos = self._fh.tell()
                first = self._fh.readline()
                self._fh.seek(pos)
                format = "genbank" if first.startswith("LOCUS") else "fasta"
            except (OSError, ValueError):
                format = "fasta"
        self.format = format
        if digital and alphabet is None:
            self.alphabet = self.guess_alphabet()
            if self.alphabet is None:
                raise ValueError("Could not determine alphabet of file")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self) -> None:
        if self._own:
            self._fh.close()

    def rewind(self) -> None:
        self._fh.seek(0)
        self._pending = None
        self._touched = False
        self._chunk_pos = 0
        self._chunking = False

    def guess_alphabet(self) -> Optional[Alphabet]:
        pos = self._fh.tell()
        counts = np.zeros(256, dtype=np.int64)
        n = 0
        in_origin = self.format != "genbank"
        for line in self._fh:
            if line.startswith(">"):
                continue
            if self.format == "genbank":
                if line.startswith("ORIGIN"):
                    in_origin = True
                    continue
                if line.startswith("//"):
                    in_origin = False
                if not in_origin:
                    continue
                line = "".join(c for c in line if c.isalpha())
            raw = np.frombuffer(line.strip().upper().encode("ascii", "ignore"), dtype=np.uint8)
            counts += np.bincount(raw, minlength=256)
            n += raw.size
            if n > 4000:
                break
        self._fh.seek(pos)
        if n == 0:
            return None
        nuc = sum(int(counts[ord(c)]) for c in "ACGTUN")
        return Alphabet.dna() if nuc >= 0.9 * n else Alphabet.amino()

    def _read_genbank(self) -> Optional[TextSequence]:
        """One record of a GenBank flat file: name from LOCUS, accession from VERSION (else ACCESSION), description from
        DEFINITION (continuation lines joined), residues from ORIGIN .. //."""
        name = acc = ""
        desc: list = []
        chunks: list = []
        state = None
        seen = False
        for line in self._fh:
            if line.startswith("//"):
                if seen:
                    break
                continue
            key = line[:12].strip()
            if key == "LOCUS":
                name = line.split()[1]
                seen = True
                state = None
            elif key == "DEFINITION":
                desc = [line[12:].strip()]
                state = "def"
            elif key == "VERSION":
                parts = line.split()
                acc = parts[1] if len(parts) > 1 else acc
                state = None
            elif key == "ACCESSION":
                parts = line.split()
                acc = acc or (parts[1] if len(parts) > 1 else "")
                state = None
            elif key == "ORIGIN":
                state = "seq"
            elif state == "seq":
                chunks.append("".join(c for c in line if c.isalpha()))
            elif state == "def" and line.startswith(" "):
                desc.append(line.strip())
            elif key:
                state = None
        if not seen:
            return None
        return TextSequence(name=name, description=" ".join(desc), accession=acc, sequence="".join(chunks))

    def _read_text(self) -> Optional[TextSequence]:
        self._touched = True
        if self.format == "genbank":
            return self._read_genbank()
        header = self._pending
        self._pending = None
        if header is None:
            for line in self._fh:
                if line.startswith(">"):
                    header = line
                    break
            if header is None:
                return None
        chunks = []
        for line in self._fh:
            if line.startswith(">"):
                self._pending = line
                break
            chunks.append(line.strip())
        head = header[1:].rstrip("\r\n")
        parts = head.split(None, 1)
        name = parts[0] if parts else ""
        desc = parts[1].strip() if len(parts) > 1 else ""
        seq = "".join(chunks).replace(" ", "")
        return TextSequence(name=name, description=desc, sequence=seq)

    def read(self):
        s = self._read_text()
        if s is None:
            return None
        return s.digitize(self.alphabet) if self.digital else s

    def __iter__(self):
        return self

    def __next__(self):
        s = self.read()
        if s is None:
            raise StopIteration
        return s

    def _read_block_native(self) -> "DigitalSequenceBlock":
        """Whole file -> packed block through the C parser (no per-record Python work)."""
        block = self._parse_native(np.fromfile(self.name, dtype=np.uint8))
        self._touched = True
        self._fh.seek(0, 2)                                   # the file is consumed
        return block

    def read_chunk(self, max_bytes: int = 1 << 28) -> "DigitalSequenceBlock":
        """The next whole records of a digital FASTA file, about ``max_bytes`` of text at a time, through the C parser:
        how ``hmmsearch`` walks a target database that is larger than memory (the reference iterates the file, one
        sequence at a time: ``plan7.pyx:6244-6252``, ``_search_loop_file`` ``:6456``).  An empty block at the end of the
        file; ``rewind()`` starts over.  Other formats and text mode fall back to ``read_block(residues=max_bytes)``."""
        if not (self.digital and self._own and self.format != "genbank"):
            return self.read_block(residues=max_bytes)
        if self._touched and not self._chunking:
            raise ValueError("read_chunk() cannot continue a file that was partly read record by record; rewind() first")
        with open(self.name, "rb") as f:
            f.seek(self._chunk_pos)
            data = f.read(max_bytes)
            if len(data) == max_bytes:                        # most likely inside a record: take the rest of it
                tail = data[-1:]
                while True:
                    more = f.read(1 << 20)
                    if not more:
                        break
                    k = (tail + more).find(b"\n>")
                    if k >= 0:
                        data += more[:k]                      # up to and including the newline before the next header
                        break
                    data += more
                    tail = more[-1:]
        self._chunk_pos += len(data)
        self._touched = True
        self._chunking = True
        self._fh.seek(self._chunk_pos)                        # record-by-record reads continue where the chunks ended
        self._pending = None
        if not data.strip():
            return DigitalSequenceBlock(self.alphabet, [])
        return self._parse_native(np.frombuffer(data, dtype=np.uint8))

    def _parse_native(self, data: np.ndarray) -> "DigitalSequenceBlock":
        import ctypes as C
        from . import _lib
        lut = self.alphabet._lut.copy()
        for ch in b" \t\r\n0123456789":
            lut[ch] = 254                                     # ignored inside sequence data, as Easel's sqio does
        ns, nr, sb, bad = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        fn = _lib.lib().p7x_fasta_parse
        st = fn(data.ctypes.data, data.shape[0], lut.ctypes.data, C.byref(ns), C.byref(nr), C.byref(sb), None, None, None,
                None, None, None, C.byref(bad))
        if st == 0:
            dsq = np.empty(nr.value + ns.value + 1, dtype=np.uint8)
            offsets, lengths = np.empty(ns.value, dtype=np.int64), np.empty(ns.value, dtype=np.int32)
            strtab = np.empty(max(sb.value, 1), dtype=np.uint8)
            name_off, desc_off = np.empty(ns.value, dtype=np.int64), np.empty(ns.value, dtype=np.int64)
            st = fn(data.ctypes.data, data.shape[0], lut.ctypes.data, C.byref(ns), C.byref(nr), C.byref(sb), dsq.ctypes.data,
                    offsets.ctypes.data, lengths.ctypes.data, strtab.ctypes.data, name_off.ctypes.data, desc_off.ctypes.data,
                    C.byref(bad))
        if st != 0:
            raise ValueError(f"{self.name}: {_lib.last_error()} (byte {bad.value})")
        return _LazyDigitalSequenceBlock(self.alphabet, PackedBlock.from_arrays(dsq, offsets, lengths), strtab, name_off, desc_off)

    def read_block(self, sequences: Optional[int] = None, residues: Optional[int] = None):
        if self.digital and self._own and not self._touched and sequences is None and residues is None and self.format != "genbank":
            return self._read_block_native()
        out = []
        nres = 0
        while True:
            if sequences is not None and len(out) >= sequences:
                break
            if residues is not None and nres >= residues:
                break
            s = self.read()
            if s is None:
                break
            out.append(s)
            nres += len(s)
        if self.digital:
            return DigitalSequenceBlock(self.alphabet, out)
        return TextSequenceBlock(out)


class MSA:
    """A multiple sequence alignment (reference ``easel.pyx`` ``MSA`` / ``TextMSA`` / ``DigitalMSA``; ``ESL_MSA``).

    Rows are kept as text: residues, ``-`` for deletions and ``.`` for gaps in insert columns, inserts in lower case (as
    hmmalign builds them).  Optional per-column / per-row annotation: ``posterior_probabilities`` (``#=GR PP``),
    ``pp_consensus`` (``#=GC PP_cons``), ``reference`` (``#=GC RF``), ``secondary_structure`` (``#=GC SS_cons``).
    """

    def __init__(self, name: Optional[str] = None, description: Optional[str] = None, accession: Optional[str] = None,
                 sequences: Optional[Iterable] = None):
        self.name, self.description, self.accession = name, description, accession
        self.author: Optional[str] = None               # ``#=GF AU``: the program that made the alignment
        self._names: List[str] = []
        self._rows: List[str] = []
        self._descs: List[str] = []
        self._accs: List[str] = []
        self.posterior_probabilities: Optional[List[str]] = None
        self.pp_consensus: Optional[str] = None
        self.reference: Optional[str] = None
        self.secondary_structure: Optional[str] = None
        self._weights: Optional[np.ndarray] = None      # None: the default weights (Easel's eslMSA_HASWGTS unset)
        for seq in sequences or ():
            self._add(seq)

    def _add(self, seq) -> None:
        row = seq.sequence if isinstance(seq, TextSequence) else seq.alphabet.decode(seq.sequence)
        if self._rows and len(row) != len(self._rows[0]):
            raise ValueError("all the sequences of an alignment must have the same length")
        if seq.name in self._names:
            raise ValueError(f"duplicate sequence name {seq.name!r}")
        self._names.append(seq.name)
        self._rows.append(row)
        self._descs.append(seq.description or "")
        self._accs.append(seq.accession or "")

    @classmethod
    def _from_rows(cls, names, rows, descs, accs, pp=None, pp_cons=None, rf=None, ss_cons=None, alphabet=None):
        self = cls.__new__(cls)
        MSA.__init__(self)
        if alphabet is not None:
            self.alphabet = alphabet
        self._names, self._rows, self._descs, self._accs = list(names), list(rows), list(descs), list(accs)
        self.posterior_probabilities, self.pp_consensus, self.reference, self.secondary_structure = pp, pp_cons, rf, ss_cons
        return self

    def __len__(self) -> int:
        """The alignment length (number of columns), as ``len(MSA)`` in the reference."""
        return len(self._rows[0]) if self._rows else 0

    def __eq__(self, other) -> bool:
        if not isinstance(other, MSA) or type(self) is not type(other):
            return NotImplemented
        return (self._names == other._names and self._rows == other._rows and self._descs == other._descs
                and self._accs == other._accs and self.posterior_probabilities == other.posterior_probabilities
                and self.pp_consensus == other.pp_consensus and self.reference == other.reference
                and self.secondary_structure == other.secondary_structure
                and getattr(self, "alphabet", None) == getattr(other, "alphabet", None))

    def __repr__(self) -> str:
        return f"<{type(self).__name__} nseq={len(self._rows)} alen={len(self)}>"

    @property
    def names(self) -> tuple:
        return tuple(self._names)

    @property
    def alignment(self) -> tuple:
        return tuple(self._rows)

    # ---- sequence weights, fragments, subsets (reference easel.pyx:5135-5196, 5274, 5324)
    @property
    def sequence_weights(self) -> np.ndarray:
        """The weights of the rows (float64, one per row; a numpy array where the reference returns a ``VectorD``): ones
        by default.  Set them through the property, which checks that there is one per row and that they sum to the
        number of rows within 1e-3; ``del msa.sequence_weights`` goes back to the default."""
        if self._weights is None:
            return np.ones(len(self._rows), dtype=np.float64)
        return self._weights

    @sequence_weights.setter
    def sequence_weights(self, weights) -> None:
        if weights is None:
            raise TypeError("weights must not be None")
        w = np.array(weights, dtype=np.float64)
        n = len(self._rows)
        if w.ndim != 1 or w.shape[0] != n:
            raise ValueError(f"dimension mismatch: expected {n}, found {w.shape[0] if w.ndim == 1 else w.shape}")
        s = float(w.sum())
        if not abs(s - n) <= 0.001:
            raise ValueError(f"weights must sum to {n}, got {s} instead")
        self._weights = w

    @sequence_weights.deleter
    def sequence_weights(self) -> None:
        self._weights = None

    def _residue_mask(self) -> np.ndarray:
        """``(N, L)`` bool: the cells that hold a residue.  In a text alignment every alphanumeric character is one."""
        n, alen = len(self._rows), len(self)
        raw = np.frombuffer("".join(self._rows).encode("ascii"), dtype=np.uint8).reshape(n, alen)
        return ((raw >= 48) & (raw <= 57)) | ((raw >= 65) & (raw <= 90)) | ((raw >= 97) & (raw <= 122))

    def _spans(self):
        """Per row: whether it has a residue, the columns of its first and last one."""
        res = self._residue_mask()
        alen = res.shape[1]
        has = res.any(axis=1) if alen else np.zeros(res.shape[0], dtype=bool)
        first = res.argmax(axis=1) if alen else np.zeros(res.shape[0], dtype=np.int64)
        last = alen - 1 - res[:, ::-1].argmax(axis=1) if alen else np.zeros(res.shape[0], dtype=np.int64)
        return res, has, first, last

    def mark_fragments(self, threshold: float) -> np.ndarray:
        """Which rows are fragments (a bool array where the reference returns a ``Bitfield``): those whose span, first to
        last residue, is less than ``threshold`` (taken as a C ``float``, as in the reference) of the columns.  A row
        without residues is not one (the rule of ``Builder.build_msa``).  Host code."""
        from .errors import InvalidParameter
        if not 0.0 <= threshold <= 1.0:
            raise InvalidParameter("threshold", threshold, hint="real number between 0 and 1")
        n, alen = len(self._rows), len(self)
        if n == 0 or alen == 0:
            return np.zeros(n, dtype=bool)
        _, has, first, last = self._spans()
        return has & ((last - first + 1).astype(np.float64) / float(alen) < float(np.float32(threshold)))

    def select(self, sequences=None, columns=None) -> "MSA":
        """A copy holding a subset of the rows and / or columns, by index, in the alignment's own order (the indices make
        a mask, as in the reference); per-row and per-column annotation follows.  `IndexError` for an index out of bounds."""
        import operator

        def mask(indices, n):
            m = np.zeros(n, dtype=bool)
            for i in indices:
                i = operator.index(i)
                if not 0 <= i < n:
                    raise IndexError(i)
                m[i] = True
            return np.flatnonzero(m)

        n, alen = len(self._rows), len(self)
        rows = np.arange(n) if sequences is None else mask(sequences, n)
        cols = None if columns is None else mask(columns, alen)
        cut = (lambda s: s) if cols is None else (
            lambda s: s if not s else np.frombuffer(s.encode("ascii"), dtype=np.uint8)[cols].tobytes().decode("ascii"))    # "": a row without a PP line
        pp = self.posterior_probabilities
        out = type(self)._from_rows([self._names[i] for i in rows], [cut(self._rows[i]) for i in rows],
                                    [self._descs[i] for i in rows], [self._accs[i] for i in rows],
                                    None if pp is None else [cut(pp[i]) for i in rows], cut(self.pp_consensus), cut(self.reference),
                                    cut(self.secondary_structure), alphabet=getattr(self, "alphabet", None))
        out.name, out.description, out.accession, out.author = self.name, self.description, self.accession, self.author
        if self._weights is not None:
            out._weights = self._weights[rows].copy()
        return out

    def write(self, fh, format: str = "stockholm") -> None:
        """Write the alignment to a file object (binary or text) in Stockholm format, as Easel's writer prints it."""
        if format != "stockholm":
            raise ValueError(f"unsupported MSA format: {format!r} (only 'stockholm')")
        fh.write(self._stockholm() if isinstance(fh, io.TextIOBase) else self._stockholm().encode())

    def _stockholm(self) -> str:
        import ctypes as C
        from . import _lib
        n = len(self._rows)
        arr = lambda xs: (C.c_char_p * max(n, 1))(*[x.encode() if x else None for x in xs])
        names, rows = arr(self._names), arr(self._rows)
        accs, descs = arr(self._accs), arr(self._descs)
        pps = arr(self.posterior_probabilities) if self.posterior_probabilities is not None else None
        enc = lambda x: x.encode() if x else None
        args = (n, len(self), names, accs, descs, rows, pps, enc(self.secondary_structure), enc(self.pp_consensus),
                enc(self.reference))
        fn = _lib.lib().p7x_msa_write_stockholm
        size = fn(*args, None, 0)
        if size < 0:
            raise ValueError(_lib.last_error())
        buf = C.create_string_buffer(int(size) + 1)
        fn(*args, buf, size + 1)
        text = buf.raw[:size].decode()
        # the per-file annotation of a named alignment (`TopHits.to_msa`), where Easel's writer puts it: after the header
        gf = "".join(f"#=GF {tag} {v}\n" for tag, v in (("ID", self.name), ("AC", self.accession), ("DE", self.description), ("AU", self.author)) if v)
        head, sep, rest = text.partition("\n")
        return head + sep + gf + rest


class TextMSA(MSA):
    """An alignment of text sequences (reference ``easel.pyx`` ``TextMSA``)."""

    @property
    def sequences(self) -> List[TextSequence]:
        return [TextSequence(name=nm, description=d, accession=a, sequence=r)
                for nm, r, d, a in zip(self._names, self._rows, self._descs, self._accs)]

    def digitize(self, alphabet: Alphabet) -> "DigitalMSA":
        out = DigitalMSA._from_rows(self._names, self._rows, self._descs, self._accs, self.posterior_probabilities,
                                    self.pp_consensus, self.reference, self.secondary_structure, alphabet=alphabet)
        out._weights = None if self._weights is None else self._weights.copy()
        return out


class DigitalMSA(MSA):
    """An alignment of digital sequences (reference ``easel.pyx`` ``DigitalMSA``).  Gap characters are digitised to
    the alphabet's gap code; ``alignment`` gives the rows as text, as the reference textizes them."""

    def __init__(self, alphabet: Alphabet, name: Optional[str] = None, description: Optional[str] = None,
                 accession: Optional[str] = None, sequences: Optional[Iterable] = None):
        self.alphabet = alphabet
        super().__init__(name, description, accession, sequences)

    @property
    def sequences(self) -> List[DigitalSequence]:
        gap = self.alphabet.symbols[self.alphabet.K]
        return [DigitalSequence(self.alphabet, name=nm, description=d, accession=a,
                                sequence=self.alphabet.encode(r.upper().replace(".", gap).replace("-", gap)))
                for nm, r, d, a in zip(self._names, self._rows, self._descs, self._accs)]

    def textize(self) -> TextMSA:
        out = TextMSA._from_rows(self._names, self._rows, self._descs, self._accs, self.posterior_probabilities,
                                 self.pp_consensus, self.reference, self.secondary_structure)
        out._weights = None if self._weights is None else self._weights.copy()
        return out

    def reverse_complement(self, inplace: bool = False) -> Optional["DigitalMSA"]:
        """The reverse complement of every row, gaps kept (reference ``easel.pyx:6479-6523``); per-column annotation is
        reversed with the columns.  `ValueError` for an alphabet without complements."""
        if not self.alphabet.is_nucleotide():
            raise ValueError(f"{self.alphabet} has no defined complement")
        rev = lambda x: None if x is None else x[::-1]
        rows = [r.encode("ascii")[::-1].translate(_TEXT_COMPLEMENT_KEEP).decode("ascii") for r in self._rows]
        pp = None if self.posterior_probabilities is None else [rev(r) for r in self.posterior_probabilities]
        out = self if inplace else DigitalMSA._from_rows(self._names, rows, self._descs, self._accs, alphabet=self.alphabet)
        out._rows, out._code_matrix = rows, None
        out.posterior_probabilities, out.pp_consensus = pp, rev(self.pp_consensus)
        out.reference, out.secondary_structure = rev(self.reference), rev(self.secondary_structure)
        if not inplace:
            out.name, out.description, out.accession, out.author = self.name, self.description, self.accession, self.author
            out._weights = None if self._weights is None else self._weights.copy()
            return out
        return None

    def _residue_mask(self) -> np.ndarray:
        """Residues are the canonical and the degenerate codes; the gap, ``*`` and ``~`` are none."""
        ax, K, Kp = self._codes(), self.alphabet.K, self.alphabet.Kp
        return (ax < K) | ((ax > K) & (ax <= Kp - 3))

    # ---- preparing an alignment: identity filter and relative weights (reference easel.pyx:6247-6477)
    @staticmethod
    def _check_weight_arguments(fragment_threshold, consensus_fraction, sample_threshold, sample_count, max_fragments, preference):
        from .errors import InvalidParameter
        if fragment_threshold < 0 or fragment_threshold > 1:
            raise InvalidParameter("fragment_threshold", fragment_threshold, hint="real number between 0 and 1")
        if consensus_fraction < 0 or consensus_fraction > 1:
            raise InvalidParameter("consensus_fraction", consensus_fraction, hint="real number between 0 and 1")
        if sample_threshold < 0:
            raise InvalidParameter("sample_threshold", sample_threshold, hint="positive integer")
        if sample_count < 0:
            raise InvalidParameter("sample_count", sample_count, hint="positive integer")
        if max_fragments < 0:
            raise InvalidParameter("max_fragments", max_fragments, hint="positive integer")
        if preference not in _MSA_WEIGHT_PREFERENCES:
            raise InvalidParameter("preference", preference, choices=list(_MSA_WEIGHT_PREFERENCES))

    def _rf_mask(self, ignore_rf: bool) -> Optional[np.ndarray]:
        if self.reference is None or ignore_rf:
            return None
        return np.array([c not in "-._~" for c in self.reference], dtype=np.uint8)

    def _conscover_order(self, fragment_threshold: float, consensus_fraction: float, ignore_rf: bool) -> np.ndarray:
        """The rows by decreasing number of consensus columns inside their span; ties keep the alignment's order.
        Consensus columns: the ``#=GC RF`` columns, or residues / (residues + gaps) >= ``consensus_fraction`` over all
        the rows, a fragment's cells outside its span counting as missing.  O(N L) host code."""
        res, has, first, last = self._spans()
        n, alen = res.shape
        cons = self._rf_mask(ignore_rf)
        if cons is None:
            gap = self._codes() == self.alphabet.K
            frag = has & ((last - first + 1).astype(np.float64) / float(alen) < fragment_threshold)
            if frag.any():
                cols = np.arange(alen)
                gap &= ~(frag[:, None] & ((cols[None, :] < first[:, None]) | (cols[None, :] > last[:, None])))
            r, g = res.sum(axis=0, dtype=np.int64), gap.sum(axis=0, dtype=np.int64)
            cons = (r + g > 0) & (r.astype(np.float64) >= consensus_fraction * (r + g).astype(np.float64))
        cum = np.concatenate([[0], np.cumsum(cons != 0, dtype=np.int64)])
        cover = np.where(has, cum[last + 1] - cum[first], 0)
        return np.argsort(-cover, kind="stable").astype(np.int64)

    def _filter_order(self, preference: str, fragment_threshold: float = 0.5, consensus_fraction: float = 0.5,
                      ignore_rf: bool = False, seed: Optional[int] = 42) -> np.ndarray:
        """The order in which ``identity_filter`` visits the rows (int64 row indices)."""
        n = len(self._rows)
        if preference == "conscover":
            return self._conscover_order(float(np.float32(fragment_threshold)), float(np.float32(consensus_fraction)), bool(ignore_rf))
        order = np.arange(n, dtype=np.int64)
        if preference == "random":
            u = Randomness((int(seed) & 0xFFFFFFFF) if seed else None)._draw(max(n - 1, 1))
            for k, i in enumerate(range(n - 1, 0, -1)):            # Fisher-Yates, from the top
                j = int(u[k] * (i + 1))
                order[i], order[j] = order[j], order[i]
        return order

    def identity_filter(self, max_identity: float = 0.8, fragment_threshold: float = 0.5, consensus_fraction: float = 0.5,
                        ignore_rf: bool = False, sample: bool = True, sample_threshold: int = 50000, sample_count: int = 10000,
                        max_fragments: int = 5000, seed: Optional[int] = 42, preference: str = "conscover",
                        device: int = 0) -> "DigitalMSA":
        """Remove rows by fractional identity (``esl-weight -f``; reference ``easel.pyx:6369-6477``): the rows are visited
        in the order of ``preference`` and a row is kept unless its pairwise identity -- identical canonical residues over
        the shorter of the two rows -- to a row already kept is at least ``max_identity`` (taken as a C ``float``, as
        in the reference).  The result holds the rows kept, in the alignment's own order.

        ``preference``: ``"conscover"`` (rows whose span covers more consensus columns first), ``"origorder"``, or
        ``"random"`` (a shuffle drawn from ``Randomness(seed)``; 0 or `None`: an arbitrary seed).  The consensus is always
        taken from all the rows: ``sample``, ``sample_threshold``, ``sample_count`` and ``max_fragments`` are checked as
        the reference checks them and otherwise unused.  The pairwise identities are counted on ``device``; there is no
        CPU path (`DeviceUnavailable` without a device)."""
        from . import _lib
        from .errors import status_to_exception
        self._check_weight_arguments(fragment_threshold, consensus_fraction, sample_threshold, sample_count, max_fragments, preference)
        n, alen = len(self._rows), len(self)
        if n == 0 or alen == 0:
            return self.select()
        order = self._filter_order(preference, fragment_threshold, consensus_fraction, ignore_rf, seed)
        ax = np.ascontiguousarray(self._codes())
        keep = np.zeros(n, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.int64)
        st = _lib.lib().p7x_msa_idfilter(self.alphabet.type_code, ax.ctypes.data, n, alen, order.ctypes.data, float(max_identity),
                                         int(device), keep.ctypes.data, stats.ctypes.data)
        if st != 0:
            raise status_to_exception(st, "p7x_msa_idfilter", _lib.last_error())
        out = self.select(sequences=np.flatnonzero(keep))
        out._pair_stats = stats
        return out

    def compute_weights(self, method: str = "pb", max_identity: float = 0.62, fragment_threshold: float = 0.5,
                        consensus_fraction: float = 0.5, ignore_rf: bool = False, sample: bool = True, sample_threshold: int = 50000,
                        sample_count: int = 10000, max_fragments: int = 5000, seed: Optional[int] = 42,
                        preference: str = "conscover", device: int = 0) -> np.ndarray:
        """Relative weights of the rows (``esl-weight``; reference ``easel.pyx:6247-6367``), stored in
        ``sequence_weights`` and returned (a numpy array where the reference returns a ``VectorD``).

        ``"blosum"``: single-linkage clusters of the rows at ``max_identity`` (pairwise identity as in
        ``identity_filter``), 1 / (size of the row's cluster), scaled to sum to the number of rows; any alphabet; the
        identities are counted on ``device``.  ``"pb"``: Henikoff position-based weights over the consensus columns, by
        the unit behind ``Builder.build_msa`` (``fragment_threshold``, ``consensus_fraction`` and the ``#=GC RF`` line
        mapped onto it; weights in fixed point, unit 2^-40): amino alignments only.  ``"gsc"`` is not built.  The four
        sampling arguments and ``preference`` are checked and otherwise unused."""
        import ctypes as C
        from . import _lib
        from .errors import InvalidParameter, status_to_exception
        method = method.lower()
        if method == "gsc":
            raise NotImplementedError("Gerstein/Sonnhammer/Chothia weights are not built (DESIGN.md 3.16)")
        if method not in ("pb", "blosum"):
            raise InvalidParameter("method", method, choices=["pb", "gsc", "blosum"])
        n, alen = len(self._rows), len(self)
        if method == "blosum":
            if n == 0 or alen == 0:
                w = np.ones(n, dtype=np.float64)
            else:
                ax = np.ascontiguousarray(self._codes())
                cluster = np.zeros(n, dtype=np.int32)
                ncl, stats = C.c_int64(), np.zeros(4, dtype=np.int64)
                st = _lib.lib().p7x_msa_linkage(self.alphabet.type_code, ax.ctypes.data, n, alen, float(max_identity), int(device),
                                                cluster.ctypes.data, C.byref(ncl), stats.ctypes.data)
                if st != 0:
                    raise status_to_exception(st, "p7x_msa_linkage", _lib.last_error())
                w = 1.0 / np.bincount(cluster, minlength=n)[cluster].astype(np.float64)
                w *= n / w.sum()
                self._pair_stats, self._clusters = stats, cluster
        else:
            self._check_weight_arguments(fragment_threshold, consensus_fraction, sample_threshold, sample_count, max_fragments, preference)
            if not self.alphabet.is_amino():
                raise NotImplementedError("position-based weights are built for amino alignments only (the unit behind Builder.build_msa)")
            if n == 0 or alen == 0:
                raise ValueError("the alignment is empty")
            ax = np.ascontiguousarray(self._codes())
            rf = self._rf_mask(bool(ignore_rf))
            handle = C.c_void_p()
            lib = _lib.lib()
            st = lib.p7x_msa_counts(self.alphabet.type_code, ax.ctypes.data, n, alen, None if rf is None else rf.ctypes.data, 1,
                                    float(np.float32(consensus_fraction)), float(np.float32(fragment_threshold)), int(device), C.byref(handle))
            if st != 0:
                raise status_to_exception(st, "p7x_msa_counts", _lib.last_error())
            try:
                wq = np.zeros(n, dtype=np.uint64)
                if lib.p7x_msacounts_get(handle, 1, wq.ctypes.data, wq.nbytes) != 0:
                    raise ValueError(_lib.last_error())
            finally:
                lib.p7x_msacounts_destroy(handle)
            w = np.ldexp(wq.astype(np.float64), -40)
        self._weights = w
        return w

    def _codes(self) -> np.ndarray:
        """The alignment as an ``(N, L)`` matrix of digital codes (every gap character is the alphabet's gap code):
        what ``Builder.build_msa`` counts over.  An alignment that came with its matrix (``TopHits.to_msa`` with
        ``digitize``: ``p7x_msa_codes``) hands that out, read-only, for as long as its rows are the ones it was made of;
        every other one encodes its text rows."""
        kept = getattr(self, "_code_matrix", None)
        if kept is not None:
            ax, rows = kept
            if len(rows) == len(self._rows) and all(a is b for a, b in zip(rows, self._rows)):
                return ax
            self._code_matrix = None             # the rows were replaced: the matrix is no longer theirs
        return self._encode_rows()

    def _keep_codes(self, ax: np.ndarray) -> None:
        """Keep ``ax`` as the code matrix of the rows as they are now (strings are immutable: the same row objects are the
        same text).  ``select`` / ``identity_filter`` / ``digitize`` / ``textize`` build new alignments, which start without one."""
        ax.setflags(write=False)
        self._code_matrix = (ax, tuple(self._rows))

    def _encode_rows(self) -> np.ndarray:
        """The text rows encoded: the ``(N, L)`` matrix of ``_codes`` from scratch."""
        n, alen = len(self._rows), len(self)
        out = self.alphabet._lut[np.frombuffer("".join(self._rows).encode("ascii"), dtype=np.uint8)].reshape(n, alen)
        if (out == 255).any():
            i, c = np.argwhere(out == 255)[0]
            raise ValueError(f"Invalid symbol {self._rows[i][c]!r} for alphabet {self.alphabet!r}")
        return out


class KeyHash:
    """A dynamic set of keys that remembers the order they came in (reference ``easel.pyx`` ``KeyHash``; ``ESL_KEYHASH``):
    ``add`` returns the index of a key, new or not; ``key in kh``; ``kh[key]`` its index (`KeyError` when absent);
    ``len``; iteration in insertion order; ``clear``; ``copy``.  What ``TopHits.compare_ranking`` keeps the included hits
    of a jackhmmer round in."""

    __slots__ = ("_index",)

    def __init__(self):
        self._index: dict = {}

    def add(self, key: str) -> int:
        if not isinstance(key, str):
            raise TypeError(f"expected str, found {type(key).__name__}")
        return self._index.setdefault(key, len(self._index))

    def __contains__(self, key) -> bool:
        return isinstance(key, str) and key in self._index

    def __getitem__(self, key: str) -> int:
        if not isinstance(key, str):
            raise TypeError(f"expected str, found {type(key).__name__}")
        return self._index[key]

    def __len__(self) -> int:
        return len(self._index)

    def __iter__(self):
        return iter(list(self._index))

    def __eq__(self, other) -> bool:
        if not isinstance(other, KeyHash):
            return NotImplemented
        return list(self._index) == list(other._index)

    def __repr__(self) -> str:
        return f"<KeyHash of {len(self._index)} keys>"

    def clear(self) -> None:
        self._index.clear()

    def copy(self) -> "KeyHash":
        out = KeyHash()
        out._index = dict(self._index)
        return out

    __copy__ = copy


class MSAFile:
    """Alignment reader with the reference's ``MSAFile`` surface (``read``, iteration, context manager).  Interleaved or
    single-block Stockholm only: ``#=GF ID / AC / DE``, ``#=GS <name> AC / DE / WT``, ``#=GC RF / SS_cons / PP_cons``,
    ``#=GR <name> PP``, any number of alignments per file, each closed by ``//``.  Other annotation is skipped."""

    def __init__(self, file, format: str = "stockholm", *, digital: bool = False, alphabet: Optional[Alphabet] = None):
        if format not in ("stockholm", "pfam"):
            raise ValueError(f"unsupported MSA format: {format!r} (only 'stockholm')")
        if isinstance(file, (str, bytes, os.PathLike)):
            self._fh = open(file, "r")
            self._own = True
            self.name = os.fspath(file)
        else:
            self._fh = file
            self._own = False
            self.name = getattr(file, "name", None)
        self.format = "stockholm"
        self.digital = digital
        self.alphabet = alphabet
        if digital and alphabet is None:
            self.alphabet = self.guess_alphabet()
            if self.alphabet is None:
                raise ValueError("Could not determine alphabet of file")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self) -> None:
        if self._own:
            self._fh.close()

    def guess_alphabet(self) -> Optional[Alphabet]:
        """Amino unless at least nine residues in ten of the first alignment are nucleotides (RNA when it holds a U)."""
        pos = self._fh.tell()
        msa = self._read_text()
        self._fh.seek(pos)
        if msa is None:
            return None
        text = "".join(msa._rows).upper()
        res = [c for c in text if c.isalpha()]
        if not res:
            return None
        if sum(c in "ACGTUN" for c in res) >= 0.9 * len(res):
            return Alphabet.rna() if "U" in res else Alphabet.dna()
        return Alphabet.amino()

    def _line(self) -> str:
        line = self._fh.readline()
        return line.decode() if isinstance(line, bytes) else line

    def _read_text(self) -> Optional["TextMSA"]:
        line = self._line()
        while line and not line.strip():
            line = self._line()
        if not line:
            return None
        if not line.startswith("# STOCKHOLM 1."):
            raise ValueError(f"not a Stockholm file: expected '# STOCKHOLM 1.0', found {line.rstrip()!r}")
        gf, gc = {}, {}
        names: List[str] = []
        rows, pp, accs, descs, wts = {}, {}, {}, {}, {}
        closed = False
        for line in iter(self._line, ""):
            line = line.rstrip("\r\n")
            if line.startswith("//"):
                closed = True
                break
            if not line.strip():
                continue
            if line.startswith("#=GF"):
                f = line.split(None, 2)
                if len(f) == 3 and f[1] in ("ID", "AC", "DE"):
                    gf[f[1]] = (gf[f[1]] + " " if f[1] in gf else "") + f[2].strip()
            elif line.startswith("#=GS"):
                f = line.split(None, 3)
                if len(f) == 4 and f[2] in ("AC", "DE"):
                    (accs if f[2] == "AC" else descs)[f[1]] = f[3].strip()
                elif len(f) == 4 and f[2] == "WT":
                    wts[f[1]] = float(f[3])
            elif line.startswith("#=GC"):
                f = line.split()
                if len(f) == 3:
                    gc[f[1]] = gc.get(f[1], "") + f[2]
            elif line.startswith("#=GR"):
                f = line.split()
                if len(f) == 4 and f[2] == "PP":
                    pp[f[1]] = pp.get(f[1], "") + f[3]
            elif line.startswith("#"):
                continue
            else:
                f = line.split()
                if len(f) != 2:
                    raise ValueError(f"malformed Stockholm line: {line!r}")
                if f[0] not in rows:
                    names.append(f[0])
                    rows[f[0]] = ""
                rows[f[0]] += f[1]
        if not closed:
            raise ValueError("Stockholm alignment is not closed by '//'")
        alen = len(rows[names[0]]) if names else 0
        for what, d in (("sequence", rows), ("#=GR PP", pp), ("#=GC", gc)):
            for key, text in d.items():
                if len(text) != alen:
                    raise ValueError(f"{what} line {key!r} has {len(text)} columns, the alignment {alen}")
        msa = TextMSA._from_rows(names, [rows[n] for n in names], [descs.get(n, "") for n in names],
                                 [accs.get(n, "") for n in names], [pp[n] for n in names] if len(pp) == len(names) and names else None,
                                 gc.get("PP_cons"), gc.get("RF"), gc.get("SS_cons"))
        msa.name, msa.accession, msa.description = gf.get("ID"), gf.get("AC"), gf.get("DE")
        if names and all(n in wts for n in names):      # the file's weights as they stand, as Easel takes them
            msa._weights = np.array([wts[n] for n in names], dtype=np.float64)
        return msa

    def read(self):
        """The next alignment of the file (``TextMSA``, or ``DigitalMSA`` in digital mode); ``None`` at the end."""
        msa = self._read_text()
        if msa is None or not self.digital:
            return msa
        out = msa.digitize(self.alphabet)
        out.name, out.accession, out.description = msa.name, msa.accession, msa.description
        out._codes()                        # an illegal character is reported where the file is read
        return out

    def __iter__(self):
        return self

    def __next__(self):
        msa = self.read()
        if msa is None:
            raise StopIteration
        return msa


class Randomness:
    """A random number generator (reference ``easel.pyx:7006-7161``, ``ESL_RANDOMNESS``): Easel's Mersenne Twister
    (MT19937 seeded by ``mt[z] = 69069 mt[z-1]``) or, with ``fast=True``, its linear congruential generator
    ``x <- 69069 x + 1`` -- the two generators the calibration stream and the domain-definition ensembles already draw
    from (``p7x_rng.hpp``), so the streams of deviates are Easel's.  A seed of ``0`` or `None` takes an arbitrary seed
    (from the operating system, where Easel mixes the clock and the process id).

    ``normalvariate`` has the distribution of ``esl_rnd_Gaussian`` but not its stream: it is the polar Box-Muller method on
    ``random()``, not the RANLIB routine Easel restates.  As in the reference ``seed`` is a method; the seed in use is
    ``getstate()[1]`` and shows in the ``repr``."""

    _WORDS = 626                  # P7X_RNG_STATE_WORDS: mt[624], mti, x

    def __init__(self, seed=None, fast: bool = False):
        self._fast = bool(fast)
        self._state = np.zeros(self._WORDS, dtype=np.uint32)
        self._seed = 0
        self.seed(seed)

    def seed(self, n=None) -> None:
        """Reinitialize the generator with the given seed (``esl_randomness_Init``)."""
        import ctypes as C
        from . import _lib
        n = 0 if n is None else int(n)
        if not 0 <= n < 1 << 32:
            raise OverflowError("seed does not fit 32 bits")
        while n == 0:
            n = int.from_bytes(os.urandom(4), "little")
        self._seed = n
        if _lib.lib().p7x_rng_seed(1 if self._fast else 0, n, self._state.ctypes.data) != 0:
            raise ValueError(_lib.last_error())

    @property
    def fast(self) -> bool:
        """`True` when the linear congruential generator is in use."""
        return self._fast

    def __repr__(self) -> str:
        return f"{type(self).__name__}({self._seed!r}, fast={self._fast!r})"

    def getstate(self) -> tuple:
        if self._fast:
            return (True, self._seed, int(self._state[625]))
        return (False, self._seed, int(self._state[624]), [int(x) for x in self._state[:624]])

    def setstate(self, state: tuple) -> None:
        self._seed = int(state[1])
        self._fast = bool(state[0])
        if self._fast:
            self._state[625] = int(state[2])
        else:
            self._state[624] = int(state[2])
            self._state[:624] = np.asarray(state[3], dtype=np.uint32)

    def __getstate__(self):
        return self.getstate()

    def __setstate__(self, state):
        if not hasattr(self, "_state"):
            self._state = np.zeros(self._WORDS, dtype=np.uint32)
        self.setstate(state)

    def __reduce__(self):
        state = self.getstate()
        return Randomness, (state[1], state[0]), state

    def copy(self) -> "Randomness":
        new = Randomness.__new__(Randomness)
        new._fast, new._seed, new._state = self._fast, self._seed, self._state.copy()
        return new

    def __copy__(self) -> "Randomness":
        return self.copy()

    def _draw(self, n: int) -> np.ndarray:
        from . import _lib
        out = np.empty(n, dtype=np.float64)
        if _lib.lib().p7x_rng_draw(1 if self._fast else 0, self._state.ctypes.data, n, out.ctypes.data) != 0:
            raise ValueError(_lib.last_error())
        return out

    def random(self) -> float:
        """A uniform deviate on [0, 1) (``esl_random``)."""
        return float(self._draw(1)[0])

    def normalvariate(self, mu: float, sigma: float) -> float:
        """A Gaussian deviate of mean ``mu`` and standard deviation ``sigma``."""
        import math
        while True:
            u, v = 2.0 * self._draw(2) - 1.0
            s = u * u + v * v
            if 0.0 < s < 1.0:
                return float(mu + sigma * u * math.sqrt(-2.0 * math.log(s) / s))
