"""Helpers of the shuffle tests: Philox-4x32-10 and the modes "reverse", "mono" and "window" restated in plain Python from
their definitions, nothing shared with the library; a brute-force enumerator of the arrangements of a short
sequence that keep its first residue, its last residue and every adjacent-pair count; invariants; and block builders."""
import itertools
from collections import Counter

import numpy as np

from pyhmmer_amd import easel

M32 = 0xFFFFFFFF
MODES = ("mono", "di", "window", "reverse")


def philox4x32_10(key, ctr):
    """Salmon et al., SC'11: ten rounds, the key bumped by the Weyl constants after each."""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draws(seed, seq, attempt=0):
    """The 64-bit draws of (sequence, attempt): block <step> of the counter (seq low, seq high, attempt, step) gives two."""
    for step in itertools.count():
        v = philox4x32_10((seed, 0), (seq & M32, seq >> 32, attempt, step))
        yield v[0] | v[1] << 32
        yield v[2] | v[3] << 32


def fisher_yates(x, lo, n, stream):
    """From the last position down: position i takes the element at mulhi64(draw, i + 1)."""
    for i in range(n - 1, 0, -1):
        j = (next(stream) * (i + 1)) >> 64
        x[lo + i], x[lo + j] = x[lo + j], x[lo + i]


def restated(codes, mode, seed, seq=0, window=0):
    """reverse / mono / window of one sequence, as specified."""
    x = [int(c) for c in codes]
    L = len(x)
    if mode == "reverse":
        return x[::-1]
    stream = draws(seed, seq)
    if mode == "mono":
        fisher_yates(x, 0, L, stream)
    elif mode == "window":
        for b in range(0, L, window):
            fisher_yates(x, b, min(window, L - b), stream)
    else:
        raise ValueError(mode)
    return x


def pair_counts(codes, Kp):
    m = np.zeros((Kp, Kp), dtype=np.int64)
    c = np.asarray(codes, dtype=np.int64)
    if c.size > 1:
        np.add.at(m, (c[:-1], c[1:]), 1)
    return m


def di_arrangements(codes):
    """Every sequence with the first residue, the last residue and the adjacent-pair counts of <codes>, by trying every
    way to spend the pairs from the first residue on (sorted tuples)."""
    x = [int(c) for c in codes]
    if len(x) < 3:
        return [tuple(x)]
    left = Counter(zip(x[:-1], x[1:]))
    found = []

    def extend(path):
        if len(path) == len(x):
            if path[-1] == x[-1]:
                found.append(tuple(path))
            return
        for (a, b), k in sorted(left.items()):
            if a == path[-1] and k > 0:
                left[(a, b)] -= 1
                path.append(b)
                extend(path)
                path.pop()
                left[(a, b)] += 1

    extend([x[0]])
    return sorted(set(found))


def di_arrangements_by_permutation(codes):
    """The same by filtering every permutation of the inner residues (for sequences of up to nine residues)."""
    x = [int(c) for c in codes]
    want = Counter(zip(x[:-1], x[1:]))
    out = set()
    for inner in set(itertools.permutations(x[1:-1])):
        y = (x[0],) + inner + (x[-1],)
        if Counter(zip(y[:-1], y[1:])) == want:
            out.add(y)
    return sorted(out)


def make_block(seqs, alphabet):
    """A DigitalSequenceBlock of code arrays, named s0, s1, ... with a description and an accession each."""
    return easel.DigitalSequenceBlock(alphabet, [
        easel.DigitalSequence(alphabet, name=f"s{i}", description=f"sequence {i}", accession=f"ACC{i}",
                              sequence=np.asarray(s, dtype=np.uint8)) for i, s in enumerate(seqs)])


def random_codes(rng, L, alphabet, degenerate=True):
    """L codes; with <degenerate> about one in eight from the whole alphabet (degenerate codes, *, ~), the rest canonical."""
    c = rng.integers(0, alphabet.K, size=L)
    if degenerate and L:
        any_code = rng.integers(0, alphabet.Kp, size=L)
        c = np.where(rng.random(L) < 0.125, any_code, c)
    return c.astype(np.uint8)


def decoys(block_out):
    """The sequences of a shuffled block as a list of uint8 arrays, from its packed arrays."""
    pk = block_out.packed()
    return [pk.dsq[o:o + L] for o, L in zip(pk.offsets.tolist(), pk.lengths.tolist())]


def check_invariants(src, out, mode, window, Kp):
    """What every mode keeps of one sequence."""
    src, out = np.asarray(src), np.asarray(out)
    assert out.shape == src.shape
    assert np.array_equal(np.sort(out), np.sort(src))
    L = len(src)
    if mode == "reverse":
        assert np.array_equal(out, src[::-1])
    if mode == "window":
        for b in range(0, L, window):
            assert np.array_equal(np.sort(out[b:b + window]), np.sort(src[b:b + window]))
    if mode == "di":
        if L < 3:
            assert np.array_equal(out, src)
        if L:
            assert out[0] == src[0] and out[-1] == src[-1]
        assert np.array_equal(pair_counts(out, Kp), pair_counts(src, Kp))
