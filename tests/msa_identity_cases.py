"""Pairwise identity of alignment rows: a plain numpy restatement of the definitions, a seeded generator
of alignments, and thin wrappers of the C entry points, shared by tests/test_host_msa_identity.py and
tests/test_gpu_msa_identity.py.

The restatement divides in double and compares with the threshold as a C float, as the definitions are written; it shares
nothing with the library's integer table ``need[]``."""
import ctypes as C
import functools
import io

import numpy as np

from pyhmmer_amd import _lib, easel

THRESHOLDS = (0.0, 0.25, 0.62, 1.0)


# ----------------------------------------------------------------------------- the restatement
def pair_counts(ax: np.ndarray, K: int):
    """idents[N][N] (uint32) and len[N] (uint32)."""
    canon = ax < K
    n = ax.shape[0]
    idents = np.zeros((n, n), dtype=np.uint32)
    for i in range(n):
        idents[i] = ((ax == ax[i][None, :]) & canon & canon[i][None, :]).sum(axis=1)
    return idents, canon.sum(axis=1).astype(np.uint32)


def linked_matrix(ax: np.ndarray, K: int, max_identity: float) -> np.ndarray:
    idents, length = pair_counts(ax, K)
    shorter = np.minimum.outer(length, length).astype(np.float64)
    pid = np.divide(idents.astype(np.float64), shorter, out=np.zeros_like(shorter), where=shorter > 0)
    return pid >= float(np.float32(max_identity))


def max_identity_of(ax: np.ndarray, K: int) -> float:
    idents, length = pair_counts(ax, K)
    shorter = np.minimum.outer(length, length).astype(np.float64)
    pid = np.divide(idents.astype(np.float64), shorter, out=np.zeros_like(shorter), where=shorter > 0)
    np.fill_diagonal(pid, 0.0)
    return float(pid.max())


def greedy_keep(linked: np.ndarray, order) -> np.ndarray:
    keep = np.zeros(linked.shape[0], dtype=np.uint8)
    kept = []
    for i in order:
        if not any(linked[i, k] for k in kept):
            kept.append(int(i))
            keep[i] = 1
    return keep


def cluster_labels(linked: np.ndarray) -> np.ndarray:
    """Single-linkage clusters: the smallest row index of every row's cluster."""
    n = linked.shape[0]
    label = np.full(n, -1, dtype=np.int32)
    for s in range(n):
        if label[s] >= 0:
            continue
        label[s] = s
        stack = [s]
        while stack:
            i = stack.pop()
            for j in np.flatnonzero(linked[i]):
                if label[j] < 0:
                    label[j] = s
                    stack.append(int(j))
    return label


def blosum_weights(linked: np.ndarray) -> np.ndarray:
    label = cluster_labels(linked)
    w = 1.0 / np.bincount(label, minlength=len(label))[label]
    return w * len(label) / w.sum()


def conscover_order(ax: np.ndarray, K: int, Kp: int, fragthresh: float = 0.5, symfrac: float = 0.5) -> np.ndarray:
    """Loops, cell by cell: rows by decreasing number of consensus columns inside their span, ties in the original order."""
    n, alen = ax.shape
    is_res = lambda a: a < K or K < a <= Kp - 3
    span = []
    for i in range(n):
        cols = [c for c in range(alen) if is_res(ax[i, c])]
        span.append((cols[0], cols[-1]) if cols else None)
    cons = []
    for c in range(alen):
        r = g = 0
        for i in range(n):
            if is_res(ax[i, c]):
                r += 1
            elif ax[i, c] == K:
                frag = span[i] is not None and (span[i][1] - span[i][0] + 1) / alen < fragthresh
                if not (frag and (c < span[i][0] or c > span[i][1])):
                    g += 1
        cons.append(r + g > 0 and r / (r + g) >= symfrac)
    cover = [0 if s is None else sum(cons[s[0]:s[1] + 1]) for s in span]
    return np.array(sorted(range(n), key=lambda i: -cover[i]), dtype=np.int64)


# ----------------------------------------------------------------------------- generated alignments
@functools.lru_cache(maxsize=None)
def generated(n: int, alen: int, amino: bool = True, seed: int = 0) -> np.ndarray:
    """An ``(n, alen)`` code matrix: a few ancestors mutated at several rates, gaps, degenerate codes, ``*``, ``~``, all-gap
    rows, exact and near duplicates.  Read-only (shared between tests)."""
    abc = easel.Alphabet.amino() if amino else easel.Alphabet.dna()
    K, Kp = abc.K, abc.Kp
    rng = np.random.default_rng(1000003 * n + 1009 * alen + 17 * seed + int(amino))
    anc = rng.integers(0, K, size=(3, alen), dtype=np.uint8)
    ax = np.empty((n, alen), dtype=np.uint8)
    for i in range(n):
        row = anc[rng.integers(0, 3)].copy()
        rate = (0.0, 0.1, 0.3, 0.5, 0.9)[rng.integers(0, 5)]
        hit = rng.random(alen) < rate
        row[hit] = rng.integers(0, K, size=int(hit.sum()), dtype=np.uint8)
        other = rng.random(alen)
        row[other < 0.12] = K                                                             # gaps
        row[(other >= 0.12) & (other < 0.15)] = rng.integers(K + 1, Kp - 2)               # a degenerate code
        row[(other >= 0.15) & (other < 0.16)] = Kp - 2                                    # '*'
        row[(other >= 0.16) & (other < 0.17)] = Kp - 1                                    # '~'
        if rng.random() < 0.25 and alen >= 4:                                             # a fragment: gaps outside a span
            a, b = sorted(rng.integers(0, alen, size=2))
            row[:a] = K
            row[b + 1:] = K
        ax[i] = row
    for i in range(2, n, 7):                                                              # planted duplicates
        ax[i] = ax[rng.integers(0, i)]
        if i % 2 and alen > 2:
            ax[i, rng.integers(0, alen)] = rng.integers(0, K)                             # a near duplicate
    for i in range(5, n, 23):
        ax[i] = K                                                                         # all gaps
    ax.setflags(write=False)
    return ax


def as_msa(ax: np.ndarray, amino: bool = True) -> easel.DigitalMSA:
    abc = easel.Alphabet.amino() if amino else easel.Alphabet.dna()
    sym = np.frombuffer(abc.symbols.encode(), dtype=np.uint8)
    rows = [sym[r].tobytes().decode() for r in ax]
    n = len(rows)
    msa = easel.DigitalMSA._from_rows([f"row{i}" for i in range(n)], rows, [""] * n, [""] * n, alphabet=abc)
    msa.name = "generated"
    return msa


def parse(text: bytes, abc: easel.Alphabet) -> easel.DigitalMSA:
    return easel.MSAFile(io.BytesIO(text), digital=True, alphabet=abc).read()


# ----------------------------------------------------------------------------- the C entry points
def _check(st: int, what: str):
    if st != 0:
        from pyhmmer_amd.errors import status_to_exception
        raise status_to_exception(st, what, _lib.last_error())


def lib_counts(ax: np.ndarray, abc_type: int, device: int = 0):
    ax = np.ascontiguousarray(ax)
    n, alen = ax.shape
    idents, length = np.zeros((n, n), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    _check(_lib.lib().p7x_msa_pair_idents(abc_type, ax.ctypes.data, n, alen, device, idents.ctypes.data, length.ctypes.data), "p7x_msa_pair_idents")
    return idents, length


def lib_filter(ax: np.ndarray, abc_type: int, order, max_identity: float, device: int = 0):
    ax = np.ascontiguousarray(ax)
    n, alen = ax.shape
    order = np.ascontiguousarray(order, dtype=np.int64)
    keep, stats = np.zeros(n, dtype=np.uint8), np.zeros(4, dtype=np.int64)
    _check(_lib.lib().p7x_msa_idfilter(abc_type, ax.ctypes.data, n, alen, order.ctypes.data, max_identity, device, keep.ctypes.data,
                                       stats.ctypes.data), "p7x_msa_idfilter")
    return keep, stats


def lib_linkage(ax: np.ndarray, abc_type: int, max_identity: float, device: int = 0):
    ax = np.ascontiguousarray(ax)
    n, alen = ax.shape
    cluster, ncl, stats = np.zeros(n, dtype=np.int32), C.c_int64(), np.zeros(4, dtype=np.int64)
    _check(_lib.lib().p7x_msa_linkage(abc_type, ax.ctypes.data, n, alen, max_identity, device, cluster.ctypes.data, C.byref(ncl),
                                      stats.ctypes.data), "p7x_msa_linkage")
    return cluster, int(ncl.value), stats


def lib_links(ax: np.ndarray, abc_type: int, max_identity: float, rows_a, rows_b, device: int = 0):
    """Link bits ``[na][(nb + 63) // 64]`` (uint64) and the flags ``[na]`` of rows_a against rows_b."""
    ax = np.ascontiguousarray(ax)
    n, alen = ax.shape
    ra, rb = np.ascontiguousarray(rows_a, dtype=np.int32), np.ascontiguousarray(rows_b, dtype=np.int32)
    bits, flags = np.zeros((len(ra), (len(rb) + 63) // 64), dtype=np.uint64), np.zeros(len(ra), dtype=np.uint8)
    _check(_lib.lib().p7x_debug_msa_pair_links(abc_type, ax.ctypes.data, n, alen, max_identity, device, ra.ctypes.data, len(ra),
                                               rb.ctypes.data, len(rb), bits.ctypes.data, flags.ctypes.data), "p7x_debug_msa_pair_links")
    return bits, flags


def pack_bits(linked: np.ndarray) -> np.ndarray:
    """A bool matrix as the library packs link bits: bit j & 63 of word j // 64."""
    na, nb = linked.shape
    out = np.zeros((na, (nb + 63) // 64), dtype=np.uint64)
    for j in range(nb):
        out[:, j // 64] |= linked[:, j].astype(np.uint64) << np.uint64(j % 64)
    return out
