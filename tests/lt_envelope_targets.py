"""Targets for the long-target envelope reference (test input only): DNA models whose planted fragments go through every
nodes-per-lane tier of the envelope kernel's long-target instantiation, and the float64 reference of
tests/lt_envelope_reference.py on them, computed once per session and shared by tests/test_host_lt_envelope_reference.py and
tests/test_gpu_lt_envelope_reference.py.

Per tier: random_hmm(M, alphabet = DNA) for the last model length of every tier of P7X_NODE_TIERS and the first of the next
-- M = 64 C and 64 C + 1 -- plus M = 12,288 and one model below 64 nodes (SHORT_M: padding lanes).  What changes with C for
this mode: the per-envelope table's layout in HBM (node k at ((k - 1) % C) * 64 + (k - 1) / C of its row), which is never
staged in LDS.

One target per model: TARGET_LENGTH residues of i.i.d. ACGT with three fragments emitted from the model
(envelope_targets.emit_window over at most FRAGMENT_NODES nodes) at POSITIONS: the model's first nodes, its last nodes
(ending at node M; planted on the reverse strand) and a window centred on the boundary between lanes 31 and 32, node 32 C.
Models shorter than the window: the whole emission, three times.  Searches run with window_length = WINDOW_LENGTH.

"rnd1100 long": full-length emissions of random_hmm(1100), about 1,000 residues each, one per strand -- float32 sums over
Ld rows, and nothing for the second round to trim.
"rnd300 edges": full-length emissions, one per strand, with N and the two-letter IUPAC codes in 10 % of their residues: the
degenerate rows of the per-envelope table and the fractional counts of the composition.

QUEUE_LABEL, "rnd320 queue" (not part of LABELS): the DNA model of the tier C = 5 and one contig with QUEUE_FRAGMENTS planted
fragments of 60 nodes up to the whole model (320: the model has no 400), alternating strands, shortest first, 1,400 residues
apart -- so that a search forced onto one block (the test option env_blocks) hands every wavefront several envelopes, each
with its own emission table, through one workspace slab: tests/test_gpu_envelope_queue.py."""
import numpy as np

import envelope_targets as ET
from conftest import random_hmm
from host_pipeline import DNA_COMP
from pyhmmer_amd import easel, plan7

SHORT_M = 48
FULL_LENGTHS = tuple(sorted({SHORT_M, 12288} | {64 * c for c in ET.TIER_C} | {64 * c + 1 for c in ET.TIER_C}))
FRAGMENT_NODES = 200
TARGET_LENGTH = 24_000
POSITIONS = (4_000, 12_000, 20_000)
WINDOW_LENGTH = 1200
# Replaced where a planted fragment is not a reported hit of the default pipeline.  Fragments emitted from the model carry
# its insertions and deletions, so their ungapped diagonals are short: a few of them do not seed an SSV window or lose it at
# the MSV test (all three of rnd6144; rnd2049's boundary fragment is seeded and dropped at MSV), and the short models' score
# a few bits.  A fragment's salt re-draws that fragment alone (the first salt of 1, 2, ... that gives a hit).  The model below
# 64 nodes: none of 31 seeds of M = 16, 24, 32, 40 gives three reported hits; M = 48 does with seed 8048 (7348 does not).
MODEL_SEEDS = {48: 8048}
TARGET_SALTS = {("rnd64", "boundary"): 2, ("rnd65", "first"): 1, ("rnd2049", "boundary"): 1,
                ("rnd6144", "first"): 2, ("rnd6144", "last"): 1, ("rnd6144", "boundary"): 1,
                # not for a missing hit: the optimal-accuracy traces of this fragment (salt 0) and of the label's "last" one each
                # pass a match cell whose two best predecessors differ by less than the near-tie guard's band in float64 already
                # (2.0e-4 at 105.7 and 3.4e-4 at 187.1; band 4e-6 (value + 1)), so the guard rightly sends two of the label's
                # three envelopes to the host, and "at most half repeated" fails on the data, not on the guard.  Salts 1 and 2
                # are no hits; salt 3 is one and has no such cell.  The "last" fragment keeps its near-tie.
                ("rnd8193", "boundary"): 3}
DEGENERATE_CODES = (15, 5, 6, 7, 8, 9, 10)          # N; R Y M K S W
QUEUE_LABEL = "rnd320 queue"
QUEUE_FRAGMENTS = 16
QUEUE_NODES = (60, 400)
QUEUE_FIRST, QUEUE_STEP = 1_000, 1_400

_models, _targets, _ref_models, _refs = {}, {}, {}, {}


def dna():
    return easel.Alphabet.dna()


def label_of(M):
    return f"rnd{M}"


def model(label):
    """label: "rnd<M>", with a suffix for the two extra families ("rnd1100 long", "rnd300 edges")."""
    M = int(label.split()[0][3:])
    if M not in _models:
        _models[M] = random_hmm(M, seed=MODEL_SEEDS.get(M, 7300 + M), alphabet=dna())
    return _models[M]


def windows(M):
    """(name, first node, last node, reverse strand) of the three fragments."""
    n = min(M, FRAGMENT_NODES)
    mid = 32 * ET.tier_of(M)
    a = min(max(1, mid - n // 2 + 1), M - n + 1)
    return (("first", 1, n, False), ("last", M - n + 1, M, True), ("boundary", a, a + n - 1, False))


def queue_windows(M):
    """(name, first node, last node, reverse strand) of the fragments of QUEUE_LABEL, shortest first."""
    mid = 32 * ET.tier_of(M)
    out = []
    for t, n in enumerate(np.linspace(QUEUE_NODES[0], min(QUEUE_NODES[1], M), QUEUE_FRAGMENTS).round().astype(int)):
        n = int(n)
        a = (M - n + 1, min(max(1, mid - n // 2 + 1), M - n + 1), 1 + (7919 * (t + 1)) % (M - n + 1))[t % 3]
        out.append((f"q{t:02d}", a, a + n - 1, t % 2 == 1))
    return out


def _rng(label, name):
    return np.random.default_rng([sum(label.encode()), sum(name.encode()), TARGET_SALTS.get((label, name), 0), 16])


def target(label):
    """(residues, planted) of a label: planted = [(name, first residue (1-based), last residue, reverse strand)]."""
    if label in _targets:
        return _targets[label]
    hmm = model(label)
    M = hmm.M
    seq = _rng(label, "background").integers(0, 4, size=TARGET_LENGTH).astype(np.uint8)
    if label.endswith(" long"):
        plan = (("full", 1, M, False), ("full_rev", 1, M, True))
    elif label.endswith(" edges"):
        plan = (("degenerate", 1, M, False), ("degenerate_rev", 1, M, True))
    else:
        plan = windows(M)
    positions = POSITIONS
    if label.endswith(" queue"):
        plan = queue_windows(M)
        positions = tuple(QUEUE_FIRST + QUEUE_STEP * t for t in range(len(plan)))
    planted = []
    for pos, (name, first, last, rev) in zip(positions, plan):
        rng = _rng(label, name)
        frag = ET.emit_window(hmm, rng, first, last).astype(np.uint8)
        if label.endswith(" edges"):
            hit = rng.random(len(frag)) < 0.10
            frag[hit] = rng.choice(DEGENERATE_CODES, size=int(hit.sum()))
        assert pos + len(frag) + 500 < TARGET_LENGTH
        seq[pos:pos + len(frag)] = DNA_COMP[frag[::-1]] if rev else frag
        planted.append((name, pos + 1, pos + len(frag), rev))
    _targets[label] = (seq, planted)
    return _targets[label]


TIER_LABELS = tuple(label_of(M) for M in FULL_LENGTHS)
EXTRA_LABELS = ("rnd1100 long", "rnd300 edges")
LABELS = TIER_LABELS + EXTRA_LABELS
assert tuple(sorted({ET.tier_of(M) for M in FULL_LENGTHS})) == ET.ALL_TIERS          # every tier of the kernel, none twice missing


def block(label):
    return easel.DigitalSequenceBlock(dna(), [easel.DigitalSequence(dna(), name="target", sequence=target(label)[0])])


def pipeline(**options):
    return plan7.LongTargetsPipeline(dna(), window_length=WINDOW_LENGTH, **options)


def strand_residues(seq, lo, hi, rev):
    """Residues lo..hi (1-based, on the forward strand) as the strand <rev> reads them."""
    sub = np.asarray(seq[lo - 1:hi])
    return DNA_COMP[sub[::-1]] if rev else sub


def hit_envelope(d):
    """(lo, hi, reverse strand) of a long-target domain; the strand column reads "-" for an alignment of one residue, so the
    envelope's ends tell."""
    rev = d.env_from > d.env_to if d.env_from != d.env_to else d.strand == "-"
    return min(d.env_from, d.env_to), max(d.env_from, d.env_to), rev


def covers(planted_one, lo, hi, rev):
    """Does the envelope lo..hi on strand <rev> lie on the planted fragment (at least half of the fragment inside it)?"""
    _, a, b, prev = planted_one
    return prev == rev and min(hi, b) - max(lo, a) + 1 >= (b - a + 1) // 2


# ---- the float64 reference, once per (model, envelope)
def ref_model(label):
    key = label.split()[0]
    if key not in _ref_models:
        hmm = model(label)
        _ref_models[key] = ET.ref_model(("dna", key), hmm)
    return _ref_models[key]


def reference(label, lo, hi, rev):
    """tests/lt_envelope_reference.envelope of residues lo..hi of the label's target on strand <rev>, s = 0.25 (every window
    that holds a checked envelope is at least 100 residues long: asserted where the envelopes are collected)."""
    import lt_envelope_reference as LR
    slot = (label, int(lo), int(hi), bool(rev))
    if slot not in _refs:
        hmm = model(label)
        bg = plan7.Background(hmm.alphabet).residue_frequencies
        _refs[slot] = LR.envelope(ref_model(label), hmm.match_emissions, bg, strand_residues(target(label)[0], lo, hi, rev),
                                  ET.degeneracy(hmm.alphabet))
    return _refs[slot]
