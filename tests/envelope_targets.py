"""Targets for the domain-envelope reference (test input only): small homologues whose one domain goes through every
nodes-per-lane tier of the envelope kernel, and the float64 reference of tests/envelope_reference.py on them, computed once
per session and shared by tests/test_host_envelope_reference.py and tests/test_gpu_envelope_reference.py.

Per tier: random_hmm(M) for the last model length of every tier of P7X_NODE_TIERS and the first of the next -- M = 64 C and
64 C + 1 -- plus M = 5, 63 and 12,288.  What changes with C in env_kernel: padding lanes, emissions out of LDS above 1,024
nodes, four wavefronts per block above 448, rolled loops above C = 32, transitions through L2 above 4,096.

Three targets per model, each a fragment emitted from the model (bench.emit_from_model over a window of at most
FRAGMENT_NODES nodes) between random flanks of 0-50 residues: the model's first nodes, its last nodes (ending at node M), and
a window centred on the boundary between lanes 31 and 32, node 32 C.  Models shorter than the window: the whole emission,
three times.

"rnd1100 long": a full-length emission of random_hmm(1100), about 1,000 residues -- float32 sums over Ld rows.
"rnd300 edges": an envelope from residue 1 to residue L (no flanks), a homologue with X, B and Z in 10 % of its residues, and
a homologue followed by '*'.

"rnd<M> queue" (QUEUE_LABELS, not part of LABELS): many short fragments of one model, so that a search forced onto one block
(the test option env_blocks) hands every wavefront several envelopes of different lengths, one after the other through the
same workspace slab -- tests/test_gpu_envelope_queue.py.  M = 64, 320, 512, 1025, 2049 and 4097: eight wavefronts per block,
four of them from 512 on, emissions out of LDS, rolled loops, transitions through L2.  QUEUE_TARGETS[M] targets of one
fragment each, the window lengths spread evenly from QUEUE_MIN_NODES nodes to min(M, 300) (120 from M = 2049 on), every
third window ending at node M and every third lying across nodes 32 C and 32 C + 1; the block lists them shortest first, the
reverse of the queue's order.  One more target carries six fragments 80 random residues apart: six envelopes of one item at
different offsets into the sequence."""
from types import SimpleNamespace

import numpy as np

import bench
from conftest import random_hmm
from pyhmmer_amd import easel, plan7

TIER_C = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 96, 128)          # P7X_NODE_TIERS below the last, 192
ALL_TIERS = TIER_C + (192,)
FULL_LENGTHS = tuple(sorted({5, 63, 12288} | {64 * c for c in TIER_C} | {64 * c + 1 for c in TIER_C}))
TIER_LENGTHS = FULL_LENGTHS          # (the CPU module stays well under two minutes with every length: none is dropped)
FRAGMENT_NODES = 300
MAX_FLANK = 50
# A seed is replaced here when a fragment of random_hmm(M, seed = 7000 + M) is not one single-domain hit (M = 5: the third
# emission of seed 7005 lies in a region that the traceback ensemble resolves).
MODEL_SEEDS = {5: 7108}
# ("rnd2049 queue", "q01"): the 44-node fragment of salt 0 passes no filter; salt 1 is a hit.
TARGET_SALTS = {("rnd2049 queue", "q01"): 1}
# The whole emission of a 5-node model scores 2-10 bits: no filter lets it through, so this model's searches run with the
# filters open and every target reaches the domain definition.
PIPELINE_OPTIONS = {"rnd5": dict(F1=1.0, F2=1.0, F3=1.0, E=1e3, domE=1e3)}
QUEUE_LENGTHS = (64, 320, 512, 1025, 2049, 4097)
QUEUE_TARGETS = {64: 36, 320: 36, 512: 18, 1025: 18, 2049: 10, 4097: 10}
QUEUE_MIN_NODES = 40
QUEUE_SPACER = 80
QUEUE_MULTI = 6

_models, _ref_models, _refs = {}, {}, {}


def tier_of(M):
    return next(c for c in ALL_TIERS if 64 * c >= M)


def label_of(M):
    return f"rnd{M}"


def model(label):
    """label: "rnd<M>", with a suffix for the two extra families ("rnd1100 long", "rnd300 edges")."""
    M = int(label.split()[0][3:])
    if M not in _models:
        _models[M] = random_hmm(M, seed=MODEL_SEEDS.get(M, 7000 + M))
    return _models[M]


def _tables(hmm):
    t = hmm.transition_probabilities.astype(np.float64)
    mat, ins = hmm.match_emissions.astype(np.float64), hmm.insert_emissions.astype(np.float64)
    cmat = np.cumsum(mat / np.maximum(mat.sum(axis=1, keepdims=True), 1e-30), axis=1)
    cins = np.cumsum(ins / np.maximum(ins.sum(axis=1, keepdims=True), 1e-30), axis=1)
    ct = np.zeros((hmm.M + 1, 4))
    s3 = np.maximum(t[:, 0:3].sum(axis=1), 1e-30)
    ct[:, 0], ct[:, 1] = t[:, 0] / s3, (t[:, 0] + t[:, 1]) / s3
    ct[:, 2] = t[:, 3] / np.maximum(t[:, 3] + t[:, 4], 1e-30)
    ct[:, 3] = t[:, 5] / np.maximum(t[:, 5] + t[:, 6], 1e-30)
    return cmat, cins, ct


def emit_window(hmm, rng, first, last):
    """One sampled pass through nodes first..last of the model: bench.emit_from_model on the tables from node <first> on."""
    cmat, cins, ct = _tables(hmm)
    window = SimpleNamespace(M=last - first + 1, alphabet=hmm.alphabet)
    return bench.emit_from_model(window, rng, (cmat[first - 1:], cins[first - 1:], ct[first - 1:]))


def windows(M):
    """(name, first node, last node) of the three fragments."""
    n = min(M, FRAGMENT_NODES)
    mid = 32 * tier_of(M)
    a = min(max(1, mid - n // 2 + 1), M - n + 1)
    return (("first", 1, n), ("last", M - n + 1, M), ("boundary", a, a + n - 1))


def _rng(label, name):
    return np.random.default_rng([sum(label.encode()), sum(name.encode()), TARGET_SALTS.get((label, name), 0)])


def _flank(rng):
    return rng.integers(0, 20, size=int(rng.integers(0, MAX_FLANK + 1))).astype(np.uint8)


def _between_flanks(rng, fragment):
    return np.concatenate([_flank(rng), fragment, _flank(rng)]).astype(np.uint8)


_targets = {}


def targets(label):
    """[(name, residues)] of a label."""
    if label in _targets:
        return _targets[label]
    hmm = model(label)
    M = hmm.M
    named = []
    if label.endswith(" queue"):
        named = _queue_targets(label, hmm)
    elif label.endswith(" long"):
        rng = _rng(label, "full")
        named.append((f"{label}_full".replace(" ", "_"), _between_flanks(rng, emit_window(hmm, rng, 1, M))))
    elif label.endswith(" edges"):
        rng = _rng(label, "noflanks")
        named.append(("edges_noflanks", emit_window(hmm, rng, 1, M).astype(np.uint8)))
        rng = _rng(label, "degenerate")
        seq = _between_flanks(rng, emit_window(hmm, rng, 1, M))
        hit = rng.random(len(seq)) < 0.10
        seq[hit] = rng.choice([26, 21, 23], size=int(hit.sum()))                  # X, B, Z
        named.append(("edges_degenerate", seq))
        rng = _rng(label, "star")
        named.append(("edges_star", np.concatenate([_flank(rng), emit_window(hmm, rng, 1, M), [27]]).astype(np.uint8)))
    else:
        for name, first, last in windows(M):
            rng = _rng(label, name)
            named.append((f"{label}_{name}", _between_flanks(rng, emit_window(hmm, rng, first, last))))
    _targets[label] = named
    return named


def queue_windows(M):
    """(name, first node, last node) of the single-fragment targets of "rnd<M> queue", shortest first."""
    top = min(M, FRAGMENT_NODES) if M <= 1025 else 120
    mid = 32 * tier_of(M)
    out = []
    for t, n in enumerate(np.linspace(QUEUE_MIN_NODES, top, QUEUE_TARGETS[M]).round().astype(int)):
        n = int(n)
        if t % 3 == 0:
            a = M - n + 1                                                    # ends at node M
        elif t % 3 == 1:
            a = min(max(1, mid - n // 2 + 1), M - n + 1)                     # across nodes 32 C and 32 C + 1
        else:
            a = 1 + (7919 * (t + 1)) % (M - n + 1)                           # anywhere
        out.append((f"q{t:02d}", a, a + n - 1))
    return out


def _queue_targets(label, hmm):
    M = hmm.M
    named = []
    for name, first, last in queue_windows(M):
        rng = _rng(label, name)
        named.append((f"rnd{M}_{name}", _between_flanks(rng, emit_window(hmm, rng, first, last))))
    rng = _rng(label, "multi")
    wins = queue_windows(M)
    parts = [_flank(rng)]
    for f in range(QUEUE_MULTI):                                             # lengths from both ends of the range, mixed
        _, first, last = wins[(f * 7 + 3) % len(wins)]
        parts += [emit_window(hmm, rng, first, last), rng.integers(0, 20, size=QUEUE_SPACER)]
    parts[-1] = _flank(rng)
    named.append((f"rnd{M}_multi", np.concatenate(parts).astype(np.uint8)))
    return named


BATCH_FRAGMENTS = {300: 26, 310: 9, 320: 1, 100: 5}      # single-fragment targets per query; M = 300 gets one more with four fragments
BATCH_NODES = {300: (60, 150), 310: (60, 150), 320: (320, 320), 100: (60, 100)}
BATCH_SILENT = 200                                       # a query with no fragment in the block
_batch = []


def batch_case():
    """(models, [(name, residues)]): five queries for one batched search against one block -- three of one nodes-per-lane
    class (M = 300, 310, 320: C = 5) with about 30, 9 and 1 envelopes, one of another class (M = 100) and one that hits
    nothing.  The one envelope of M = 320 is the whole model, the class's longest by a factor of two: the slabs of the
    other two jobs are sized by it and not by their own fragments of 60 to 150 nodes (shortest first per query; one target
    holds four fragments of the first model)."""
    if not _batch:
        named = []
        for M, n in BATCH_FRAGMENTS.items():
            hmm = model(label_of(M))
            for t, nodes in enumerate(np.linspace(*BATCH_NODES[M], n).round().astype(int)):
                rng = _rng("batch", f"b{M}_{t}")
                first = 1 + (7919 * (t + 1)) % (M - int(nodes) + 1)
                named.append((f"b{M}_{t:02d}", _between_flanks(rng, emit_window(hmm, rng, first, first + int(nodes) - 1))))
        hmm = model(label_of(300))
        rng = _rng("batch", "four")
        parts = [_flank(rng)]
        for first, last in ((1, 90), (151, 300), (40, 180), (200, 300)):
            parts += [emit_window(hmm, rng, first, last), rng.integers(0, 20, size=QUEUE_SPACER)]
        parts[-1] = _flank(rng)
        named.append(("b300_four", np.concatenate(parts).astype(np.uint8)))
        _batch.append(([model(label_of(M)) for M in (300, 310, 320, 100, BATCH_SILENT)], named))
    return _batch[0]


TIER_LABELS = tuple(label_of(M) for M in TIER_LENGTHS)
EXTRA_LABELS = ("rnd1100 long", "rnd300 edges")
LABELS = TIER_LABELS + EXTRA_LABELS
QUEUE_LABELS = tuple(f"rnd{M} queue" for M in QUEUE_LENGTHS)


def pipeline_options(label):
    return dict(PIPELINE_OPTIONS.get(label, {}))


def search_block(hmm, named):
    """The targets among 20 background sequences."""
    from conftest import synthetic_block
    return easel.DigitalSequenceBlock(hmm.alphabet, list(block(hmm.alphabet, named)) + list(synthetic_block(20, 200, seed=hmm.M)))


def block(alphabet, named):
    return easel.DigitalSequenceBlock(alphabet, [easel.DigitalSequence(alphabet, name=n, sequence=s) for n, s in named])


# ---- the float64 reference, once per (model, target, envelope)
def degeneracy(alphabet):
    import oracle_lib
    return oracle_lib.degeneracy_sets(alphabet.K)


def ref_model(key, hmm):
    """The reference's tables of a model, read from the product's optimized profile.  key: whatever names the model."""
    import dp_reference
    if key not in _ref_models:
        _ref_models[key] = dp_reference.RefModel.from_oprofile(plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400))
    return _ref_models[key]


def reference(key, hmm, name, seq, ienv, jenv):
    import envelope_reference
    slot = (key, name, int(ienv), int(jenv))
    if slot not in _refs:
        _refs[slot] = envelope_reference.envelope(ref_model(key, hmm), seq, int(ienv), int(jenv), degeneracy(hmm.alphabet))
    return _refs[slot]
