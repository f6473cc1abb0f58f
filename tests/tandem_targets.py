"""Targets built from a model's own consensus (test input only): the inputs on which Backward leaves Forward's scale
factors behind, on which posterior decoding overflows, and ragged lengths around the Backward kernel's 64-row blocks.

Models: random_hmm(M, seed=M) for M = 40, 100, 300, 1100, 4200 -- tiers 1, 2, 5, 20 (the first that reads emissions through
L2) and 96 (the first that reads transitions through L2) of nodes per lane -- and the KR fixture; random_hmm(45) joins family
(b) as its smallest case (a whole copy of M = 40 scores 85 nats, below the overflow window).

(a) own scales, no overflow: two and four fragments consensus[a : a + n] (a spread over the model, in descending order)
    between 10-residue random spacers.  n is fixed per model so that the float64 reference's unihit score of every fragment alone lies in [45, 80] nats:
    ln 1e16 + 8 (Backward's xB test) and ln FLT_MAX - 8, a factor of 3,000 inside either threshold where float32 summation
    orders differ by 1e-5.  tests/test_host_dp_reference.py asserts the window.
(b) overflow: two and three copies of a piece whose reference score alone is >= 100 nats (ln FLT_MAX + 11).  The piece is the
    whole consensus where the target then stays within MAX_L residues, else the consensus' first PREFIX_NODES nodes (a
    whole copy of the long models is longer than MAX_L by itself; the condition on the score is what makes the case).
(c) edges: lengths 1, 2, 3, 63, 64, 65, 127, 128, 129 of random residues with fragment 0 of (a) embedded from position 20
    where it fits (from 63 on; KR's 65-node fragment from 127 on).

Every target has L <= MAX_L; a model's block holds 13 targets."""
import numpy as np

from conftest import load_hmms, random_hmm
from pyhmmer_amd import easel

MAX_L = 700
SPACER = 10
PREFIX_NODES = 120
RANDOM_M = (40, 100, 300, 1100, 4200)
MODEL_KEYS = tuple(f"rnd{M}" for M in RANDOM_M) + ("KR",)
OVERFLOW_KEYS = ("rnd45",) + tuple(k for k in MODEL_KEYS if k != "rnd40")
# nodes per fragment of family (a): the reference's unihit score of each of the four fragments alone, in nats, is in the
# comment (tests/test_host_dp_reference.py::test_family_a_fragments_score_inside_the_window asserts [45, 80])
FRAGMENT_NODES = {
    "rnd40": 32,         # 65.9 68.2 68.2 67.2
    "rnd100": 32,        # 68.2 63.9 71.0 67.4
    "rnd300": 32,        # 72.1 68.3 65.9 65.4
    "rnd1100": 32,       # 56.8 64.5 62.5 58.7
    "rnd4200": 32,       # 62.0 64.0 63.5 66.7
    "KR": 65,            # 53.6 63.4 62.4 63.1
}
RAGGED = (1, 2, 3, 63, 64, 65, 127, 128, 129)

_models = {}


def model(key):
    if key not in _models:
        _models[key] = load_hmms("KR")[0] if key == "KR" else random_hmm(int(key[3:]), seed=int(key[3:]))
    return _models[key]


def consensus(hmm):
    sym = hmm.alphabet.symbols
    return np.array([sym.index(c.upper()) for c in hmm.consensus], dtype=np.uint8)


def _rng(key, salt):
    return np.random.default_rng([sum(key.encode()), salt])


def _spacer(rng, n=SPACER):
    return rng.integers(0, 20, size=n).astype(np.uint8)


def fragments(key):
    """The four fragments of family (a): consensus[a : a + n], a = j (M - n) / 3 for j = 3, 2, 1, 0.  Descending, so that a
    later fragment of the target lies earlier in the model and no single pass through the model can chain two of them (in
    ascending order M = 40, 100, 300 and KR align the fragments as ONE domain with a run of deletes or inserts between them;
    Forward's scale factors then cover the whole of it and Backward never needs its own)."""
    hmm = model(key)
    n = FRAGMENT_NODES[key]
    cons = consensus(hmm)
    return [cons[a:a + n] for a in ((j * (hmm.M - n)) // 3 for j in (3, 2, 1, 0))]


def _tandem(rng, pieces):
    parts = [_spacer(rng)]
    for p in pieces:
        parts += [p, _spacer(rng)]
    return np.concatenate(parts)


def overflow_piece(key, copies):
    cons = consensus(model(key))
    return cons if copies * len(cons) + SPACER * (copies + 1) <= MAX_L else cons[:PREFIX_NODES]


def family_a(key):
    fr = fragments(key)
    return [(f"{key}_a2", _tandem(_rng(key, 2), fr[:2])), (f"{key}_a4", _tandem(_rng(key, 4), fr))]


def family_b(key):
    return [(f"{key}_b{c}", _tandem(_rng(key, 10 + c), [overflow_piece(key, c)] * c)) for c in (2, 3)]


def family_c(key):
    frag = fragments(key)[0] if key in FRAGMENT_NODES else None
    out = []
    for L in RAGGED:
        seq = _rng(key, 100 + L).integers(0, 20, size=L).astype(np.uint8)
        if frag is not None and L >= 20 + len(frag):
            seq[20:20 + len(frag)] = frag
        out.append((f"{key}_c{L}", seq))
    return out


_targets = {}


def targets(key, family):
    """[(name, residues)] of one family; the M = 4,200 model keeps the two shortest of each (the reference's cost is L x M)."""
    if (key, family) not in _targets:
        named = {"a": family_a, "b": family_b, "c": family_c}[family](key)
        if model(key).M >= 4200:
            named = sorted(named, key=lambda t: len(t[1]))[:2]
        _targets[(key, family)] = named
    return _targets[(key, family)]


def block(alphabet, named):
    return easel.DigitalSequenceBlock(alphabet, [easel.DigitalSequence(alphabet, name=n, sequence=s) for n, s in named])


# ---- the float64 reference on these targets, computed once per session and shared by the tests
_ref_models, _refs = {}, {}


def ref_model(key):
    """The reference's tables of a model, read from the product's optimized profile."""
    import dp_reference
    from pyhmmer_amd import plan7
    if key not in _ref_models:
        hmm = model(key)
        _ref_models[key] = dp_reference.RefModel.from_oprofile(plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400))
    return _ref_models[key]


def reference(key, name, seq, multihit, cells=False):
    import dp_reference
    slot = (key, name, bool(multihit), bool(cells))
    if slot not in _refs:
        other = (key, name, bool(multihit), True)
        _refs[slot] = _refs[other] if other in _refs else dp_reference.forward_backward(ref_model(key), seq, multihit, cells=cells)
    return _refs[slot]
