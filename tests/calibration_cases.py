"""Inputs and references of the calibration tests (test input only): the models that make p7x_calibrate_batch leave the
path its first tests walk -- a sample that overflows a filter, position-specific transitions, four-letter alphabets, a
second background -- and two references of what it must return for them.

own_stream restates, in plain Python over the ORACLE's filters and the two host seams (p7x_calibration_draw_of,
p7x_calibration_redraw), the rule the device path implements for a model whose sample overflows: throw the first
overflowed draw away, draw the rest of the stream again, score, and repeat.  forward_reference is the float64 log-space
Forward score (tests/dp_reference.py) of the 200 Forward samples, for which the oracle is a float32 engine like the device.

The host file (tests/test_host_calibrate_reference.py) and the GPU file (tests/test_gpu_calibrate_edges.py) build their
inputs here, so that they are the same ones."""
import hashlib

import numpy as np

import dp_reference as R
import gap_models
import long_models
from conftest import load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, plan7
from test_host_builder import N, fit, oracle_scores, sample, stream_of

MAX_ROUNDS = 64                 # cal_alone's
GENERATOR = 1                   # P7X_RNG_FAST, the one p7x_calibrate_batch draws with
REFERENCE_MAX_M = 1025          # forward_reference costs about 4 s per model there; longer models keep the oracle

# name -> (the first overflowed kept sample of every round, the skipped draws at the end): what the oracle gives on the CPU
OVERFLOW_TABLE = {
    "msv5": ([5], [5]),
    "vit50": ([250], [250]),
    "both": ([5, 249], [5, 250]),
    "msv5+msv6": ([5, 5], [5, 6]),
    "vit199": ([399], [399]),
    "vit50half": ([250], [250]),
}
# the smallest models on both sides of every staging threshold of the calibration kernels (nodes per lane C = 1 | 2,
# 16 | 20: Forward emissions, 32 | 48: MSV / Viterbi emissions, 64 | 96: Forward transitions, 128: the widest staged
# Viterbi transitions); 8,193 (C = 192, Viterbi transitions through L2) joins them where the library takes it
GAPPY_GPU_M = (64, 65, 1024, 1025, 2048, 2049, 4096, 4097, 8192)
GAPPY_HOST_M = (65, 320, 641)
GAPPY_SEED = 5
FIXTURE_MODELS = (("PF02826", 0), ("KR", 0), ("LuxC", 0), ("RREFam", 0), ("RREFam", 1))      # hmmbuild's own transitions
NUCLEOTIDE_M = (50, 64, 65, 129)
NUCLEOTIDE_SEED = 3
UNIFORM_MAX_M = 320


def amino():
    return easel.Alphabet.amino()


def overflow_models():
    """[(name, hmm)]: single-sequence models whose query is cut from the common stream (seed 42, the fast generator, amino,
    default background), so that a sample is the model's own query and saturates a filter."""
    abc = amino()
    bg = plan7.Background(abc)
    stream = stream_of(bg)
    queries = {
        "msv5": sample(stream, 0, 5),
        "vit50": sample(stream, 1, 50),
        "both": np.concatenate([sample(stream, 0, 5), sample(stream, 1, 50)]),
        "msv5+msv6": np.concatenate([sample(stream, 0, 5), sample(stream, 0, 6)]),
        "vit199": sample(stream, 1, 199),
        "vit50half": sample(stream, 1, 50)[:60],
    }
    builder = plan7.Builder(abc)
    return [(name, builder._model(easel.DigitalSequence(abc, name=name, sequence=np.ascontiguousarray(q, dtype=np.uint8)), bg))
            for name, q in queries.items()]


def ordinary_models(lengths=(64, 65, 300)):
    """Single-sequence models of i.i.d. background queries (tests/test_gpu_calibrate.py's recipe; the query of a length is
    the same whatever the other lengths asked for, so a name is one model): none overflows."""
    abc = amino()
    bg = plan7.Background(abc)
    f = bg.residue_frequencies.astype(np.float64)
    builder = plan7.Builder(abc)
    return [(f"ord{M}", builder._model(easel.DigitalSequence(abc, name=f"ord{M}", sequence=np.random.default_rng([77, M]).choice(abc.K, size=M, p=f / f.sum()).astype(np.uint8)), bg))
            for M in lengths]


def gappy_models(lengths):
    """gappy_hmm(M, 5); gap_models lists the tiers of up to 128 nodes per lane, so a model beyond 8,192 nodes is made with
    the tier of 192 added for the length of the call (as tests/test_gpu_long_models.py does)."""
    tiers = gap_models._TIERS
    gap_models._TIERS = tiers + tuple(c for c in long_models.NEW_TIERS if c not in tiers)
    try:
        return [(f"gappy{M}", gap_models.gappy_hmm(M, GAPPY_SEED)) for M in lengths]
    finally:
        gap_models._TIERS = tiers


def gappy_gpu_lengths():
    limit = int(_lib.lib().p7x_max_model_length())
    return GAPPY_GPU_M + ((8193,) if limit >= 8193 else ())


def fixture_models():
    return [(f"{name}/{i}" if name == "RREFam" else name, load_hmms(name)[i]) for name, i in FIXTURE_MODELS]


def nucleotide_models():
    return [(f"{kind}{M}", random_hmm(M, NUCLEOTIDE_SEED, abc))
            for kind, abc in (("dna", easel.Alphabet.dna()), ("rna", easel.Alphabet.rna())) for M in NUCLEOTIDE_M]


def background_of(hmm, uniform=False):
    return plan7.Background(hmm.alphabet, uniform=True) if uniform else plan7.Background(hmm.alphabet)


# ------------------------------------------------------------------------------------------------ the redraw rule
def redraw(bg, abc_type, seed, skipped):
    out = np.zeros(100000, dtype=np.uint8)
    bgf = np.ascontiguousarray(bg.residue_frequencies, dtype=np.float32)
    sk = np.asarray(skipped, dtype=np.int32)
    st = _lib.lib().p7x_calibration_redraw(int(abc_type), bgf.ctypes.data, int(seed), GENERATOR, sk.ctypes.data, len(sk), out.ctypes.data)
    assert st == 0, _lib.last_error()
    return out


def draw_of(kept, skipped):
    sk = np.asarray(skipped, dtype=np.int32)
    return int(_lib.lib().p7x_calibration_draw_of(int(kept), sk.ctypes.data, len(sk)))


def first_overflow(ovf):
    """The first overflowed kept sample (0 .. 399) in MSV-then-Viterbi order, or -1."""
    hit = np.flatnonzero(np.asarray(ovf).reshape(-1))
    return int(hit[0]) if len(hit) else -1


class OwnStream:
    """skipped: the draws thrown away; firsts: the kept sample that overflowed first in every round; stream: the final
    100,000 residues; raw: the oracle's xJ / xC [2][200]; sc: its float32 scores [3][200]; ovf: what still overflows
    (all zero unless the rounds ran out); status, ev: the fit of sc; mh: the model's summed match relative entropy."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def own_stream(oracle, hmm, bg, abc_type, seed=42):
    """The stream a model is calibrated on and what the oracle scores on it.  Start from the common stream; while a kept
    sample overflows its filter, add the DRAW that sample was (not its number among the kept ones) to the skipped draws and
    draw the stream again without them; give up after MAX_ROUNDS redraws, as the device path does."""
    op = oracle.OracleProfile(hmm, bg, 100)
    mh = _lib.lib().p7x_oprofile_match_relent(plan7.OptimizedProfile(hmm, bg, 100)._handle)
    stream = stream_of(bg, seed=seed, generator=GENERATOR, abc_type=abc_type)
    skipped, firsts = [], []
    sc, ovf, raw = oracle_scores(op, stream)
    for _ in range(MAX_ROUNDS):
        first = first_overflow(ovf)
        if first < 0:
            break
        firsts.append(first)
        skipped.append(draw_of(first, skipped))
        stream = redraw(bg, abc_type, seed, skipped)
        sc, ovf, raw = oracle_scores(op, stream)
    status, ev = fit(sc, ovf, mh)
    return OwnStream(skipped=skipped, firsts=firsts, stream=stream, raw=raw, sc=sc, ovf=ovf, status=status, ev=ev, mh=mh)


_own = {}


def own_stream_of(oracle, name, hmm, uniform=False, seed=42):
    """own_stream of a model of the lists above, computed once per (name, background, seed) and not to be changed."""
    key = (name, bool(uniform), int(seed))
    tables = model_digest(hmm)
    if key not in _own:
        _own[key] = (tables, own_stream(oracle, hmm, background_of(hmm, uniform), hmm.alphabet.type_code, seed))
    assert _own[key][0] == tables, f"two models are called {name}"
    return _own[key][1]


def model_digest(hmm):
    """What tells two models apart: alphabet, transitions and match emissions."""
    h = hashlib.sha1(bytes([hmm.alphabet.type_code]))
    h.update(np.ascontiguousarray(hmm.transition_probabilities, dtype=np.float32).tobytes())
    h.update(np.ascontiguousarray(hmm.match_emissions, dtype=np.float32).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ float64 Forward
_fwd = {}


def _fwd_key(om, stream):
    h = hashlib.sha1()
    h.update(np.ascontiguousarray(om.rfv).tobytes())
    h.update(np.ascontiguousarray(om.tfv).tobytes())
    h.update(np.ascontiguousarray(stream[80000:]).tobytes())
    return (om.M, h.hexdigest())


def forward_reference(om, stream):
    """Float64 multihit Forward scores (nats) of the 200 Forward samples of <stream> under the length model of 100 residues,
    from the profile's own float32 tables; computed once per (tables, samples)."""
    key = _fwd_key(om, stream)
    if key not in _fwd:
        rm = R.RefModel.from_oprofile(om)
        out = np.array([R.forward_backward(rm, sample(stream, 2, i), True, length=100, backward=False).fwd for i in range(N)])
        out.setflags(write=False)
        _fwd[key] = out
    return _fwd[key]
