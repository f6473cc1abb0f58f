"""p7x_calibrate_batch where its first tests (tests/test_gpu_calibrate.py) do not go: models whose samples overflow a filter
(the device's redraw path, alone and inside a batch), gap-rich and alignment-built models on both sides of every staging
threshold of the three kernels, four-letter alphabets and a second background, a second chunk of 1,024 models, more seeds
than resident streams are kept, two leases at once -- and the Forward scores against the float64 reference.

The references are calibration_cases.own_stream (the oracle's filters and the host seams of the redraw rule, checked by
tests/test_host_calibrate_reference.py) and calibration_cases.forward_reference.  Every raw result comes from
plan7._calibrate(oms, want_scores=True).  A model's entry -- its profile, own_stream, p7x_filters_batch on the same final
stream and its calibration alone -- is made once and shared by the tests."""
import ctypes as C
import sys
import threading

import numpy as np
import pytest

import calibration_cases as cc
from pyhmmer_amd import _lib, easel, plan7
from test_gpu_calibrate import FWD_TOL, TAU_MARGIN
from test_gpu_dp_reference import DEVICE_FACTOR, REL_SCORE
from test_host_builder import LENGTHS, N, fit, sample
from test_host_calibrate_reference import MEASURED

pytestmark = pytest.mark.gpu


def say(line):
    print("[calibrate-edges] " + line, file=sys.stderr)


def resident_block(abc, stream):
    """The 600 samples of a stream as a resident block for p7x_filters_batch (as test_gpu_calibrate.world builds it)."""
    lens = np.concatenate([np.full(N, L, np.int32) for L in LENGTHS])
    offs = np.zeros(3 * N, np.int64)
    flat = [np.array([255], np.uint8)]
    pos = 1
    for st in range(3):
        for i in range(N):
            offs[st * N + i] = pos
            flat += [sample(stream, st, i), np.array([255], np.uint8)]
            pos += LENGTHS[st] + 1
    return plan7.SequenceDatabase.from_packed(abc, np.concatenate(flat), offs, lens, device=0)


class Entry:
    pass


_entries, _blocks = {}, {}


def entry(oracle, name, hmm, uniform=False):
    """Everything the tests compare of one model under one background, computed once: own (calibration_cases.own_stream),
    par (p7x_filters_batch on own.stream: xJ, xC, Forward), tau_spread = |tau(oracle) - tau(oracle's scores with par's
    Forward)|, and ev / raw of the model calibrated alone."""
    key = (name, uniform)
    if key in _entries:
        return _entries[key]
    e = Entry()
    e.name, e.hmm, e.bg = name + ("/uniform" if uniform else ""), hmm, cc.background_of(hmm, uniform)
    e.om = plan7.OptimizedProfile(hmm, e.bg, 100)
    e.own = cc.own_stream_of(oracle, name, hmm, uniform)
    assert e.own.status == 0 and not e.own.ovf.any(), e.name
    bkey = (hmm.alphabet.type_code, e.own.stream.tobytes())
    if bkey not in _blocks:
        _blocks[bkey] = resident_block(hmm.alphabet, e.own.stream)
    got = _blocks[bkey].filters(e.om, msv=True, viterbi=True, forward=True)
    e.par = dict(xJ=got["xJ"][:N].copy(), xC=got["xC"][N:2 * N].copy(), fwd=got["fwd"][2 * N:].astype(np.float32).copy())
    sc = e.own.sc.copy()
    sc[2] = e.par["fwd"]
    e.tau_spread = abs(float(fit(sc, None, e.own.mh)[1][4]) - float(e.own.ev[4]))
    ev, raw = plan7._calibrate([e.om], want_scores=True)
    e.ev, e.raw = ev[0].copy(), raw[0].copy()
    _entries[key] = e
    return e


def entries(oracle, models, uniform=False):
    return [entry(oracle, name, hmm, uniform) for name, hmm in models]


def check_raw(e, raw, cascade=True):
    """xJ and xC bit for bit own_stream's (and p7x_filters_batch's), no overflow code left; Forward finite, within FWD_TOL of
    the oracle (and equal to p7x_filters_batch's)."""
    assert np.array_equal(raw[0], e.own.raw[0]), (e.name, np.flatnonzero(raw[0] != e.own.raw[0])[:5])
    assert np.array_equal(raw[1], e.own.raw[1]), (e.name, np.flatnonzero(raw[1] != e.own.raw[1])[:5])
    assert int(raw[0].min()) >= 0 and int(raw[1].max()) < 32767, e.name
    fwd = raw[2].view(np.float32)
    assert np.all(np.isfinite(fwd)), e.name
    d = float(np.max(np.abs(fwd - e.own.sc[2])))
    assert d <= FWD_TOL, (e.name, d)
    if cascade:
        assert np.array_equal(raw[0], e.par["xJ"]) and np.array_equal(raw[1], e.par["xC"]), e.name
        assert np.array_equal(fwd, e.par["fwd"]), (e.name, float(np.max(np.abs(fwd - e.par["fwd"]))))


def check_parameters(what, es, evs):
    """mu (MSV, Viterbi) and the three lambda equal to the CPU fit of own_stream's scores; tau within TAU_MARGIN times the
    largest |tau(oracle) - tau(p7x_filters_batch's Forward)| over these models, measured here on each model's final stream."""
    worst = max(e.tau_spread for e in es)
    say(f"{what}: largest |tau(oracle) - tau(p7x_filters_batch)| over {len(es)} models: {worst:.3g}")
    for e, ev in zip(es, evs):
        assert np.array_equal(ev[[0, 1, 2, 3, 5]], e.own.ev[[0, 1, 2, 3, 5]]), (e.name, ev, e.own.ev)
        assert abs(float(ev[4]) - float(e.own.ev[4])) <= TAU_MARGIN * worst, (e.name, ev[4], e.own.ev[4], worst)


def stored(om):
    _lib.lib().p7x_oprofile_get_info(om._handle, C.byref(om._info))
    return om.evalue_parameters.as_vector()


# ------------------------------------------------------------------------------------------------ 1. overflow, alone
def test_every_overflow_model_alone(oracle):
    """The device's redraw path (cal_alone) ends on own_stream's stream: the table of tests/calibration_cases.py says which
    draws that takes -- a draw's number and not a kept sample's, MSV before Viterbi, a redraw across the stage boundary."""
    es = entries(oracle, cc.overflow_models())
    for e in es:
        assert e.own.skipped == cc.OVERFLOW_TABLE[e.name][1], e.name
        check_raw(e, e.raw)
    check_parameters("overflow models", es, [e.ev for e in es])
    for e in es:
        ev, _ = plan7._calibrate([e.om], want_scores=True)
        assert np.array_equal(ev[0], e.ev), e.name
        assert np.array_equal(stored(e.om), e.ev) and np.array_equal(e.hmm._evparam, e.ev), e.name


# ------------------------------------------------------------------------------------------------ 2. overflow, in a batch
def test_overflow_inside_a_batch(oracle):
    """Ordinary models keep the common stream and their row while a neighbour goes through the redraw path, which runs
    through record 0 of the batch's own buffers; the resident stream is the common one afterwards; twice the same bytes."""
    ov = {e.name: e for e in entries(oracle, cc.overflow_models())}
    a, b, c = entries(oracle, cc.ordinary_models())
    orders = ([a, ov["msv5"], b, ov["both"], ov["vit50half"], c, ov["vit199"]],
              [ov["vit199"], ov["msv5+msv6"], ov["vit50"], a, c, ov["both"], b])
    for es in orders:
        oms = [e.om for e in es]
        ev, raw = plan7._calibrate(oms, want_scores=True)
        for j, e in enumerate(es):
            assert np.array_equal(raw[j], e.raw) and np.array_equal(ev[j], e.ev), (j, e.name)
            assert np.array_equal(stored(e.om), e.ev), (j, e.name)
        e1, r1 = plan7._calibrate([a.om], want_scores=True)
        assert np.array_equal(r1[0], a.raw) and np.array_equal(e1[0], a.ev)
        assert not a.own.skipped                 # the common stream's result, checked against it in check_raw
        ev2, raw2 = plan7._calibrate(oms, want_scores=True)
        assert ev2.tobytes() == ev.tobytes() and raw2.tobytes() == raw.tobytes()
    for e in (a, b, c):
        check_raw(e, e.raw)


# ------------------------------------------------------------------------------------------------ 3. staging thresholds
@pytest.fixture(scope="module")
def staged(oracle):
    es = entries(oracle, cc.gappy_models(cc.gappy_gpu_lengths()) + cc.fixture_models())
    ev, raw = plan7._calibrate([e.om for e in es], want_scores=True)           # one batch
    return es, ev, raw


def test_gap_rich_models_on_both_sides_of_each_staging_threshold(staged):
    """Deletion corridors and hmmbuild's own transitions, where a wrong transition row changes the score: the models of one
    batch, against own_stream and against p7x_filters_batch on the same stream."""
    es, ev, raw = staged
    for j, e in enumerate(es):
        check_raw(e, raw[j])
        assert np.array_equal(raw[j], e.raw) and np.array_equal(ev[j], e.ev), e.name
        assert np.array_equal(stored(e.om), ev[j]) and np.array_equal(e.hmm._evparam, ev[j]), e.name
    check_parameters("gap-rich and fixture models", es, ev)


# ------------------------------------------------------------------------------------------------ 4. Forward, float64
REFERENCE_NAMES = (list(cc.OVERFLOW_TABLE) + [f"gappy{M}" for M in cc.GAPPY_GPU_M if M <= cc.REFERENCE_MAX_M]
                   + [f"{n}/{i}" if n == "RREFam" else n for n, i in cc.FIXTURE_MODELS])


def test_reference_covers_the_models_of_up_to_1025_nodes(oracle, staged):
    have = {e.name for e in entries(oracle, cc.overflow_models()) + staged[0] if e.hmm.M <= cc.REFERENCE_MAX_M}
    assert have == set(REFERENCE_NAMES) and {e.hmm.M for e in staged[0]} >= {64, 65, 1024, 1025}


@pytest.mark.parametrize("name", REFERENCE_NAMES)
def test_forward_against_the_float64_reference(oracle, staged, name):
    """All 200 Forward samples of a model of up to 1,025 nodes: |device - reference| <= max(DEVICE_FACTOR x the oracle's
    recorded distance, REL_SCORE |reference|) -- the device sums the same float32 terms in another association.  Printed
    beside the device's tau: the tau fitted from the reference's scores cast to float32 (nothing is asserted of it)."""
    e, = [e for e in entries(oracle, cc.overflow_models()) + staged[0] if e.name == name]
    ref = cc.forward_reference(e.om, e.own.stream)
    fwd = e.raw[2].view(np.float32).astype(np.float64)
    d = np.abs(fwd - ref)
    sc = e.own.sc.copy()
    sc[2] = ref.astype(np.float32)
    tau_ref = float(fit(sc, None, e.own.mh)[1][4])
    say(f"{e.name}: M = {e.hmm.M}, worst |device - float64| {float(d.max()):.2e} nat (oracle {MEASURED[e.name]:.1e}); "
        f"tau device {float(e.ev[4]):.7f}, from the float32-cast reference {tau_ref:.7f}, oracle {float(e.own.ev[4]):.7f}")
    bound = np.maximum(DEVICE_FACTOR * MEASURED[e.name], REL_SCORE * np.abs(ref))
    assert np.all(d <= bound), (e.name, int(np.argmax(d - bound)), float(d.max()))


# ------------------------------------------------------------------------------------------------ 5. alphabets, backgrounds
def test_nucleotide_alphabets_and_a_uniform_background(oracle, staged):
    """K = 4 emission rows staged (DNA and RNA: each its own resident stream, residues < 4), and the amino models of up to
    320 nodes under a uniform background, which keys a second resident stream; the two backgrounds in turn give each its
    own results every time."""
    nuc = entries(oracle, cc.nucleotide_models())
    for e in nuc:
        assert e.hmm.alphabet.K == 4 and int(e.own.stream.max()) < 4, e.name
    small = [(e.name, e.hmm) for e in staged[0] if e.hmm.M <= cc.UNIFORM_MAX_M]
    assert len(small) >= 3
    uni = entries(oracle, small, uniform=True)
    dft = entries(oracle, small)
    for what, es in (("DNA", nuc[:len(nuc) // 2]), ("RNA", nuc[len(nuc) // 2:]), ("uniform background", uni)):
        ev, raw = plan7._calibrate([e.om for e in es], want_scores=True)
        for j, e in enumerate(es):
            check_raw(e, raw[j])
            assert np.array_equal(raw[j], e.raw) and np.array_equal(ev[j], e.ev), e.name
            assert np.array_equal(stored(e.om), ev[j]), e.name
        check_parameters(what, es, ev)
    for u, d in zip(uni, dft):
        assert not np.array_equal(u.own.stream, d.own.stream) and not np.array_equal(u.raw, d.raw), u.name
    for turn in range(3):
        for es in (dft, uni):
            ev, raw = plan7._calibrate([e.om for e in es], want_scores=True)
            for j, e in enumerate(es):
                assert np.array_equal(raw[j], e.raw) and np.array_equal(ev[j], e.ev), (turn, e.name)


def test_mixed_alphabets_or_backgrounds_are_refused(oracle, staged):
    """P7X_EINVAL, and no profile's parameters change."""
    nuc = entries(oracle, cc.nucleotide_models())
    small = [(e.name, e.hmm) for e in staged[0] if e.hmm.M <= cc.UNIFORM_MAX_M]
    uni, dft = entries(oracle, small, uniform=True), entries(oracle, small)
    for es in ([dft[0], nuc[0]], [nuc[0], nuc[-1]], [dft[0], dft[1], uni[0]], [uni[0], dft[0]]):
        before = [stored(e.om) for e in es]
        assert all(np.array_equal(b, e.ev) for b, e in zip(before, es))
        handles = (C.c_void_p * len(es))(*[e.om._handle for e in es])
        ev = np.full((len(es), 6), 7.0, np.float32)
        assert _lib.lib().p7x_calibrate_batch(handles, len(es), 0, 42, ev.ctypes.data, None) == 11, [e.name for e in es]
        assert "one alphabet and one background" in _lib.last_error()
        with pytest.raises(ValueError):
            plan7._calibrate([e.om for e in es])
        assert all(np.array_equal(stored(e.om), b) for b, e in zip(before, es)) and np.all(ev == 7.0)


# ------------------------------------------------------------------------------------------------ 6. second chunk
def test_second_chunk_of_models(oracle):
    """1,025 entries: one past the 1,024 models of a launch set, so the last entry is a chunk of its own at an offset into
    the profiles and the results."""
    es = entries(oracle, cc.ordinary_models((1, 2, 63, 64, 65)))
    for e in es:
        check_raw(e, e.raw)
    pick = [i % 5 for i in range(1025)]
    ev, raw = plan7._calibrate([es[i].om for i in pick], want_scores=True)
    for j in (0, 1023, 1024):
        assert np.array_equal(raw[j], es[pick[j]].raw) and np.array_equal(ev[j], es[pick[j]].ev), j
    want_raw, want_ev = np.stack([es[i].raw for i in pick]), np.stack([es[i].ev for i in pick])
    bad = np.flatnonzero([not (np.array_equal(raw[j], want_raw[j]) and np.array_equal(ev[j], want_ev[j])) for j in range(1025)])
    assert bad.size == 0, bad[:10]


# ------------------------------------------------------------------------------------------------ 7. eviction
def test_more_seeds_than_resident_streams_are_kept(oracle):
    """Seed 42, nine other seeds (one more than the streams kept), seed 42 again: the stream that was dropped is made
    again and is the same; every seed has its own stream; seed 3's is the one the host draws."""
    (name, hmm), = cc.ordinary_models((65,))
    e = entry(oracle, name, hmm)
    first = plan7._calibrate([e.om], seed=42, want_scores=True)
    others = {s: plan7._calibrate([e.om], seed=s, want_scores=True) for s in range(1, 10)}
    last = plan7._calibrate([e.om], seed=42, want_scores=True)
    assert np.array_equal(first[1], last[1]) and np.array_equal(first[0], last[0]) and np.array_equal(first[1][0], e.raw)
    for s, (ev, raw) in others.items():
        assert not np.array_equal(raw[0], e.raw) and not np.array_equal(ev[0], e.ev), s
    assert len({raw.tobytes() for ev, raw in others.values()}) == 9
    own3 = cc.own_stream_of(oracle, name, hmm, seed=3)
    assert own3.status == 0
    ev3, raw3 = others[3]
    assert np.array_equal(raw3[0][:2], own3.raw)
    assert float(np.max(np.abs(raw3[0][2].view(np.float32) - own3.sc[2]))) <= FWD_TOL
    assert np.array_equal(ev3[0][[0, 1, 2, 3, 5]], own3.ev[[0, 1, 2, 3, 5]])
    sc = own3.sc.copy()
    sc[2] = resident_block(hmm.alphabet, own3.stream).filters(e.om, msv=False, forward=True)["fwd"][2 * N:].astype(np.float32)
    spread = abs(float(fit(sc, None, own3.mh)[1][4]) - float(own3.ev[4]))
    say(f"seed 3: |tau(oracle) - tau(p7x_filters_batch)| {spread:.3g}")
    assert np.array_equal(raw3[0][2].view(np.float32), sc[2])
    assert abs(float(ev3[0][4]) - float(own3.ev[4])) <= TAU_MARGIN * spread, (ev3[0][4], own3.ev[4], spread)
    assert np.array_equal(stored(e.om), e.ev)          # the last call left seed 42's parameters in the shared entry


# ------------------------------------------------------------------------------------------------ 8. two leases at once
def test_four_threads_calibrate_at_once(oracle, staged):
    """Four plain threads of this process, each with its own list of profiles (no profile in two lists), three calls each:
    the overflow models; the gap-rich and fixture models of up to 1,025 nodes; the DNA, the RNA and the uniform-background
    models (a batch each); 65 entries of ordinary models.  Every result is the sequential one."""
    nuc = entries(oracle, cc.nucleotide_models())
    ordinary = entries(oracle, cc.ordinary_models((1, 2, 63, 64, 65)))
    uni = entries(oracle, [(e.name, e.hmm) for e in staged[0] if e.hmm.M <= cc.UNIFORM_MAX_M], uniform=True)
    lists = [[entries(oracle, cc.overflow_models())],
             [[e for e in staged[0] if e.hmm.M <= cc.REFERENCE_MAX_M]],
             [nuc[:len(nuc) // 2], nuc[len(nuc) // 2:], uni],
             [[ordinary[i % 5] for i in range(65)]]]
    got, errors = {}, []

    def work(t):
        try:
            got[t] = [[plan7._calibrate([e.om for e in es], want_scores=True) for es in lists[t]] for rep in range(3)]
        except BaseException as err:          # reported by the main thread
            errors.append((t, repr(err)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(len(lists))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, batches in enumerate(lists):
        for rep in range(3):
            for es, (ev, raw) in zip(batches, got[t][rep]):
                for j, e in enumerate(es):
                    assert np.array_equal(raw[j], e.raw) and np.array_equal(ev[j], e.ev), (t, rep, j, e.name)
