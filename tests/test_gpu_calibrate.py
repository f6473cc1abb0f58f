"""p7x_calibrate_batch on the device: raw scores of the resident stream against the oracle and against p7x_filters_batch (the
wave-per-target kernels the cascade already runs), results independent of the batch's composition, and the fitted parameters
against the CPU path (oracle scores + the same fit)."""
import numpy as np
import pytest

from pyhmmer_amd import _lib, easel, plan7
from test_host_builder import LENGTHS, N, OFFSETS, fit, oracle_scores, sample, stream_of

pytestmark = pytest.mark.gpu

TIERS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 96, 128)      # P7X_NODE_TIERS: M <= 64 C
# 1, 2, the first lane boundary, the last model of every tier and the first of the next, 2049, the longest model
LENGTHS_M = sorted({1, 2, 63, 64, 65, 2049, 8192} | {64 * c for c in TIERS[:-1]} | {64 * c + 1 for c in TIERS[:-1]})
FWD_TOL = 2e-3          # nats: DESIGN 3.3, fwd_kernel against the oracle
# tau's bound is measured where the test runs: the largest |tau(oracle scores) - tau(p7x_filters_batch scores)| over LENGTHS_M --
# the reference and the parent's kernels, never the new one -- times two (another summation order may be as far away again).
# On the MI355X the largest difference seen was 3.8e-6, at M = 8,192: four units in the last place of a float near -10.
TAU_MARGIN = 2.0


@pytest.fixture(scope="module")
def world(libp7x, oracle):
    abc = easel.Alphabet.amino()
    bg = plan7.Background(abc)
    f = bg.residue_frequencies.astype(np.float64)
    rng = np.random.default_rng(77)
    builder = plan7.Builder(abc)
    stream = stream_of(bg)
    hmms = [builder._model(easel.DigitalSequence(abc, name=f"q{M}", sequence=rng.choice(abc.K, size=M, p=f / f.sum()).astype(np.uint8)), bg)
            for M in LENGTHS_M]
    oms = [plan7.OptimizedProfile(h, bg, 100) for h in hmms]
    ev, raw = plan7._calibrate(oms, device=0, seed=42, want_scores=True)            # one batch mixing every tier
    # the same 600 sequences as a resident block for p7x_filters_batch
    lens = np.concatenate([np.full(N, L, np.int32) for L in LENGTHS])
    offs = np.zeros(3 * N, np.int64)
    flat = [np.array([255], np.uint8)]
    pos = 1
    for st in range(3):
        for i in range(N):
            offs[st * N + i] = pos
            flat += [sample(stream, st, i), np.array([255], np.uint8)]
            pos += LENGTHS[st] + 1
    db = plan7.SequenceDatabase.from_packed(abc, np.concatenate(flat), offs, lens, device=0)
    cpu, par = [], []
    for h, om in zip(hmms, oms):
        mh = _lib.lib().p7x_oprofile_match_relent(om._handle)
        sc, ovf, xraw = oracle_scores(oracle.OracleProfile(h, bg, 100), stream)
        assert not ovf.any()
        cpu.append(dict(sc=sc, raw=xraw, ev=fit(sc, ovf, mh)[1], mh=mh))
        got = db.filters(om, msv=True, viterbi=True, forward=True)
        par.append(dict(xJ=got["xJ"][:N].copy(), xC=got["xC"][N:2 * N].copy(), fwd=got["fwd"][2 * N:].astype(np.float32).copy()))
    return dict(abc=abc, bg=bg, hmms=hmms, oms=oms, ev=ev, raw=raw, cpu=cpu, par=par)


def test_raw_scores_against_the_oracle_and_the_cascade_kernels(world):
    """xJ and xC bit for bit the oracle's and p7x_filters_batch's; Forward within DESIGN 3.3's tolerance of the oracle and equal
    to p7x_filters_batch.  The calibration kernels and the cascade kernels (msv_wave_kernel, vit_kernel, fwd_kernel) run one row
    body each (p7x_waverows.hpp), so their equality compares two users of it; the oracle pins both."""
    for M, raw, cpu, par in zip(LENGTHS_M, world["raw"], world["cpu"], world["par"]):
        assert np.array_equal(raw[0], cpu["raw"][0]) and np.array_equal(raw[0], par["xJ"]), M
        assert np.array_equal(raw[1], cpu["raw"][1]) and np.array_equal(raw[1], par["xC"]), M
        fwd = raw[2].view(np.float32)
        assert np.all(np.isfinite(fwd)), M
        d = float(np.max(np.abs(fwd - cpu["sc"][2])))
        assert d <= FWD_TOL, (M, d)
        assert np.array_equal(fwd, par["fwd"]), (M, float(np.max(np.abs(fwd - par["fwd"]))))


def test_results_do_not_depend_on_the_batch(world):
    """Every model alone, and a batch of 65 (one past 64 models), give the 600 scores of the mixed batch."""
    oms, raw, ev = world["oms"], world["raw"], world["ev"]
    for i, om in enumerate(oms):
        e1, r1 = plan7._calibrate([om], want_scores=True)
        assert np.array_equal(r1[0], raw[i]) and np.array_equal(e1[0], ev[i]), LENGTHS_M[i]
    pick = [i % 12 for i in range(65)]                      # M = 1 .. 321: five tiers, every model several times
    e65, r65 = plan7._calibrate([oms[i] for i in pick], want_scores=True)
    for j, i in enumerate(pick):
        assert np.array_equal(r65[j], raw[i]) and np.array_equal(e65[j], ev[i]), (j, LENGTHS_M[i])
    assert plan7._calibrate([]).shape == (0, 6)


def test_parameters_against_the_cpu_path(world):
    """mu (MSV, Viterbi) and lambda identical to the CPU path: integer scores, the same fit code.  tau within twice the largest
    difference between the oracle-scored and the p7x_filters_batch-scored fits over these models (3.8e-6 on the MI355X, so
    7.6e-6).  The parameters are stored in the profile and in the HMM it was made from."""
    worst = 0.0
    for M, om, h, cpu, par in zip(LENGTHS_M, world["oms"], world["hmms"], world["cpu"], world["par"]):
        sc = cpu["sc"].copy()
        sc[2] = par["fwd"]
        worst = max(worst, abs(float(fit(sc, None, cpu["mh"])[1][4]) - float(cpu["ev"][4])))
    print(f"largest |tau(oracle) - tau(p7x_filters_batch)| over {len(LENGTHS_M)} models: {worst:.3g}")
    for M, om, h, ev, cpu in zip(LENGTHS_M, world["oms"], world["hmms"], world["ev"], world["cpu"]):
        assert np.array_equal(ev[[0, 1, 2, 3, 5]], cpu["ev"][[0, 1, 2, 3, 5]]), (M, ev, cpu["ev"])
        assert abs(float(ev[4]) - float(cpu["ev"][4])) <= TAU_MARGIN * worst, (M, ev[4], cpu["ev"][4], worst)
        assert np.array_equal(om.evalue_parameters.as_vector(), ev) and np.array_equal(h._evparam, ev), M


def test_no_device_and_bad_arguments(world):
    om = world["oms"][0]
    handles = (__import__("ctypes").c_void_p * 1)(om._handle)
    ev = np.zeros(6, np.float32)
    assert _lib.lib().p7x_calibrate_batch(handles, 1, 9999, 42, ev.ctypes.data, None) == 100          # P7X_ENODEVICE
