"""hmmalign on the device (p7x_align.hip) against the host twin in upstream's order (test seam "host_align" = 1, itself
pinned byte for byte to HMMER's own hmmalign output by tests/test_host_align.py).

Traces, PP lines and PP_cons must be identical: the kernel flags every optimal-accuracy choice on the trace that lies within
its near-tie guard and every posterior within the guard of a printed digit's boundary, and the host twin repeats exactly
those sequences; a PP_cons column near a digit boundary is averaged again over host-twin posteriors.  The float posteriors
themselves agree to PP_TOL."""
import io
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, hmmer, plan7

pytestmark = pytest.mark.gpu

PP_TOL = 2e-5          # |device - host| of a float posterior (another summation order in Forward / Backward; measured <= 7.5e-6)


def _stockholm(msa) -> bytes:
    buf = io.BytesIO()
    msa.write(buf, "stockholm")
    return buf.getvalue()


def _host_traces(hmm, block):
    _lib.set_debug_option("host_align", 1)
    try:
        return plan7.TraceAligner().compute_traces(hmm, block)
    finally:
        _lib.set_debug_option("host_align", -1)


def _check_device_share(traces, block, label, max_flagged=0.5):
    """The hot path is the kernel: the traces come from it, the host twin repeats only what it flagged (on the proteome at
    most half; profiles/r07_align.txt has the measured shares)."""
    nonempty = sum(1 for s in block if len(s))
    ndev = sum(1 for t in traces if t._device)
    assert ndev == traces.ndevice and ndev + traces.nflagged == nonempty, label
    assert ndev > 0 and traces.nflagged <= max_flagged * nonempty, (label, ndev, traces.nflagged)
    return ndev


def _compare(hmm, block, label, max_flagged=0.5):
    aligner = plan7.TraceAligner()
    dev = aligner.compute_traces(hmm, block)
    host = _host_traces(hmm, block)
    assert len(dev) == len(host) == len(block)
    ndev = _check_device_share(dev, block, label, max_flagged)
    assert host.ndevice == 0 and host.rounds == 0
    worst = 0.0
    for idx, (d, h) in enumerate(zip(dev, host)):
        assert np.array_equal(d.st, h.st) and np.array_equal(d.k, h.k) and np.array_equal(d.i, h.i), (label, block[idx].name)
        if len(d.st):
            worst = max(worst, float(np.abs(d.posterior_probabilities - h.posterior_probabilities).max()))
    assert worst <= PP_TOL, (label, worst)
    md = aligner.align_traces(hmm, block, dev, all_consensus_cols=True)
    mh = aligner.align_traces(hmm, block, host, all_consensus_cols=True)
    assert md.alignment == mh.alignment, label
    assert md.posterior_probabilities == mh.posterior_probabilities, label
    assert md.pp_consensus == mh.pp_consensus, label
    print(f"[align] {label}: M={hmm.M} n={len(block)} device traces {ndev} flagged->host {dev.nflagged} "
          f"max |dpp| {worst:.2e}", file=sys.stderr)
    return dev


def test_golden_on_the_device(models):
    hmm = models["LuxC"][0]
    with easel.SequenceFile(GOLDEN / "seqs" / "LuxC.faa", digital=True, alphabet=hmm.alphabet) as sf:
        seqs = sf.read_block()
    msa = hmmer.hmmalign(hmm, seqs, trim=True)
    assert _stockholm(msa) == (GOLDEN / "msa" / "LuxC.hmmalign.sto").read_bytes()
    untrimmed = _stockholm(hmmer.hmmalign(hmm, seqs))
    _lib.set_debug_option("host_align", 1)
    try:
        assert untrimmed == _stockholm(hmmer.hmmalign(hmm, seqs))
    finally:
        _lib.set_debug_option("host_align", -1)
    traces = plan7.TraceAligner().compute_traces(hmm, seqs)
    _check_device_share(traces, seqs, "LuxC")


@pytest.mark.parametrize("name,index", [("PF02826", 0), ("Thioesterase", 0), ("KR", 0)] + [("RREFam", i) for i in range(10)])
def test_device_against_host_twin_on_the_proteome(models, proteome, name, index):
    hmm = models[name][index]
    assert max(len(s) for s in proteome) > 2000
    _compare(hmm, proteome, f"{name}[{index}] x proteome")


# one model per tier of nodes per lane (p7x_vitfwd.hip kCList) against a sample of the proteome with its longest sequences
@pytest.mark.parametrize("M", [40, 100, 150, 230, 300, 350, 500, 600, 700, 1000, 1200, 1500, 2000, 3000, 4000, 6000, 8000])
def test_every_tier_of_nodes_per_lane(proteome, M):
    order = np.argsort([-len(s) for s in proteome])
    pick = [int(i) for i in order[:3]] + list(range(0, len(proteome), 150))
    block = easel.DigitalSequenceBlock(proteome.alphabet, [proteome[i] for i in pick])
    # (a synthetic model against unrelated proteins: long flanks, many posteriors near a digit boundary, and a sample of 17
    # sequences -- the flagged share is higher and noisier than on the fixture models; measured 3-10 of 17)
    _compare(random_hmm(M, seed=M), block, f"random M={M}", max_flagged=0.75)


def test_small_workspace_budget_same_msa(models, proteome):
    """A 1 GB budget: the rounds run with fewer resident wavefronts (the workspace stays within the budget, also after a
    larger workspace went back to the pool) and give the same alignment."""
    hmm = models["KR"][0]
    block = easel.DigitalSequenceBlock(proteome.alphabet, list(proteome) * 4)
    aligner = plan7.TraceAligner()
    big = aligner.compute_traces(hmm, block)
    _lib.set_debug_option("align_workspace_gb", 1)
    try:
        small = aligner.compute_traces(hmm, block)
    finally:
        _lib.set_debug_option("align_workspace_gb", -1)
    print(f"[align] workspace default {big.workspace_bytes / 1e9:.2f} GB in {big.rounds} rounds, "
          f"budget 1 GB {small.workspace_bytes / 1e9:.2f} GB in {small.rounds} rounds", file=sys.stderr)
    assert small.workspace_bytes <= 1 << 30 < big.workspace_bytes
    assert small.rounds == big.rounds >= 2
    assert small == big
    want = aligner.align_traces(hmm, block, big, all_consensus_cols=True)
    assert _stockholm(aligner.align_traces(hmm, block, small, all_consensus_cols=True)) == _stockholm(want)


def test_sequence_alone_too_large_for_the_budget(proteome):
    """One sequence whose wavefront slabs alone exceed the budget is an error that names it, never a mis-alignment."""
    longest = max(proteome, key=len)
    block = easel.DigitalSequenceBlock(proteome.alphabet, [proteome[0], longest])
    _lib.set_debug_option("align_workspace_gb", 1)
    try:
        with pytest.raises(MemoryError):
            plan7.TraceAligner().compute_traces(random_hmm(8000, seed=8000), block)
    finally:
        _lib.set_debug_option("align_workspace_gb", -1)
    assert "sequence 1 (L = %d)" % len(longest) in _lib.last_error()
