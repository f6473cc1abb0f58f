"""hmmalign's float64 log-space path on the device (p7x_alignlog.hip) against its host twin (seam "host_align" = 1,
p7x_logdp.cpp) and the float64 reference, with the bounds of tests/test_host_align_logspace.py: every posterior within 2^-24
of the reference's, the trace optimal to within 2 L 2^-24.

Device and twin sum in different orders, in float64: the traces (st, k, i) must be the same -- a choice the two could take
differently is flagged by the kernel's guard and repeated by the twin -- and the float32 posteriors they round to may
differ by one unit in the last place of a value <= 1, 2^-23 at most."""
import ctypes as C
import io
import sys

import numpy as np
import pytest

import tandem_targets as T
from pyhmmer_amd import _lib, hmmer, plan7
from test_host_align_logspace import check_against_reference

pytestmark = pytest.mark.gpu

TWIN_BOUND = 2.0 ** -23
# rnd45: M < 64, one partly filled chunk of nodes, the smallest overflow case; rnd100: two chunks; KR: 262 nodes;
# rnd1100 and rnd4200: 18 and 66 chunks per row (20 and 96 nodes per lane in the scaled kernels)
DEVICE_KEYS = ("rnd45", "rnd100", "KR", "rnd1100", "rnd4200")


def _aligned(hmm, block, logspace=False, host=False, everything=False):
    if host:
        _lib.set_debug_option("host_align", 1)
    if everything:
        _lib.set_debug_option("align_logspace", 1)
    try:
        return plan7.TraceAligner(logspace=logspace).compute_traces(hmm, block)
    finally:
        _lib.set_debug_option("host_align", -1)
        _lib.set_debug_option("align_logspace", -1)


def _same_as_twin(named, dev, host):
    worst = 0.0
    for (name, _), d, h in zip(named, dev, host):
        assert d._logspace and h._logspace, name
        assert np.array_equal(d.st, h.st) and np.array_equal(d.k, h.k) and np.array_equal(d.i, h.i), name
        worst = max(worst, float(np.abs(d.posterior_probabilities - h.posterior_probabilities).max()))
    assert worst <= TWIN_BOUND, worst
    return worst


def _memory_stats():
    out = (C.c_int64 * 4)()
    assert _lib.lib().p7x_debug_memory_stats(0, out) == 0, _lib.last_error()
    return tuple(out)


@pytest.mark.parametrize("key", DEVICE_KEYS)
def test_device_path_against_twin_and_reference(key):
    """Family b and family a (own scales) under the flag, families a and c under the seam that sends everything through."""
    hmm = T.model(key)
    has_ac = key in T.FRAGMENT_NODES
    cases = [("flag", T.targets(key, "b") + (T.targets(key, "a") if has_ac else []), dict(logspace=True))]
    if has_ac:
        cases.append(("seam", T.targets(key, "a") + T.targets(key, "c"), dict(everything=True)))
    for label, named, how in cases:
        block = T.block(hmm.alphabet, named)
        dev = _aligned(hmm, block, **how)
        host = _aligned(hmm, block, host=True, **how)
        assert dev.nlogspace == host.nlogspace == len(named)
        worst = _same_as_twin(named, dev, host)
        e_pp, e_oa = check_against_reference(key, named, dev)
        ndev = sum(1 for t in dev if t._device)
        print(f"[align-logspace] device {key} {label}: {len(named)} sequences, {ndev} traces from the device, flagged "
              f"{dev.nlogspace_flagged}; worst |pp - twin| {worst:.2e}, |pp - reference| {e_pp:.2e}, optimal-accuracy shortfall "
              f"{e_oa:.2e} of its bound; {dev.rounds} rounds, workspace {dev.workspace_bytes / 1e6:.1f} MB", file=sys.stderr)
        assert ndev + dev.nlogspace_flagged == len(named)
        assert 2 * dev.nlogspace_flagged <= dev.nlogspace
        if label == "flag":
            assert any(t._device for (name, _), t in zip(named, dev) if "_b" in name), "no family-b trace came from the device"
        plan7.TraceAligner().align_traces(hmm, block, dev)


@pytest.mark.parametrize("key", ("rnd40", "KR"))
def test_ragged_lengths(key):
    """Lengths 1, 2, 3 and around one and two 64-row blocks, every one through the log kernel."""
    hmm = T.model(key)
    named = T.targets(key, "c")
    assert [len(s) for _, s in named] == list(T.RAGGED)
    block = T.block(hmm.alphabet, named)
    dev = _aligned(hmm, block, everything=True)
    host = _aligned(hmm, block, host=True, everything=True)
    assert dev.nlogspace == len(named)
    worst = _same_as_twin(named, dev, host)
    e_pp, e_oa = check_against_reference(key, named, dev)
    print(f"[align-logspace] device {key} ragged: flagged {dev.nlogspace_flagged} of {len(named)}; worst |pp - twin| {worst:.2e}, "
          f"|pp - reference| {e_pp:.2e}", file=sys.stderr)
    assert 2 * dev.nlogspace_flagged <= dev.nlogspace


def _mixed(copies=1):
    """fine, b2, b3, fine for KR: the fine ones are single-domain (family c, 128 and 129 residues) and stay on the scaled path."""
    c = dict(T.targets("KR", "c"))
    b = dict(T.targets("KR", "b"))
    one = [("KR_c128", c["KR_c128"]), ("KR_b2", b["KR_b2"]), ("KR_b3", b["KR_b3"]), ("KR_c129", c["KR_c129"])]
    return [(f"{n}.{r}", s) for r in range(copies) for n, s in one] if copies > 1 else one


def test_mixed_block_and_small_workspace():
    hmm = T.model("KR")
    named = _mixed()
    block = T.block(hmm.alphabet, named)
    with pytest.raises(OverflowError):
        _aligned(hmm, block)
    got = _aligned(hmm, block, logspace=True)
    assert [t._logspace for t in got] == [False, True, True, False] and got.nlogspace == 2
    alone = _aligned(hmm, T.block(hmm.alphabet, [named[0], named[3]]))
    assert got[0] == alone[0] and got[3] == alone[1]
    host = _aligned(hmm, block, logspace=True, host=True)
    _same_as_twin(named[1:3], got[1:3], host[1:3])
    # 256 tandems need 1.5 GB of slabs at once: under a budget of 1 GB the same traces in more rounds, and the buffers go
    # back to the pool (a second call changes nothing in the pool's books)
    many = _mixed(copies=128)
    big_block = T.block(hmm.alphabet, many)
    big = _aligned(hmm, big_block, logspace=True)
    _lib.set_debug_option("align_workspace_gb", 1)
    try:
        small = _aligned(hmm, big_block, logspace=True)
        before = _memory_stats()
        again = _aligned(hmm, big_block, logspace=True)
        after = _memory_stats()
    finally:
        _lib.set_debug_option("align_workspace_gb", -1)
    print(f"[align-logspace] mixed block x 128: default budget {big.rounds} rounds, {big.workspace_bytes / 1e9:.2f} GB; 1 GB budget "
          f"{small.rounds} rounds, {small.workspace_bytes / 1e9:.2f} GB; flagged {big.nlogspace_flagged} of {big.nlogspace}", file=sys.stderr)
    assert small.rounds > big.rounds and small.workspace_bytes <= 1 << 30
    assert small == big and again == small
    assert before == after
    for r in range(0, 128, 37):
        assert all(big[4 * r + j] == got[j] for j in range(4)), r


def test_hmmalign_writes_pp_lines_for_the_tandems():
    hmm = T.model("KR")
    block = T.block(hmm.alphabet, _mixed())
    msa = hmmer.hmmalign(hmm, block, logspace=True)
    buf = io.BytesIO()
    msa.write(buf, "stockholm")
    text = buf.getvalue().decode()
    rows = {line.split()[1] for line in text.splitlines() if line.startswith("#=GR") and line.split()[2] == "PP"}
    assert {"KR_b2", "KR_b3"} <= rows, rows
    assert "#=GC PP_cons" in text
    with pytest.raises(OverflowError):
        hmmer.hmmalign(hmm, block)
