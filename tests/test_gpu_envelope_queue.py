"""The envelope kernel as a scheduler (env_kernel of p7x_envkernel.hpp, DeviceEnvelopeScorer::begin of p7x_envscore.hip): a
wavefront that takes one envelope after the other from its job's queue (atomicAdd on the cursor, then order[q], longest
first) through one workspace slab, jobs of one class merged into one launch (gridDim.y) with slabs sized for the class's
longest envelope, and a second call of a search on the buffers the first one used.  tests/test_gpu_envelope_reference.py
checks the kernel's arithmetic with one envelope per wavefront; here the test option env_blocks caps a job's blocks, so that
small inputs run the schedule a library search runs, and p7x_debug_env_plan (_lib.env_plan) says what was scheduled:
[0] begin calls with envelopes, [1] jobs, [2] envelopes, [3] launches, [4] wavefronts, [5] envelopes that came second or later
in their wavefront at the least, [6] jobs whose order is no identity, [7] the most jobs of one launch.

Two kinds of statement.  Against the float64 reference (tests/envelope_reference.py, tests/lt_envelope_reference.py), with the
bounds of tests/test_gpu_envelope_reference.py: DEVICE_FACTOR times what the ORACLE was measured to differ on the same label
(MEASURED_ENV, MEASURED_LT: profiles/r29_envelope_queue.md), or the float32 floors; no tolerance comes from the device.  And
the schedule does not show: the kernel has no arithmetic across envelopes, so the records of a search are the same floats
and strings under any cap -- an invariant, not a tolerance.  The queue's order does not depend on the cap, so a result filed
under the queue position q instead of the envelope order[q] lands in the same wrong place under every cap: the same targets
listed the other way round are searched too, and must give the same records.

profiles/r29_envelope_queue.md: the plan counters of every test, the device's distances next to their bounds, and the three
deliberately wrong builds these tests were run against once."""
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import envelope_targets as T
import lt_envelope_targets as LT
from conftest import load_hmms, synthetic_block
from pyhmmer_amd import _lib, easel, hmmer, plan7
from test_gpu_envelope_reference import GUARDS, _check
from test_host_envelope_reference import fixture_hits
from test_host_lt_envelope_reference import DEVICE_FACTOR as LT_DEVICE_FACTOR, hits_against_the_reference, oracle_case

pytestmark = pytest.mark.gpu


def env_waves(M):
    """env_waves(C) of p7x_kernels.hpp: wavefronts per block, 4 from C = 8 on (more than 448 nodes)."""
    return 4 if T.tier_of(M) >= 8 else 8


@contextmanager
def schedule(env_blocks):
    """Searches under env_blocks = n (None: nothing set) with the plan counters counting from zero; both put back."""
    try:
        _lib.env_plan(reset=True)
        if env_blocks is not None:
            _lib.set_debug_option("env_blocks", env_blocks)
        yield
    finally:
        _lib.set_debug_option("env_blocks", -1)
        _lib.env_plan(reset=True)


def say(line):
    print(f"[envelope-queue] {line}", file=sys.stderr)


def records(hits):
    """What a search reports, as floats and strings: equal under every schedule."""
    out = []
    for h in hits:
        for d in h.domains:
            a = d.alignment
            out.append((h.name, d.env_from, d.env_to, a.hmm_from, a.hmm_to, a.target_from, a.target_to,
                        d._rec.envsc, d._rec.domcorrection, d._rec.oasc, h.score, h.bias, d.score, d.bias,
                        a.hmm_sequence, a.identity_sequence, a.target_sequence, a.posterior_probabilities))
    return out, hits.guard_counts


def same_records(got, want, what):
    """(Compared in one order: a hit list is sorted by score, and two hits of one score may change places.)"""
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    for g, w in zip(sorted(got[0]), sorted(want[0])):
        assert g == w, (what, g, w)
    assert got[1] == want[1], (what, got[1], want[1])


def queue_was_run(plan, waves, least):
    """All but one envelope of every wavefront went through a slab another envelope had used ([5]; per job nenv - waves, so
    with one job envelopes - waves), at least <least> envelopes were queued, and the order was a real permutation."""
    assert plan[0] >= 1 and plan[2] >= least, plan
    assert plan[5] >= plan[2] - waves * plan[1] and plan[5] >= least - waves, (plan, waves)
    assert plan[6] >= 1, plan


def _options(label, oa_guard):
    opts = T.pipeline_options(label)
    return opts if oa_guard is None else dict(opts, oa_guard=oa_guard)


# ------------------------------------------------------------------------------------------------ a. the queue against the reference
@pytest.mark.parametrize("oa_guard", GUARDS)
@pytest.mark.parametrize("label", T.QUEUE_LABELS)
def test_queued_envelopes_against_the_reference(label, oa_guard):
    """One block per job: every wavefront takes several envelopes of different lengths, longest first, through one slab."""
    hmm = T.model(label)
    named = T.targets(label)
    db = plan7.SequenceDatabase(T.search_block(hmm, named))
    with schedule(1):
        w = _check(label, label.split()[0], hmm, db, named, oa_guard, T.pipeline_options(label), planted=True)
        plan = _lib.env_plan()
    say(f"{label} oa_guard={'default' if oa_guard is None else oa_guard} env_blocks=1: plan {plan}; device {w.line()}")
    assert w.full >= len(named)
    assert plan[1] == plan[0] == 1, plan                   # one job: [5] >= envelopes - env_waves(C)
    queue_was_run(plan, env_waves(hmm.M), w.n)


# ------------------------------------------------------------------------------------------------ b. the schedule does not show
@pytest.mark.parametrize("oa_guard", GUARDS)
@pytest.mark.parametrize("label", T.QUEUE_LABELS)
def test_the_schedule_does_not_show(label, oa_guard):
    """env_blocks = 1, 2 and unset -- and, because the queue's order is the same permutation under every cap, the same
    targets listed longest first, where the queue takes them in the order they come: the only search here in which queue
    position and envelope index are (nearly) the same number."""
    hmm = T.model(label)
    named = T.targets(label)
    db = plan7.SequenceDatabase(T.search_block(hmm, named))
    got, plans = {}, {}
    for cap in (1, 2, None):
        with schedule(cap):
            got[cap] = records(plan7.Pipeline(hmm.alphabet, **_options(label, oa_guard)).search_hmm(hmm, db))
            plans[cap] = _lib.env_plan()
    say(f"{label} oa_guard={'default' if oa_guard is None else oa_guard}: wavefronts {[plans[c][4] for c in (1, 2, None)]} "
        f"for {plans[1][2]} envelopes, queued behind another {[plans[c][5] for c in (1, 2, None)]}")
    assert len(got[None][0]) >= len(T.targets(label))
    assert plans[1][4] == env_waves(hmm.M) and plans[2][4] == 2 * env_waves(hmm.M) and plans[None][4] > plans[2][4], plans
    same_records(got[1], got[None], (label, "env_blocks = 1"))
    same_records(got[2], got[None], (label, "env_blocks = 2"))
    with schedule(1):
        turned = records(plan7.Pipeline(hmm.alphabet, **_options(label, oa_guard)).search_hmm(hmm, plan7.SequenceDatabase(T.search_block(hmm, named[::-1]))))
    same_records(turned, got[None], (label, "targets longest first, env_blocks = 1"))


# ------------------------------------------------------------------------------------------------ c. several jobs in one launch
def test_jobs_of_one_class_share_a_launch():
    """Five queries in one batched search: three of the class C = 5 with about 30, 9 and 1 envelopes (2, 2 and 1 blocks under
    env_blocks = 2: blocks past a job's own leave at once, the slab stride is the class's longest envelope's, every job has
    its cursor), one of another class, one without a hit.  Every query's records are those of the query searched alone with
    nothing set -- against the same targets in reverse, so that the lone search queues them in another order."""
    models, named = T.batch_case()
    db = plan7.SequenceDatabase(T.search_block(models[0], named))
    turned = plan7.SequenceDatabase(T.search_block(models[0], named[::-1]))
    alone = []
    for hmm in models:
        with schedule(None):
            alone.append(records(plan7.Pipeline(hmm.alphabet).search_hmm(hmm, turned)))
    with schedule(2):
        batched = [records(hits) for hits in hmmer.hmmsearch(models, db, batch=len(models))]
        plan = _lib.env_plan()
    say(f"batch of {len(models)} queries under env_blocks = 2: plan {plan}; domains alone {[len(a[0]) for a in alone]}")
    assert len(batched) == len(models)
    counts = [len(a[0]) for a in alone]
    assert counts[0] >= 25 and 5 <= counts[1] <= 16 and counts[2] == 1 and counts[3] >= 2 and counts[4] == 0, counts
    assert max(sum(1 for r in alone[0][0] if r[0] == name) for name in {r[0] for r in alone[0][0]}) >= 4      # the four-domain target
    assert plan[7] >= 3 and plan[1] >= 4 and plan[2] >= sum(counts), plan
    for hmm, got, want in zip(models, batched, alone):
        same_records(got, want, ("batched", hmm.M))


# ------------------------------------------------------------------------------------------------ d. the second round on used buffers
@pytest.mark.parametrize("oa_guard", GUARDS)
def test_second_round_on_the_buffers_of_the_first(oa_guard, proteome):
    """PF02826 on the fixture proteome: 38 envelopes, 8 of them clustered by the ensembles and scored by a second call."""
    hmm = load_hmms("PF02826")[0]
    db = plan7.SequenceDatabase(proteome)
    options = {} if oa_guard is None else dict(oa_guard=oa_guard)
    with schedule(None):
        default = plan7.Pipeline(hmm.alphabet, **options).search_hmm(hmm, db)
        want = records(default)
    named = fixture_hits(default, proteome)
    with schedule(1):
        w = _check("PF02826", "PF02826", hmm, db, named, oa_guard, {}, planted=False)
        plan = _lib.env_plan()
        got = records(plan7.Pipeline(hmm.alphabet, **options).search_hmm(hmm, db))
    say(f"PF02826 oa_guard={'default' if oa_guard is None else oa_guard} env_blocks=1: plan {plan}; device {w.line()}")
    assert w.full >= 1 and w.n > w.full                     # clustered envelopes among them
    assert plan[0] >= 2 and plan[5] >= 1, plan
    same_records(got, want, "PF02826 under env_blocks = 1")


# ------------------------------------------------------------------------------------------------ e. long-target mode
@pytest.mark.parametrize("oa_guard", GUARDS)
def test_queued_long_target_envelopes(oa_guard, oracle):
    """Every envelope has its own emission table (env_emis + it * stride) and its own out_orig slot: an index by queue
    position instead of by envelope gives another envelope's table, far outside the bounds."""
    label = LT.QUEUE_LABEL
    hmm = LT.model(label)
    _, wins, _ = oracle_case(oracle, label)
    options = {} if oa_guard is None else dict(oa_guard=oa_guard)
    search = lambda: next(hmmer.nhmmer(hmm, LT.block(label), window_length=LT.WINDOW_LENGTH, host_envelopes=2, **options))
    with schedule(None):
        want = records(search())
    with schedule(1):
        hits = search()
        plan = _lib.env_plan()
    w, derived = hits_against_the_reference(label, hits, wins, LT_DEVICE_FACTOR, line=lambda line: say(line))
    redone = hits.guard_counts["oa_redone"]
    say(f"{label} (long targets) oa_guard={'default' if oa_guard is None else oa_guard} env_blocks=1: plan {plan}; device {w.line()}; "
        f"score {derived[0]:.2e} bias {derived[1]:.2e} bits, accuracy {derived[2]:.2e}; {redone} of {w.n} repeated on the host")
    assert w.n >= len(LT.target(label)[1])
    if oa_guard is None:
        assert 2 * redone <= w.n, (redone, w.n, "the host repeated more than half of the envelopes")
    else:
        assert redone == 0
    queue_was_run(plan, env_waves(hmm.M), len(LT.target(label)[1]))
    same_records(records(hits), want, "long targets under env_blocks = 1")


# ------------------------------------------------------------------------------------------------ f. alignment mode
def test_queued_alignments():
    """hmmalign's instantiation: 24 sequences of mixed length, shortest first, through one block's slabs.  (The aligner sorts
    a round's sequences itself, longest first, and a round holds lengths within a factor of two: these are one round.)"""
    hmm = T.model("rnd320")
    seqs = []
    for n in range(12):
        rng = np.random.default_rng([24, n])
        seqs.append(np.concatenate([T.emit_window(hmm, rng, 1, hmm.M), rng.integers(0, 20, size=12 * n)]).astype(np.uint8))
    seqs += [np.asarray(s.sequence, dtype=np.uint8) for s in synthetic_block(12, 0, seed=24, lengths=np.linspace(300, 560, 12).astype(int))]
    seqs.sort(key=len)
    assert len(seqs) == 24 and len({len(s) for s in seqs}) >= 12 and 2 * len(seqs[0]) >= len(seqs[-1])
    block = easel.DigitalSequenceBlock(hmm.alphabet, [easel.DigitalSequence(hmm.alphabet, name=f"s{n:02d}", sequence=s) for n, s in enumerate(seqs)])
    aligner = plan7.TraceAligner()
    with schedule(None):
        want = aligner.compute_traces(hmm, block)
    with schedule(1):
        got = aligner.compute_traces(hmm, block)
        plan = _lib.env_plan()
    say(f"alignment mode, 24 sequences under env_blocks = 1: plan {plan}; device traces {got.ndevice}, flagged {got.nflagged}")
    assert got.ndevice == want.ndevice > 0 and got.nflagged == want.nflagged
    assert plan[0] == plan[1] == 1 and plan[2] == 24 and plan[4] == env_waves(hmm.M) and plan[5] == 24 - env_waves(hmm.M), plan
    assert len(got) == len(want) == 24
    for n, (g, t) in enumerate(zip(got, want)):
        assert np.array_equal(g.st, t.st) and np.array_equal(g.k, t.k) and np.array_equal(g.i, t.i), n
        assert np.array_equal(g.posterior_probabilities, t.posterior_probabilities), n
