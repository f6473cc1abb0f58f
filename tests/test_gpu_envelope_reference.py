"""The envelope kernel (env_kernel<C, G, Mode> of p7x_envkernel.hpp, the search's instantiations in p7x_envelope.hip) against the
float64 reference of tests/envelope_reference.py: every domain's envsc, domcorrection and oasc as the device reports them, and
the score, bias and accuracy the host derives from them, at the device's own envelope coordinates -- for every nodes-per-lane
tier (tests/envelope_targets.py), with the near-tie guard (G = true, the default) and without it (oa_guard = 0: G = false,
nothing repeated on the host), and for the fixture models on the fixture proteome.

No tolerance comes from the kernel's output.  The bound of each kernel output is DEVICE_FACTOR times what the ORACLE was
measured to differ from the reference on the same label (MEASURED_ENV of tests/test_host_envelope_reference.py: the device
sums the same float32 terms in another association), or, where the oracle happens to sit on the reference, what float32
cannot do better: 1e-6 |envsc|; Ld 2^-23 for domcorrection and oasc (a float32 running sum of Ld addends of magnitude about
1, each rounded once).  score, bias and accuracy: those bounds carried through finish_one's formulas (derived_check)."""
import sys

import numpy as np
import pytest

import envelope_targets as T
from conftest import load_hmms
from pyhmmer_amd import plan7
from test_host_envelope_reference import DEVICE_FACTOR, FIXTURES, MEASURED_ENV, NULL2_SUM_TOL, Worst, bounds, derived_check, fixture_hits

pytestmark = pytest.mark.gpu

GUARDS = [pytest.param(None, id="guard"), pytest.param(0.0, id="no-guard")]


def _check(label, key, hmm, db, named, oa_guard, opts, planted):
    if oa_guard is not None:
        opts = dict(opts, oa_guard=oa_guard)
    hits = plan7.Pipeline(hmm.alphabet, **opts).search_hmm(hmm, db)
    by_name = {h.name: h for h in hits}
    w = Worst()
    derived = np.zeros(3)
    ndom = 0
    for name, seq in named:
        h = by_name.get(name)
        if planted:
            assert h is not None and h.nclustered == 0 and len(h.domains) >= 1, (label, name, "not a hit of single-domain regions")
        for d in (h.domains if h is not None else ()):
            ndom += 1
            ref = T.reference(key, hmm, name, seq, d.env_from, d.env_to)
            clustered = h.nclustered > 0              # their correction is null2 by trace; envsc and oasc: the kernel's second round
            got = w.add(hmm, ref, d._rec.envsc, d._rec.domcorrection, d._rec.oasc, clustered)
            E = bounds(label, ref, DEVICE_FACTOR)
            print(f"[envelope-reference] {label} {name} {d.env_from}-{d.env_to} of {len(seq)}: " +
                  " ".join(f"{what} {got[what]:.2e} (bound {E[what]:.2e})" for what in got), file=sys.stderr)
            for what, v in got.items():
                assert v <= E[what], (label, name, what, v, E[what])
            derived = np.maximum(derived, [v or 0.0 for v in derived_check(d, ref, E, clustered)])
    redone = hits.guard_counts["oa_redone"]
    m = MEASURED_ENV[label]
    print(f"[envelope-reference] {label} oa_guard={'default' if oa_guard is None else oa_guard}: device {w.line()}; "
          f"oracle envsc {m['envsc']:.1e} corr {m['corr']:.1e} oasc {m['oasc']:.1e}; score {derived[0]:.2e} bias {derived[1]:.2e} bits, "
          f"accuracy {derived[2]:.2e}; {redone} of {ndom} checked domains' searches repeated on the host", file=sys.stderr)
    assert w.null2 <= NULL2_SUM_TOL
    if oa_guard is None:
        assert 2 * redone <= sum(len(h.domains) for h in hits), (redone, "the host repeated more than half of the envelopes")
    else:
        assert redone == 0
    return w


@pytest.mark.parametrize("oa_guard", GUARDS)
@pytest.mark.parametrize("label", T.LABELS)
def test_device_envelopes_against_the_reference(label, oa_guard):
    hmm = T.model(label)
    named = T.targets(label)
    db = plan7.SequenceDatabase(T.search_block(hmm, named))
    w = _check(label, label.split()[0], hmm, db, named, oa_guard, T.pipeline_options(label), planted=True)
    assert w.full >= len(named)


@pytest.mark.parametrize("oa_guard", GUARDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_device_envelopes_of_fixture_models_against_the_reference(name, oa_guard, proteome):
    """Every domain of every hit on the fixture proteome whose target is at most 1,500 residues."""
    hmm = load_hmms(name)[0]
    db = plan7.SequenceDatabase(proteome)
    named = fixture_hits(plan7.Pipeline(hmm.alphabet).search_hmm(hmm, db), proteome)
    w = _check(name, name, hmm, db, named, oa_guard, {}, planted=False)
    assert w.full >= 1
