"""The envelope kernel's long-target instantiation (env_kernel<C, true, EnvMode::LongTarget> of p7x_envkernel.hpp, launched by
p7x_longtarget.hip::envelopes() with a per-envelope odds table in the tier's lane-chunk layout) against the float64 reference of
tests/lt_envelope_reference.py: every hit's envsc (orig: Forward with the profile's own odds), domcorrection (orig minus
Forward with the adjusted odds) and oasc as the device reports them, and the score, bias and accuracy the host derives, at the
device's own envelope coordinates -- for every nodes-per-lane tier (tests/lt_envelope_targets.py), always through the device
(host_envelopes = 2: the library's own estimate keeps a handful of hits on the host workers), with the near-tie guard at its
default and with oa_guard = 0, where nothing is flagged and every number is the kernel's.

No tolerance comes from the kernel's output.  The bound of each kernel output is DEVICE_FACTOR times what the ORACLE was
measured to differ from the reference on the same label (MEASURED_LT of tests/test_host_lt_envelope_reference.py: the device
sums the same float32 terms in another association), or that module's float32 floor, whichever is larger; score, bias and
accuracy: those bounds carried through lt_window_hits' formula (derived_check)."""
import sys

import pytest

import lt_envelope_targets as T
from pyhmmer_amd import hmmer
from test_host_lt_envelope_reference import DEVICE_FACTOR, MEASURED_LT, hits_against_the_reference, oracle_case

pytestmark = pytest.mark.gpu

GUARDS = [pytest.param(None, id="guard"), pytest.param(0.0, id="no-guard")]


@pytest.mark.parametrize("oa_guard", GUARDS)
@pytest.mark.parametrize("label", T.LABELS)
def test_device_long_target_envelopes_against_the_reference(label, oa_guard, oracle):
    _, wins, _ = oracle_case(oracle, label)
    options = {} if oa_guard is None else dict(oa_guard=oa_guard)
    hits = next(hmmer.nhmmer(T.model(label), T.block(label), window_length=T.WINDOW_LENGTH, host_envelopes=2, **options))
    say = lambda line: print(f"[lt-envelope-reference] {line}", file=sys.stderr)
    w, derived = hits_against_the_reference(label, hits, wins, DEVICE_FACTOR, line=say)
    redone = hits.guard_counts["oa_redone"]
    m = MEASURED_LT[label]
    say(f"{label} C={T.ET.tier_of(T.model(label).M)} oa_guard={'default' if oa_guard is None else oa_guard}: device {w.line()}; "
        f"oracle orig {m['orig']:.1e} corr {m['corr']:.1e} oasc {m['oasc']:.1e}; score {derived[0]:.2e} bias {derived[1]:.2e} bits, "
        f"accuracy {derived[2]:.2e}; {redone} of {w.n} envelopes repeated on the host" +
        (f" ({', '.join(f'{k} {v}' for k, v in hits.guard_counts['oa_why'].items() if v)})" if redone else ""))
    assert w.n >= len(T.target(label)[1])              # three per tier label (two full-length copies for the extra labels)
    if oa_guard is None:
        assert 2 * redone <= w.n, (redone, w.n, "the host repeated more than half of the envelopes")
    else:
        assert redone == 0
