"""The creation plan of the cascades' stream sets (p7x_debug_stream_plan: pure arithmetic, no device).

The library cannot know whether the runtime has four hardware queues or eight (p7x_device.hpp), so the plan's invariants
are stated modulo 4 and hold modulo 8 with them.  What the runtime does with a creation position was measured
(scripts/ubench/queue_probe, profiles/r10_queues.md): the first Q streams of a priority open queues 0 .. Q-1, every later
one at position p joins queue Q-1 - (p mod Q); queue_of() below restates that, and the invariants are checked on it too."""
import ctypes as C

import pytest


def queue_of(p, Q):
    return p if p < Q else Q - 1 - (p % Q)


@pytest.fixture(scope="module")
def plan(libp7x):
    hw = C.c_int32(-99)
    n = libp7x.p7x_debug_stream_plan(None, 0, C.byref(hw))
    assert n > 4 and hw.value >= -1
    buf = (C.c_int32 * n)()
    assert libp7x.p7x_debug_stream_plan(buf, n, None) == n
    v = list(buf)
    nsets, per_set, partner, nspacers = v[:4]
    assert n == 4 + nsets * per_set + nspacers
    sets = [v[4 + s * per_set: 4 + (s + 1) * per_set] for s in range(nsets)]
    return {"sets": sets, "partner": partner, "spacers": v[4 + nsets * per_set:], "per_set": per_set}


def test_the_plan_is_four_sets_of_eight_streams(plan):
    assert len(plan["sets"]) == 4 and plan["per_set"] == 8 and 0 <= plan["partner"] < 7
    for s in plan["sets"]:
        assert s == list(range(s[0], s[0] + 8))        # a set's streams are created one after the other, main first


def test_main_streams_are_pairwise_different_mod_4(plan):
    mains = [s[0] for s in plan["sets"]]
    assert len({m % 4 for m in mains}) == len(mains)
    assert len({m % 8 for m in mains}) == len(mains)
    for Q in (4, 8):
        assert len({queue_of(m, Q) for m in mains}) == len(mains)


def test_the_partner_is_on_the_main_streams_queue_of_four_and_on_another_of_eight(plan):
    for s in plan["sets"]:
        main, partner = s[0], s[1 + plan["partner"]]
        assert partner % 4 == main % 4 and partner % 8 != main % 8
        assert queue_of(partner, 4) == queue_of(main, 4) and queue_of(partner, 8) != queue_of(main, 8)


def test_every_set_covers_all_eight_residues(plan):
    for s in plan["sets"]:
        assert sorted(p % 8 for p in s) == list(range(8))
        assert sorted(queue_of(p, 8) for p in s) == list(range(8))
        assert sorted(queue_of(p, 4) for p in s) == [0, 0, 1, 1, 2, 2, 3, 3]


def test_no_position_is_used_twice_and_none_is_left_out(plan):
    used = [p for s in plan["sets"] for p in s] + plan["spacers"]
    assert len(set(used)) == len(used)
    assert sorted(used) == list(range(len(used)))      # the spacers are exactly the gaps: get_ctx creates them in this order


def test_every_stream_of_a_set_is_past_the_first_eight_positions(plan):
    """The first Q streams open the queues in ascending order, the later ones join them in descending order: only from
    position 8 on is the queue a function of the position modulo Q for four queues and for eight -- and stays one if the
    process created streams of the same priority before the library did."""
    assert min(p for s in plan["sets"] for p in s) >= 8
    for shift in range(0, 9):          # streams of that priority created before ours
        for Q in (4, 8):
            mains = [queue_of(s[0] + shift, Q) for s in plan["sets"]]
            assert len(set(mains)) == len(mains)
        for s in plan["sets"]:
            a, b = s[0] + shift, s[1 + plan["partner"]] + shift
            assert queue_of(a, 4) == queue_of(b, 4) and queue_of(a, 8) != queue_of(b, 8)
