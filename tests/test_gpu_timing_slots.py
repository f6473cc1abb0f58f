"""TopHits.timings_ms by name (enum p7x_timing, include/p7x.h): relations that hold between the slots whatever the times
are, for two protein queries searched alone and as one batch, and the long-target meanings of the slots that nhmmer fills."""
import math

import pytest

from conftest import load_hmms
from pyhmmer_amd import hmmer
from test_host_longtarget import _read

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def searches(models, proteome):
    queries = [models["PF02826"][0], models["Thioesterase"][0]]
    batch = list(hmmer.hmmsearch(queries, proteome, devices=[0], batch=2))
    alone = [list(hmmer.hmmsearch([q], proteome, devices=[0]))[0] for q in queries]
    return queries, batch, alone


def check_relations(t):
    assert all(math.isfinite(v) and v >= 0 for v in t.values()), t
    assert t["total"] == t["stage1"] + t["stage2"]
    assert t["host_stage_busy"] == max(0.0, t["host_domaindef"] - t["ensemble_wait"] - t["envelope_wait"])
    assert t["stage1"] > 0 and t["msv"] > 0


def test_slots_of_a_query_alone(searches):
    queries, _, alone = searches
    for q, hits in zip(queries, alone):
        t = hits.timings_ms
        check_relations(t)
        assert (t["batch_queries"], t["msv_launch_lanes"], t["msv_launch_nodes"]) == (1, 1, q.M)


def test_slots_of_a_batch(searches):
    queries, batch, _ = searches
    for hits in batch:
        t = hits.timings_ms
        check_relations(t)
        assert t["batch_queries"] == 2 and t["msv_launch_lanes"] in (1, 2)
        nodes = {1: {q.M for q in queries}, 2: {sum(q.M for q in queries)}}[int(t["msv_launch_lanes"])]
        assert t["msv_launch_nodes"] in nodes


def test_stage_counts_do_not_depend_on_the_batch(searches):
    _, batch, alone = searches
    for b, a in zip(batch, alone):
        assert b.stage_counts == a.stage_counts and b.stage_counts["msv"] > 0


def test_long_target_meanings():
    hmm = load_hmms("bmyD")[0]
    hits = next(hmmer.nhmmer(hmm, _read("1390.SAMEA104415756.OFHT01000022.fna", hmm.alphabet)))
    t = hits.timings_ms
    assert t["msv_kernel"] > 0                            # the SSV scan kernels
    assert t["host_domaindef"] >= t["bias"] >= 0          # everything after the seeds holds the windows' device batches
