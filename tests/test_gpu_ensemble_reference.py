"""The ensemble kernels (p7x_ensemble.hip: ens_forward_kernel<C>, ens_walk_kernel) against the float64 reference of
tests/ensemble_reference.py, on the cases of tests/ensemble_cases.py -- one model per tier of nodes per lane.

The records the Forward fill writes are compared for EVERY cell of the region, not only along the paths that were walked:
with float64 wherever the posterior is at least 1e-9 (bound: max(4 d_ref, 2^-21), d_ref measured on the upstream-order
host twin, never on the device; tests/test_host_ensemble_reference.py), and word for word with the device-order twin on all
cells.  The walks equal the twin's bit for bit, and the twin's very traces are held to float64 deviate by deviate in the
host module: together that pins the device's walk.  Its null2 sums are held to float64 null2 by trace over those paths."""
import numpy as np
import pytest

import ensemble_cases as EC
import ensemble_reference as ER
from pyhmmer_amd import plan7
from test_gpu_ensembles import _same_ensemble

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def db():
    return plan7.SequenceDatabase(EC.block(EC.NAMES))


def _device_records(db, name):
    c = EC.case(name)
    return plan7.ensemble_records(c.om, c.start, c.end, db=db, target=EC.NAMES.index(name), device=True)


@pytest.mark.parametrize("name", EC.NAMES)
def test_device_records_of_every_cell(db, name):
    """Every cell and row the fill writes -- the first node of a lane, whose predecessors come from the lane before, the rows
    after a rescale, the cells no walk visits: within the bound of float64 where the posterior is at least 1e-9, and the
    device-order twin's words everywhere, what the kernel leaves untouched (row 0, node 0) included."""
    reg = EC.reference(name)
    cells, rows, md = _device_records(db, name)
    dist = reg.threshold_distance(cells, rows, md)
    print(f"{name}: device {dist[ER.FLOOR]:.3e} d_ref {EC.d_ref(name):.3e} bound {EC.threshold_bound(name):.3e}; by floor {dist}")
    assert dist[ER.FLOOR] <= EC.threshold_bound(name)
    tc, tr, tm = EC.twin_records(name, EC.DEVICE)
    assert cells.shape == tc.shape and cells[1:, 1:].any()
    for what, got, want in (("cells", cells, tc), ("rows", rows, tr), ("md", md.view(np.uint32), tm.view(np.uint32))):
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError((name, what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("name", EC.NAMES)
def test_device_walks_and_null2_sums(db, name):
    """Four seeds: the device's ensemble is the device-order twin's bit for bit (and the twin's through the trace seam is the
    twin's through the ensemble seam); its null2 sums lie within the host module's bound of float64 null2 by trace over
    those paths."""
    c, t = EC.case(name), EC.NAMES.index(name)
    for seed in EC.EXACT_SEEDS:
        with EC.host_order(EC.DEVICE):
            _same_ensemble(db, c.om, t, c.start, c.end, seed=seed)
        status, dom, n2 = db.ensemble(c.om, t, c.start, c.end, seed=seed, device=True)
        twin = EC.twin_traces(name, seed, EC.DEVICE)
        assert status == 0 and np.array_equal(dom, twin[4])
        want = EC.null2_reference(name, seed, EC.DEVICE)
        d = np.abs(n2[1:] - want[1:])
        assert (d <= EC.null2_bound(name, want)[1:]).all(), (name, seed, float(d.max()))


@pytest.mark.parametrize("name", EC.NAMES)
def test_device_distribution(db, name):
    """25 seeds x 200 samples on the device: what its domain records alone tell -- r inside a domain, a domain starting /
    ending at r, the first domain's entry node, the last domain's last match node -- counted against the float64 marginals
    at six sigma, the rule and the pooling of the host module's test_distribution.  About 14,000 cells over the 32 cases (6,834 of them
    on the seven region-length cases): under 0.03 false alarms expected, and the seeds are fixed."""
    c, t, reg = EC.case(name), EC.NAMES.index(name), EC.reference(name)
    tally = ER.Tally(reg.marginals(), ER.NSAMPLES * len(EC.DIST_SEEDS), ER.DOM_FAMILIES)
    for seed in EC.DIST_SEEDS:
        status, dom, n2 = db.ensemble(c.om, t, c.start, c.end, seed=seed, device=True)
        assert status == 0
        tally.add_domains(dom)
    bad, cells = tally.violations()
    print(f"{name}: {cells} cells, {len(bad)} outside six sigma")
    assert not bad, bad[:10]
