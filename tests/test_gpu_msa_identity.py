"""Pairwise identity on the device (p7x_msapair.hip) against its host twin (test seam "host_pairid" = 1).  Counts, link
decisions, the filter's walk and the clusters are all integers, so the kernel must give the twin's bytes whatever the tile
("pairid_tile"), the grid, the candidate block and the band; then the recorded cases through the device, and a model built
from a filtered alignment."""
import numpy as np
import pytest

from pyhmmer_amd import _lib, easel, plan7
import msa_identity_cases as ic
from test_host_msa_identity import AMINO, DNA, check_recorded_cases, luxc

pytestmark = pytest.mark.gpu

# the smallest shapes that cross every boundary: one row, one tile of 64 rows less one, exactly, one over, three tiles;
# a partial dword of columns, exactly one, one over; a partial chunk of 128 columns less one, exactly, one over; two chunks
# less one, exactly, one over; nine chunks
SHAPES = [(1, 1), (2, 3), (63, 4), (64, 5), (65, 63), (130, 64), (64, 65), (63, 255), (65, 256), (130, 257), (2, 1030), (65, 1030)]


def on(host, tile, call, *args):
    _lib.set_debug_option("host_pairid", 1 if host else -1)
    _lib.set_debug_option("pairid_tile", tile)
    try:
        return call(*args)
    finally:
        _lib.set_debug_option("host_pairid", -1)
        _lib.set_debug_option("pairid_tile", -1)


def same_bytes(dev, twin, what):
    """Tuples of arrays (and counts): the same types, shapes and bytes."""
    dev, twin = (x if isinstance(x, tuple) else (x,) for x in (dev, twin))
    assert len(dev) == len(twin), what
    for d, t in zip(dev, twin):
        if isinstance(d, np.ndarray):
            assert d.dtype == t.dtype and d.shape == t.shape and d.tobytes() == t.tobytes(), what
        else:
            assert d == t, what


def orders_of(ax, amino):
    msa = ic.as_msa(ax, amino)
    return {p: msa._filter_order(p, seed=5) for p in ("origorder", "conscover", "random")}


@pytest.mark.parametrize("n,alen", SHAPES)
def test_kernel_equals_the_twin(n, alen):
    amino = (n + alen) % 2 == 0
    abc = AMINO if amino else DNA
    ax = ic.generated(n, alen, amino, seed=1)
    orders = orders_of(ax, amino)
    rows_a, rows_b = np.arange(n)[::-1], np.arange(0, n, 2)
    twin_counts = on(True, -1, ic.lib_counts, ax, abc.type_code)
    assert np.array_equal(twin_counts[0], ic.pair_counts(ax, abc.K)[0])
    for tile in (-1, 7, 32):
        same_bytes(on(False, tile, ic.lib_counts, ax, abc.type_code), twin_counts, (n, alen, tile, "counts"))
        for t in ic.THRESHOLDS:
            what = (n, alen, tile, t)
            same_bytes(on(False, tile, ic.lib_links, ax, abc.type_code, t, rows_a, rows_b),
                       on(True, tile, ic.lib_links, ax, abc.type_code, t, rows_a, rows_b), what + ("links",))
            for pref, order in orders.items():
                dev, stats = on(False, tile, ic.lib_filter, ax, abc.type_code, order, t)
                assert stats[3] == 1
                same_bytes(dev, on(True, tile, ic.lib_filter, ax, abc.type_code, order, t)[0], what + (pref,))
            dev = on(False, tile, ic.lib_linkage, ax, abc.type_code, t)
            assert dev[2][3] == 1
            same_bytes(dev[:2], on(True, tile, ic.lib_linkage, ax, abc.type_code, t)[:2], what + ("clusters",))


def test_deep_alignment_through_several_blocks():
    """1,500 x 300: two candidate blocks of 1,024 rows at the default tile, sixteen of 96 at a tile of 48; the filter keeps a
    strict subset and rows of every block; the clusters come back in bands."""
    n, alen = 1500, 300
    ax = ic.generated(n, alen, True, seed=2)
    order = orders_of(ax, True)["conscover"]
    twin, _ = on(True, -1, ic.lib_filter, ax, AMINO.type_code, order, 0.62)
    kept = int(twin.sum())
    assert 1 < kept < n
    pos = np.flatnonzero(twin[order])                                        # where in the order the kept rows are
    assert pos.min() < 96 and pos.max() >= 1024 and len(set((pos // 96).tolist())) > 4
    for tile in (-1, 48):
        dev, stats = on(False, tile, ic.lib_filter, ax, AMINO.type_code, order, 0.62)
        assert dev.tobytes() == twin.tobytes() and stats[3] == 1 and stats[1] > 0, tile
    again, _ = on(False, -1, ic.lib_filter, ax, AMINO.type_code, order, 0.62)
    assert again.tobytes() == twin.tobytes()
    twin_cl = on(True, -1, ic.lib_linkage, ax, AMINO.type_code, 0.62)
    assert 1 < twin_cl[1] < n
    for tile in (-1, 48):
        dev_cl = on(False, tile, ic.lib_linkage, ax, AMINO.type_code, 0.62)
        assert dev_cl[0].tobytes() == twin_cl[0].tobytes() and dev_cl[1] == twin_cl[1], tile


def test_a_second_run_gives_the_same_bytes():
    ax = ic.generated(130, 257, False, seed=1)
    first = on(False, -1, ic.lib_counts, ax, DNA.type_code)
    same_bytes(on(False, -1, ic.lib_counts, ax, DNA.type_code), first, "counts")
    first = on(False, -1, ic.lib_links, ax, DNA.type_code, 0.62, np.arange(130), np.arange(130))
    same_bytes(on(False, -1, ic.lib_links, ax, DNA.type_code, 0.62, np.arange(130), np.arange(130)), first, "links")


def test_recorded_cases_on_the_device():
    check_recorded_cases()


def test_model_of_a_filtered_alignment():
    msa = luxc().identity_filter(0.62, preference="origorder")
    assert len(msa.sequences) == 9 and msa._pair_stats[3] == 1
    hmm, _, _ = plan7.Builder(AMINO).build_msa(msa, plan7.Background(AMINO))
    assert hmm.nseq == 9
