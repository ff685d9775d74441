"""CPU preconditions of tests/test_um_tile_gpu.py: the rule the tile calls implement -- sources are the coast cells of the
tile AND of the in-domain ghost cells within the window, taken on the extended rectangle as if it were a domain
(tests/um_tile_ref.py) -- gives the whole-domain field cell for cell, the sweep-order reset included, while the
interior-only rule of sb_get_dist_um_win_* applied per tile does not; and the sparse case holds the classes of cell that
make this a test."""
import numpy as np
import pytest

import um_setup_ref as ur
import um_tile_ref as ut
import um_win_ref as uw


def _model_equals_whole(case, cuts, win, maxdist):
    whole = ut.whole_dist(case["coast"], case["land"], case["lat"], case["lon"], *win, maxdist)
    for t in ut.tiles(cuts):
        x0, x1, y0, y1 = t
        got = ut.tile_dist(case["coast"], case["land"], case["lat"], case["lon"], t, *win, maxdist)
        bad = np.count_nonzero(got != whole[y0:y1, x0:x1])
        assert bad == 0, (t, bad)
    return whole


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("cuts", sorted(ut.SPARSE_CUTS))
def test_model_is_the_whole_domain_field_sparse(cuts, prec):
    c = ut.SPARSE
    _model_equals_whole(ut.sparse_case(prec), ut.SPARSE_CUTS[cuts], c["win"], c["maxdist"])


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("grid", sorted(ur.GRIDS))
def test_model_is_the_whole_domain_field_dense(grid, prec):
    c = ut.DENSE
    whole = _model_equals_whole(ut.dense_case(grid, prec), c["cuts"], c["win"], c["maxdist"])
    assert (np.abs(whole) < 12000.0).mean() > 0.5


def test_model_is_the_whole_domain_field_at_km_scale():
    c = ut.ISLANDS
    _model_equals_whole(ut.islands_case(), c["cuts"], c["win"], c["maxdist"])


def test_all_sides_at_the_edge_is_the_whole_domain():
    c, g = ut.SPARSE, ut.sparse_case(8)
    t = (0, c["nx"], 0, c["ny"])
    assert ut.sides_of(t, c["nx"], c["ny"]) == 15
    _model_equals_whole(g, ((0, c["nx"]), (0, c["ny"])), (6, 6), c["maxdist"])


def test_cut_and_edges_model():
    """cut() brings the neighbours' cells and `fill` beyond the domain; the edges model keeps `fill` beyond ext"""
    a = np.arange(30 * 20, dtype=np.float64).reshape(20, 30)
    f = ut.cut(a, 0, 10, 5, 12, 3, 2, -1.0)
    assert f.shape == (11, 16) and (f[:, :3] == -1.0).all() and np.array_equal(f[:, 3:], a[3:14, 0:13])
    e = ut.tile_edges(a, (0, 10, 5, 12), 3, 2, 1, 1, -1.0)
    assert (e[0] == -1.0).all() and (e[:, 14:] == -1.0).all() and np.array_equal(e[1:10, 3:14], a[4:13, 0:11])
    assert ut.sides_of((0, 10, 5, 12), 30, 20) == ut.WEST and ut.sides_of((20, 30, 12, 20), 30, 20) == ut.EAST | ut.NORTH


@pytest.mark.parametrize("cuts", sorted(ut.SPARSE_CUTS))
def test_interior_only_rule_depends_on_the_cut(cuts):
    """sb_get_dist_um_win_*'s rule per tile -- a rank sees its own coast cells only -- changes cells of every tile of the
    equal cut (each has a cut side), and more than a tenth of the domain under either cut: the inputs are such that the GPU
    test cannot pass on interior sources.  (Of the unequal cut's small tiles one lies out of every coast's reach.)"""
    c, g = ut.SPARSE, ut.sparse_case(8)
    whole = ut.whole_dist(g["coast"], g["land"], g["lat"], g["lon"], *c["win"], c["maxdist"])
    total, touched = 0, 0
    for t in ut.tiles(ut.SPARSE_CUTS[cuts]):
        x0, x1, y0, y1 = t
        assert ut.sides_of(t, c["nx"], c["ny"]) != 15
        own = ut.tile_dist(g["coast"], g["land"], g["lat"], g["lon"], t, *c["win"], c["maxdist"], reach=(0, 0))
        n = np.count_nonzero(own != whole[y0:y1, x0:x1])
        assert n >= 1 or cuts != "equal", t
        total += n
        touched += n >= 1
    assert total > c["nx"] * c["ny"] // 10 and touched >= 7


def test_sparse_case_holds_every_class():
    """at least one sweep-order reset cell (so cells that hold 12000), and one tile whose only sources are ghost cells.
    Under a 40 x 9 window every cell of this mask has a coast cell in its window -- its 12000s are all resets; cells
    with no source in the window are held by the km-scale case, in every tile."""
    c, g = ut.SPARSE, ut.sparse_case(8)
    ref, reset, _, unreached = uw.field_classes(g["coast"], g["land"], g["lat"], g["lon"], *c["win"], c["maxdist"])
    assert reset.sum() >= 1 and np.array_equal(ref >= 12000.0, reset) and unreached.sum() == 0
    k, gi = ut.ISLANDS, ut.islands_case()
    reach = np.zeros(gi["coast"].shape, bool)
    for y, x in np.argwhere(gi["coast"] > 0):
        reach[max(y - k["win"][1], 0):y + k["win"][1] + 1, max(x - k["win"][0], 0):x + k["win"][0] + 1] = True
    for x0, x1, y0, y1 in ut.tiles(k["cuts"]):
        assert (~reach[y0:y1, x0:x1]).any() and reach[y0:y1, x0:x1].any()
    t = ut.GHOST_ONLY_TILE
    assert t in ut.tiles(ut.SPARSE_CUTS["ghost"]) and ut.sides_of(t, c["nx"], c["ny"]) == 0
    x0, x1, y0, y1 = t
    ex0, ex1, ey0, ey1 = ut.extended(t, c["nx"], c["ny"], *c["win"])
    assert not (g["coast"][y0:y1, x0:x1] > 0).any() and (g["coast"][ey0:ey1, ex0:ex1] > 0).any()
    got = ut.tile_dist(g["coast"], g["land"], g["lat"], g["lon"], t, *c["win"], c["maxdist"])
    assert (np.abs(got) < 12000.0).all()
    # the window reaches beyond the neighbouring tile of the unequal cut: sources from two tiles away
    xs = ut.SPARSE_CUTS["unequal"][0]
    assert xs[2] - xs[1] < c["win"][0] and xs[2] - xs[1] < 64
