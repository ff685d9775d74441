"""CPU checks behind tests/test_um_dist_win_gpu.py: the reference for a window stated apart from the layout
(tests/um_win_ref.py) on its own, the inputs of the GPU tests (they must hold reset cells, cells reached beyond
2*maxdist through later sources, and unreached cells, or a kernel that ignored the sweep-order rule would pass), the
chain test's precondition, and the declarations of sb_get_dist_um_win_* in the header.
"""
import os
import re

import numpy as np
import pytest

import um_setup_ref as ur
import um_win_ref as uw
from conftest import ROOT
from seabreeze_param_amd import hip

WIN_ENTRY_POINTS = [f"sb_get_dist_um_win_{p}{d}" for p in ("f64", "f32") for d in ("", "_dev")]


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("halo", [(0, 0), (3, 2), (7, 9)])
def test_helper_with_window_equal_to_halo_is_the_restatement(halo, prec):
    hi, hj = halo
    nx, ny = 45, 31
    dt = np.float64 if prec == 8 else np.float32
    lat, lon = ur.grid_named("dateline", nx, ny, dt, dlon=0.9, dlat=0.7)
    land, ice = ur.noise_mask(nx, ny, 5, dt)
    _, _, coast_l = ur.coast_of(land, ice, hi, hj)
    coast_l[:hj] = 1.0                                   # ghost sources: ignored by rule
    coast_l[:, :hi] = 1.0
    out = uw.sentinel_field(coast_l.shape, dt, hi, hj)
    for maxdist in (60.0, 900.0):
        a = uw.dist_win_literal(coast_l, land, lat, lon, hi, hj, hi, hj, maxdist, out=out)
        b = ur.dist_um_literal(coast_l, land, lat, lon, hi, hj, maxdist, out=out)
        assert a.dtype == b.dtype == dt and np.array_equal(a, b)


def test_helper_window_differs_from_halo():
    """A wider window reaches more cells, a narrower one fewer, whatever the layout's ghost width."""
    nx, ny, dt = 40, 30, np.float64
    lat, lon = ur.grid_named("west", nx, ny, dt)
    land = np.zeros((ny, nx), dt)
    coast_l = np.zeros((ny + 4, nx + 6), dt)
    coast_l[2 + 15, 3 + 20] = 1.0
    for wi, wj in ((0, 0), (1, 4), (9, 2), (30, 30)):
        f = uw.dist_win_literal(coast_l, land, lat, lon, 3, 2, wi, wj, 900.0)[2:2 + ny, 3:3 + nx]
        reached = f < 12000.0
        want = np.zeros((ny, nx), bool)
        want[max(15 - wj, 0):15 + wj + 1, max(20 - wi, 0):20 + wi + 1] = True
        assert np.array_equal(reached, want), (wi, wj)


def test_seven_islands_have_fifty_coast_cells():
    _, _, _, coast_l = uw.islands_case("dateline", np.float64)
    assert np.count_nonzero(coast_l) == 50


@pytest.mark.parametrize("grid", sorted(ur.GRIDS))
@pytest.mark.parametrize("win", [(113, 40), (40, 113)])
def test_seven_islands_hold_every_class_at_maxdist_30(grid, win):
    lat, lon, land, coast_l = uw.islands_case(grid, np.float64)
    _, reset, beyond, unreached = uw.field_classes(coast_l, land, lat, lon, *win, 30.0)
    counts = dict(reset=int(reset.sum()), beyond=int(beyond.sum()), unreached=int(unreached.sum()))
    print(grid, win, counts)
    assert counts["reset"] > 0 and counts["beyond"] > 0 and counts["unreached"] > 0, counts


@pytest.mark.parametrize("grid", sorted(ur.GRIDS))
def test_seven_islands_at_the_full_window(grid):
    lat, lon, land, coast_l = uw.islands_case(grid, np.float64)
    o, reset, _, unreached = uw.field_classes(coast_l, land, lat, lon, 113, 113, 180.0)
    assert reset.sum() == 0 and 0.9 < 1.0 - unreached.mean() < 1.0, (int(reset.sum()), float(unreached.mean()))


def test_chain_field_is_off_the_knife_edge():
    """The chain test compares diag steps fed by the library's field and by the reference's bit for bit: that needs the
    band test |cdist| <= maxdist to come out the same for both, so no reference distance may lie within the fields'
    tolerance of maxdist."""
    c = uw.chain_case()
    o, md = c["ref"], uw.CHAIN["maxdist"]
    assert np.min(np.abs(np.abs(o) - md)) > 1e-6
    h, ny, nx = uw.CHAIN["halo"], uw.CHAIN["ny"], uw.CHAIN["nx"]
    band = np.abs(o[h:h + ny, h:h + nx]) <= md
    assert 0.4 < band.mean() < 0.7 and (o[h:h + ny, h:h + nx] >= 12000.0).any()


def test_window_entry_points_declared():
    with open(os.path.join(ROOT, "include", "seabreeze_hip.h")) as f:
        hdr = f.read()
    for name in WIN_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
    m = re.search(r"^#define\s+SB_DIST_UM_MAX_WINDOW\s+(\d+)\s*$", hdr, re.M)
    assert m and hip.SB_DIST_UM_MAX_WINDOW == int(m.group(1)) == 255
    assert hasattr(hip.Context, "get_dist_um_win") and hasattr(hip.Context, "get_dist_um_win_dev")
