"""CPU checks of the UM-layout coast setup's restatement (tests/um_setup_ref.py) and of the C ABI's declarations.

The literal form (the UM's scatter in sweep order with the reset inside the loop) and the vectorised form (early /
late minima over coast sources) must agree on small grids, halos and maxdist values -- including inputs on which the
sweep-order reset makes the field differ from a plain minimum.  The GPU tests then use the vectorised form at sizes the
literal one cannot reach.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import um_setup_ref as ur
from conftest import ROOT

UM_ENTRY_POINTS = [f"sb_{fn}_um_{p}{d}" for fn in ("get_edges", "get_dist") for p in ("f64", "f32") for d in ("", "_dev")]


@pytest.mark.parametrize("grid", sorted(ur.GRIDS))
@pytest.mark.parametrize("shape,halo", [((23, 17), (1, 1)), ((40, 29), (3, 2)), ((31, 36), (2, 5)), ((45, 30), (7, 4)),
                                        ((20, 15), (0, 0))])
@pytest.mark.parametrize("prec", [8, 4])
def test_literal_and_vectorised_agree(grid, shape, halo, prec):
    nx, ny = shape
    hi, hj = halo
    dt = np.float64 if prec == 8 else np.float32
    lat, lon = ur.grid_named(grid, nx, ny, dt, dlon=0.9, dlat=0.7)     # coarse: distances up to a few hundred km
    for maker, seed in ((ur.noise_mask, 3), (ur.sparse_mask, 4)):
        land, ice = maker(nx, ny, seed, dt)
        _, _, coast_l = ur.coast_of(land, ice, hi, hj)
        for maxdist in (60.0, 180.0, 900.0):
            a = ur.dist_um_literal(coast_l, land, lat, lon, hi, hj, maxdist)
            b = ur.dist_um_vectorised(coast_l, land, lat, lon, hi, hj, maxdist)
            assert a.dtype == b.dtype == dt
            # one code path per target up to the rounding of the min over c (the same c values): identical
            assert np.array_equal(a, b), f"{grid} {shape} {halo} {maxdist}: {np.count_nonzero(a != b)} cells differ"


def test_reset_changes_the_field():
    """The 2*maxdist reset at the target's sweep position throws away early sources' distances that later ones do not
    restore: the UM field differs from a plain minimum (and the literal form shows the same difference)."""
    nx, ny, hi, hj = 40, 30, 6, 6
    lat, lon = ur.grid_named("dateline", nx, ny, dlon=0.9, dlat=0.7)
    land, ice = ur.sparse_mask(nx, ny, 4, np.float64)
    _, _, coast_l = ur.coast_of(land, ice, hi, hj)
    um = ur.dist_um_literal(coast_l, land, lat, lon, hi, hj, 180.0)
    plain = ur.dist_plain_min(coast_l, land, lat, lon, hi, hj, 180.0)
    diff = um != plain
    assert diff.any()
    # the reset only ever throws a distance away: where the fields differ the UM's is farther (or 12000), and the plain
    # minimum there is one the reset could discard (beyond 2*maxdist) or a later source's
    assert np.all(np.abs(um[diff]) > np.abs(plain[diff]))
    assert np.any(um[diff] == 12000.0) and np.all(np.abs(plain[diff]) > 0.5)
    assert np.array_equal(um, ur.dist_um_vectorised(coast_l, land, lat, lon, hi, hj, 180.0))


def test_generator_deterministic_and_covers_branches():
    for name in ur.GRIDS:
        a = ur.grid_named(name, 64, 48)
        b = ur.grid_named(name, 64, 48)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    lat, lon = ur.grid_named("dateline", 200, 150)
    assert (lon > 180).any() and (lon <= 180).any()             # both branches of l1 and l2
    assert lon.min() >= 0.0 and lon.max() < 360.0
    lat, lon = ur.grid_named("west", 200, 150)
    assert (lon < 0).all()
    lat, lon = ur.grid_named("polar", 200, 150)
    assert lat.max() > 89.5 and np.ptp(lon) > 300.0
    # float32 coordinates are the float64 ones rounded
    lat32, lon32 = ur.grid_named("dateline", 200, 150, np.float32)
    assert np.array_equal(lat32, ur.grid_named("dateline", 200, 150)[0].astype(np.float32))


def test_edges_um_uses_ghost_ring():
    """A land cell only in the ghost ring makes the interior cells next to it coast; one further out does not."""
    nx, ny, hi, hj = 12, 9, 3, 2
    lf = np.zeros((ny + 2 * hj, nx + 2 * hi))
    ice = np.zeros_like(lf)
    lf[hj - 1, hi + 5] = 1.0                                     # the ring above the first interior row
    co = ur.edges_um(lf, ice, hi, hj)
    assert co[hj, hi + 4:hi + 7].tolist() == [1.0, 1.0, 1.0] and co.sum() == 3
    lf[:] = 0.0
    lf[hj - 2, hi + 5] = 1.0                                     # two rows out: not read
    assert ur.edges_um(lf, ice, hi, hj).sum() == 0
    # the ice branch: land 0.4 with ice 0.25 -> land; with ice 0.2 -> sea
    lf[:] = 0.4
    ice[:] = 0.25
    lf[hj + 3, hi + 3] = 0.0
    ice[hj + 3, hi + 3] = 0.0
    assert ur.edges_um(lf, ice, hi, hj).sum() == 8               # the ring round the sea cell (itself: no gradient)
    ice[:] = 0.2
    assert ur.edges_um(lf, ice, hi, hj).sum() == 0


def test_um_setup_declared_and_exported():
    """The UM-layout setup entry points are in the header and in the library's dynamic symbol table."""
    with open(os.path.join(ROOT, "include", "seabreeze_hip.h")) as f:
        hdr = f.read()
    for name in UM_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
    from seabreeze_param_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    for name in UM_ENTRY_POINTS:
        assert hasattr(lib, name), f"{name} not exported"
