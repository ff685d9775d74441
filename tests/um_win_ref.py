"""Reference and inputs for sb_get_dist_um_win_* (tests/test_um_dist_win_host.py, tests/test_um_dist_win_gpu.py).

The restatement of the UM's get_dist (tests/um_setup_ref.py) takes window = ghost width.  A window stated apart from the
layout is the same rule on another padding: sources and targets are interior cells only, so the interior coast is
re-padded with zeros to the window's width, the restatement is called with halo = window, and the interior is cut out.
"""
from __future__ import annotations

import functools

import numpy as np

import um_setup_ref as ur

SENTINEL = -7.25

# single land cells (row, col) of the seven-island mask on 300 x 250: near two corners, on both side edges, a diagonal pair
ISLANDS = ((5, 3), (120, 150), (121, 151), (240, 296), (60, 299), (200, 0), (125, 20))
ISLANDS_SHAPE = (300, 250)          # nx, ny
KM_SCALE = 0.0135                   # degrees: 113 cells for 180 km

# the chain into the table contrast: a rotated 0.0135-degree grid, land south of the middle row
CHAIN = dict(nx=320, ny=400, halo=116, win=113, maxdist=180.0, grid="dateline")


def dist_win(fn, coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, win_i, win_j, maxdist=180.0, out=None):
    """`fn` (dist_um_literal or dist_um_vectorised) for the window +-win_i x +-win_j on a field whose layout has
    halo_i x halo_j ghost cells.  Returns the field on coast_l's layout: ghost cells from `out`, zeros without it."""
    ny, nx = landfrac.shape
    inner = coast_l[halo_j:halo_j + ny, halo_i:halo_i + nx]
    padded = np.ascontiguousarray(np.pad(inner, ((win_j, win_j), (win_i, win_i))))
    f = fn(padded, landfrac, true_lat, true_lon, win_i, win_j, maxdist=maxdist)
    res = np.zeros_like(coast_l) if out is None else out.copy()
    res[halo_j:halo_j + ny, halo_i:halo_i + nx] = f[win_j:win_j + ny, win_i:win_i + nx]
    return res


def dist_win_literal(coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, win_i, win_j, maxdist=180.0, out=None):
    return dist_win(ur.dist_um_literal, coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, win_i, win_j, maxdist, out)


def check_dist(h, o, what, rel):
    """The project's rule (tests/test_um_setup_gpu.py::_check_dist): 12000-cells and signs identical, distances to `rel`
    relative with denominator max(|o|, 1)."""
    assert np.array_equal(h >= 12000.0, o >= 12000.0), f"{what}: cells without a coast in reach differ"
    assert np.array_equal(np.sign(h), np.sign(o)), f"{what}: signs differ"
    e = np.abs(h.astype(np.float64) - o) / np.maximum(np.abs(o.astype(np.float64)), 1.0)
    assert e.max() <= rel, f"{what}: max rel err {e.max()}"


def sentinel_field(shape, dt, hi, hj):
    """A field whose ghost cells hold SENTINEL (and whose interior holds another value) -- what must survive."""
    f = np.full(shape, SENTINEL, dt)
    f[hj:shape[0] - hj, hi:shape[1] - hi] = 3.5
    return f


def seven_islands(dt):
    """land, ice of the seven-island mask (ISLANDS_SHAPE)."""
    nx, ny = ISLANDS_SHAPE
    land = np.zeros((ny, nx), dt)
    for r, c in ISLANDS:
        land[r, c] = 1.0
    return land, np.zeros((ny, nx), dt)


def islands_case(grid, dt, halo_i=0, halo_j=0):
    """lat, lon, land, coast_l of the seven-island mask on grid `grid` at 0.0135 degrees."""
    nx, ny = ISLANDS_SHAPE
    lat, lon = ur.grid_named(grid, nx, ny, dt, dlon=KM_SCALE, dlat=KM_SCALE)
    land, ice = seven_islands(dt)
    _, _, coast_l = ur.coast_of(land, ice, halo_i, halo_j)
    return lat, lon, land, coast_l


def field_classes(coast_l, land, lat, lon, win_i, win_j, maxdist):
    """(reference field, reset cells, reached cells beyond 2*maxdist, unreached cells) of a layout without ghost cells:
    reset = reached by the plain minimum over the window but 12000 in the field (the sweep-order reset threw the early
    sources away and no later one came); beyond = reached through a later source at more than 2*maxdist."""
    o = dist_win_literal(coast_l, land, lat, lon, 0, 0, win_i, win_j, maxdist)
    plain = dist_win(ur.dist_um_vectorised, coast_l, land, lat, lon, 0, 0, win_i, win_j, 1.0e30)
    reached = np.abs(plain) < 12000.0
    reset = reached & (o >= 12000.0)
    beyond = (np.abs(o) < 12000.0) & (np.abs(o) > 2.0 * maxdist)
    return o, reset, beyond, ~reached


@functools.lru_cache(maxsize=None)
def chain_case():
    """The chain test's inputs and reference on the tdims_l layout with CHAIN['halo'] ghost cells each way (enough that
    neither the distance window of 113 cells nor a contrast window of the band's largest radius is cut):
    dict(lat, lon, lf_l, ci_l, lf, coast_l, ref), ref the literal field with edge-replicated ghost cells."""
    c = CHAIN
    nx, ny, h, w, dt = c["nx"], c["ny"], c["halo"], c["win"], np.float64
    lat, lon = ur.grid_named(c["grid"], nx, ny, dt, dlon=KM_SCALE, dlat=KM_SCALE)
    lf = np.ascontiguousarray(np.broadcast_to(np.arange(ny)[:, None] < ny // 2, (ny, nx)), dt)
    lf_l, ci_l = ur.pad_edge(lf, h, h), np.zeros((ny + 2 * h, nx + 2 * h), dt)
    coast_l = ur.edges_um(lf_l, ci_l, h, h)
    ref = dist_win_literal(coast_l, lf, lat, lon, h, h, w, w, c["maxdist"])
    ref = ur.pad_edge(ref[h:h + ny, h:h + nx], h, h)
    return dict(lat=lat, lon=lon, lf_l=lf_l, ci_l=ci_l, lf=lf, coast_l=coast_l, ref=ref)
