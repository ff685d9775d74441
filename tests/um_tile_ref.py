"""Reference, cuts and cases for sb_tile_get_edges_um_* / sb_tile_get_dist_um_* (tests/test_um_tile_host.py,
tests/test_um_tile_gpu.py): the UM-layout coast setup on one tile of a 2-D domain decomposition.

The rule: a tile's sources are the coast cells of its interior and of the in-domain ghost cells within the window; its
targets are its interior.  Whether a source is swept at or before a target is a test on row and column differences, so the
numpy model is the whole-domain restatement (tests/um_win_ref.py) run on the EXTENDED rectangle -- the tile plus the
window, clipped at the domain's edge -- as if that were a domain, and the tile's cells cut out of the result.

Arrays are C-order numpy (rows, cols); a tile is (x0, x1, y0, y1), columns [x0, x1) and rows [y0, y1) of the domain.
"""
from __future__ import annotations

import functools

import numpy as np

import um_setup_ref as ur
import um_win_ref as uw

WEST, EAST, SOUTH, NORTH = 1, 2, 4, 8           # include/seabreeze_hip.h: SB_TILE_*

# 1: sparse coasts under a wide window ("west" grid): most tiles find their sources beyond a seam
SPARSE = dict(grid="west", nx=200, ny=30, seed=7, win=(40, 9), halo=(41, 10), maxdist=180.0)
SPARSE_CUTS = {
    "equal": ((0, 67, 134, 200), (0, 10, 20, 30)),
    # a tile narrower than a 64-column workgroup and than the window, row counts that are no multiples of 4, a middle tile
    # without an edge side
    "unequal": ((0, 70, 83, 200), (0, 9, 15, 30)),
    # every tile of the two cuts above holds coast cells of its own; the middle tile of this one holds none: all its
    # sources are ghost cells (tests/test_um_tile_host.py::test_sparse_case_holds_every_class)
    "ghost": ((0, 80, 100, 200), (0, 9, 15, 30)),
}
GHOST_ONLY_TILE = (80, 100, 9, 15)
# 2: dense coasts with ice on the three grids, edges and distance in a chain
DENSE = dict(nx=150, ny=22, seed=11, win=(6, 5), halos=((7, 6), (9, 9)), maxdist=180.0, cuts=((0, 50, 100, 150), (0, 7, 14, 22)))
# 3: km scale: um_win_ref.islands_case, four passes of the row staging
ISLANDS = dict(grid="dateline", win=(113, 113), halo=(114, 114), maxdist=180.0, cuts=((0, 150, 300), (0, 125, 250)))


def tiles(cuts):
    """every tile (x0, x1, y0, y1) of a cut (column bounds, row bounds), rows outer"""
    xs, ys = cuts
    return [(xs[i], xs[i + 1], ys[j], ys[j + 1]) for j in range(len(ys) - 1) for i in range(len(xs) - 1)]


def sides_of(tile, nx, ny):
    """the SB_TILE_* bits of a tile of an nx x ny domain: a set bit = that side is the domain's edge"""
    x0, x1, y0, y1 = tile
    return (WEST if x0 == 0 else 0) | (EAST if x1 == nx else 0) | (SOUTH if y0 == 0 else 0) | (NORTH if y1 == ny else 0)


def cut(field, x0, x1, y0, y1, halo_i, halo_j, fill):
    """The tile's frame (y1-y0 + 2*halo_j, x1-x0 + 2*halo_i) cut out of a whole-domain (ny, nx) field: ghost cells inside
    the domain are the neighbours' cells (what swap_bounds brings), ghost cells outside it hold `fill`."""
    ny, nx = field.shape
    f = np.full((y1 - y0 + 2 * halo_j, x1 - x0 + 2 * halo_i), fill, field.dtype)
    gx0, gx1, gy0, gy1 = max(x0 - halo_i, 0), min(x1 + halo_i, nx), max(y0 - halo_j, 0), min(y1 + halo_j, ny)
    f[gy0 - (y0 - halo_j):gy1 - (y0 - halo_j), gx0 - (x0 - halo_i):gx1 - (x0 - halo_i)] = field[gy0:gy1, gx0:gx1]
    return f


def in_domain(tile, nx, ny, halo_i, halo_j, reach_i, reach_j):
    """bool frame: the interior and the in-domain ghost cells within reach_i columns / reach_j rows of it"""
    x0, x1, y0, y1 = tile
    inside = cut(np.ones((ny, nx), bool), x0, x1, y0, y1, halo_i, halo_j, False)
    near = np.zeros_like(inside)
    near[halo_j - reach_j:halo_j + (y1 - y0) + reach_j, halo_i - reach_i:halo_i + (x1 - x0) + reach_i] = True
    return inside & near


def extended(tile, nx, ny, win_i, win_j):
    x0, x1, y0, y1 = tile
    return max(x0 - win_i, 0), min(x1 + win_i, nx), max(y0 - win_j, 0), min(y1 + win_j, ny)


def tile_dist(coast, land, lat, lon, tile, win_i, win_j, maxdist, reach=None):
    """The model: interior (ny, nx) fields of the whole domain -> the tile's cells of the distance field, from the extended
    rectangle alone.  reach=(0, 0) is the interior-only rule of sb_get_dist_um_win_* applied to the tile."""
    ny, nx = land.shape
    x0, x1, y0, y1 = tile
    ex0, ex1, ey0, ey1 = extended(tile, nx, ny, *((win_i, win_j) if reach is None else reach))
    sub = lambda a: np.ascontiguousarray(a[ey0:ey1, ex0:ex1])
    f = uw.dist_win(ur.dist_um_vectorised, sub(coast), sub(land), sub(lat), sub(lon), 0, 0, win_i, win_j, maxdist)
    return f[y0 - ey0:y1 - ey0, x0 - ex0:x1 - ex0]


def whole_dist(coast, land, lat, lon, win_i, win_j, maxdist):
    """the whole-domain reference on interior fields"""
    return uw.dist_win(ur.dist_um_vectorised, coast, land, lat, lon, 0, 0, win_i, win_j, maxdist)


def tile_edges(coast, tile, halo_i, halo_j, ext_i, ext_j, fill):
    """The model for edges: the whole-domain coast cut to the frame, `fill` in every cell the call leaves alone (beyond
    ext, and outside the domain)."""
    ny, nx = coast.shape
    f = cut(coast, *tile, halo_i, halo_j, fill)
    f[~in_domain(tile, nx, ny, halo_i, halo_j, ext_i, ext_j)] = fill
    return f


def _coast(land, ice):
    """interior coast (ny, nx) by edges_um on edge-replicated ghosts"""
    _, _, c = ur.coast_of(land, ice, 0, 0)
    return c


@functools.lru_cache(maxsize=None)
def sparse_case(prec):
    """dict(lat, lon, land, ice, coast) of SPARSE, interior (ny, nx) fields"""
    c, dt = SPARSE, (np.float64 if prec == 8 else np.float32)
    lat, lon = ur.grid_named(c["grid"], c["nx"], c["ny"], dt)
    land, ice = ur.sparse_mask(c["nx"], c["ny"], c["seed"], dt)
    return dict(lat=lat, lon=lon, land=land, ice=ice, coast=_coast(land, ice))


@functools.lru_cache(maxsize=None)
def dense_case(grid, prec):
    c, dt = DENSE, (np.float64 if prec == 8 else np.float32)
    lat, lon = ur.grid_named(grid, c["nx"], c["ny"], dt)
    land, ice = ur.noise_mask(c["nx"], c["ny"], c["seed"], dt)
    return dict(lat=lat, lon=lon, land=land, ice=ice, coast=_coast(land, ice))


@functools.lru_cache(maxsize=None)
def islands_case():
    lat, lon, land, coast = uw.islands_case(ISLANDS["grid"], np.float64)
    return dict(lat=lat, lon=lon, land=land, ice=np.zeros_like(land), coast=coast)
