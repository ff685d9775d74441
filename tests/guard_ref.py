"""Numpy model of the guard for missing and non-finite temperatures (sb_set_nonfinite_guard, sb_guard_kernels.hip,
include/seabreeze_hip.h), for tests/test_guard_model.py and tests/test_nonfinite_guard_gpu.py.

Three things, each under the three boundary rules (tests/radius_ref.py restates sb_map_cell):

  bad_plane        the cells k_guard_bits marks: !(|theta| + 0.0060956 |z| < 2048) in the working precision, over the frame;
  affected         the EXACT set: band cells whose final window -- radius from radius_ref.search_radius; the cap where the search
                   finds one class only -- holds a bad cell;
  specified_taint  what k_guard_taint is specified to produce: band cells whose window of the contrast kernel's reach R holds a
                   bad cell, or, by tile, band cells of tiles whose staged rectangle (tile plus LDS halo) holds one.

All three are written as incidence products, not as the kernels' two dilation passes: hit_x[x, X] says that frame column X
is among the columns a span round interior column x reads, hit_y likewise for rows, and a cell is hit iff
hit_y . bad . hit_x^T is positive there.
"""
from __future__ import annotations

import numpy as np

import radius_ref as rr

GMMA_ABS = 0.0060956
LIMIT = 2048.0
REACH = {"strip": 16, "strip32": 31, "table": 127}


def bad_plane(theta, z):
    dt = theta.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        return ~(np.abs(theta) + dt(GMMA_ABS) * np.abs(z.astype(theta.dtype)) < dt(LIMIT))


def _hits(n, nh, lo, hi, mapper):
    """hit[c, C]: frame index C is read by the span lo[c] .. hi[c] (interior coordinates, any integers) round interior index c"""
    hit = np.zeros((n, nh), dtype=bool)
    for c in range(n):
        C = mapper(np.arange(lo[c], hi[c] + 1))
        hit[c, C[C >= 0]] = True
    return hit


def _product(bad, hy, hx):
    return (hy.astype(np.int64) @ bad.astype(np.int64) @ hx.astype(np.int64).T) > 0


def window_holds_bad(bad, ny, nx, halo, bnd, r):
    """(ny, nx): the square of radius r (a scalar) round every interior cell holds a bad cell of the frame"""
    xs, ys = np.arange(nx), np.arange(ny)
    hx = _hits(nx, nx + 2 * halo, xs - r, xs + r, lambda a: rr.map_x(a, nx, halo, bnd, None))
    hy = _hits(ny, ny + 2 * halo, ys - r, ys + r, lambda a: rr.map_y(a, ny, halo, bnd, None))
    return _product(bad, hy, hx)


def final_radius(mask_f, maxdist, halo, bnd):
    """-> (radius plane of radius_ref, the radius of every band cell's final window: the cap where the search ends without both
    classes, 0 off the band)"""
    radius = rr.search_radius(mask_f, maxdist, halo, bnd)
    nyh, nxh = mask_f.shape
    cap = rr.cap_plane(nyh - 2 * halo, nxh - 2 * halo, halo, bnd, None)
    return radius, np.where(radius == -1, cap, radius).astype(np.int64)


def affected(bad, mask_f, maxdist, halo, bnd):
    """-> (exact set (ny, nx) bool, radius plane, is_band)"""
    nyh, nxh = mask_f.shape
    ny, nx = nyh - 2 * halo, nxh - 2 * halo
    radius, fin = final_radius(mask_f, maxdist, halo, bnd)
    isband = radius != 0
    out = np.zeros((ny, nx), dtype=bool)
    if bad.any():
        for r in np.unique(fin[isband]):
            sel = isband & (fin == r)
            out |= sel & window_holds_bad(bad, ny, nx, halo, bnd, int(r))
    return out, radius, isband


def specified_taint(bad, isband, halo, bnd, reach=None, tile=None):
    """reach: R in cells; tile = (width, rows, LDS halo): by tile.  -> (ny, nx) bool"""
    ny, nx = isband.shape
    xs, ys = np.arange(nx), np.arange(ny)
    if tile is None:
        xlo, xhi, ylo, yhi = xs - reach, xs + reach, ys - reach, ys + reach
    else:
        w, rows, hk = tile
        xlo, ylo = xs - xs % w - hk, ys - ys % rows - hk
        xhi, yhi = xlo + w - 1 + 2 * hk, ylo + rows - 1 + 2 * hk
    hx = _hits(nx, nx + 2 * halo, xlo, xhi, lambda a: rr.map_x(a, nx, halo, bnd, None))
    hy = _hits(ny, ny + 2 * halo, ylo, yhi, lambda a: rr.map_y(a, ny, halo, bnd, None))
    return isband & _product(bad, hy, hx)


def within_reach(radius, reach=None, tile=None):
    """band cells the contrast kernel answers from its fast path: those the guard has to cover (the others take the
    global-memory search, which is right with a finite centre)"""
    r = reach if tile is None else tile[2]
    return (radius >= 1) & (radius <= r)


# ---- the directed fields ---------------------------------------------------------------------------------------------------

GRID = (160, 96)            # k_strip: 5 strips, 6 blocks
TABLE_GRID = (176, 128)     # 40-cell blocks of land
NAN, INF, MISSING = float("nan"), float("inf"), 2.0e20


def coast_cells(land, isband):
    """(land band cells with a sea neighbour to the east, sea band cells with a land neighbour to the west), row-major lists of (y, x)"""
    ny, nx = land.shape
    east_sea = ~np.roll(land, -1, axis=1)
    west_land = np.roll(land, 1, axis=1)
    inner = np.zeros_like(land)
    inner[2:ny - 2, 2:nx - 2] = True
    a = np.argwhere(land & east_sea & isband & inner)
    b = np.argwhere(~land & west_land & isband & inner)
    return [tuple(int(v) for v in c) for c in a], [tuple(int(v) for v in c) for c in b]


def directed(land, isband, radius):
    """{case: [(field, y, x, value), ...]} in interior coordinates for the global grid: the cases (a) - (e), (h), (i), (k) of
    tests/test_nonfinite_guard_gpu.py"""
    ny, nx = land.shape
    lc, sc = coast_cells(land, isband)
    mid = len(lc) // 2
    (ly, lx), (sy, sx) = lc[mid], sc[len(sc) // 2]
    # (c) not a band cell, inside band cells' windows: the nearest such cell to the middle coast cell
    cand = np.argwhere(~isband)
    near = [tuple(int(v) for v in c) for c in cand
            if 2 <= c[0] < ny - 2 and isband[max(c[0] - 1, 0):c[0] + 2, max(c[1] - 1, 0):c[1] + 2].any()]
    cy, cx = min(near, key=lambda c: (c[0] - ly) ** 2 + (c[1] - lx) ** 2)
    # (e) the two pole rows -- below the band cells nearest to each pole; whether their windows reach the row is the grid's
    # business (on the block grid of tests/test_nonfinite_guard_gpu.py they do) -- and the last column in a row with band cells at the seam
    rows = np.flatnonzero(isband.any(axis=1))
    south, north = int(np.flatnonzero(isband[rows[0]])[0]), int(np.flatnonzero(isband[rows[-1]])[0])
    seam_y = int(np.flatnonzero(isband[:, nx - 1] | isband[:, 0] | isband[:, nx - 2])[0])
    # (i) +Inf on land and +Inf at sea inside one window: the coast cell and its eastern neighbour
    cases = {
        "a_nan_land_coast": [("theta", ly, lx, NAN)],
        "b_inf_sea_centre": [("theta", sy, sx, INF)],
        "c_missing_off_band": [("theta", cy, cx, MISSING)],
        "d_nan_strip_block_corner": [("theta", y, x, NAN) for y in (15, 16) for x in (31, 32)],
        "e_nan_pole_row_and_seam": [("theta", 0, south, NAN), ("theta", ny - 1, north, NAN), ("theta", seam_y, nx - 1, NAN)],
        "h_nan_in_z_land": [("z", ly, lx, NAN)],
        "i_inf_land_and_sea": [("theta", ly, lx, INF), ("theta", ly, lx + 1, INF)],
        "k_missing_block": [("theta", y, x, MISSING) for y in range(max(ly - 20, 0), min(ly + 20, ny))
                            for x in range(lx - 20, lx + 20)],
    }
    return cases


def poison(theta, z, spec, halo=0):
    """copies of (theta, z) with the case's cells set (columns wrap: the block of (k) may cross the seam)"""
    theta, z = theta.copy(), z.copy()
    nx = theta.shape[1] - 2 * halo
    for name, y, x, v in spec:
        (theta if name == "theta" else z)[y + halo, x % nx + halo] = v
    return theta, z


def must_cover(exact, radius, bad, isband, halo, bnd, reach=None, tile=None):
    """The band cells a taint has to hold: those of the exact set the contrast kernel answers itself (radius within its
    reach), and every band cell that is bad itself.  Band cells beyond the reach take the global-memory search, which sums
    about a FINITE centre there and is right as it stands."""
    ny, nx = isband.shape
    X, Y = rr.map_x(np.arange(nx), nx, halo, bnd, None), rr.map_y(np.arange(ny), ny, halo, bnd, None)
    centre = isband & bad[Y[:, None], X[None, :]]       # (the wrapper's rule reads column 1 for the centre of a last-column cell)
    return (exact & within_reach(radius, reach, tile)) | centre


def global_field(orc, dt):
    """GRID with the synthetic coast and the oracle's distance field: (st, cdist), every radius 1"""
    from seabreeze_param_amd import synth
    nx, ny = GRID
    st = synth.static_fields(nx, ny, dt)
    coast = orc.get_edges(st.landfrac, st.icefrac)
    return st, orc.get_dist(coast, st.landfrac, st.lon, st.lat)


def table_land():
    """TABLE_GRID: two 40-cell blocks of land, one up to the seam on the south pole's rows, one in mid-ocean: radii up to 60"""
    import table_ref as tr
    nx, ny = TABLE_GRID
    return tr.block_land(nx, ny, 40, nx) | tr.block_land(nx, ny, 40, nx, dx=-88, dy=70)


def um_field(orc, dt, hs=2, hl=6):
    """The UM layout (tests/test_sigma_stats_gpu.py): GRID cut from a bigger field whose rim serves as ghost cells; the band is
    the cells within one cell of the coast.  -> (st of the big field, cd_l (mask, ghost width hl), inner(a, h))"""
    from seabreeze_param_amd import synth
    nx, ny = GRID
    st = synth.static_fields(nx + 2 * hl, ny + 2 * hl, dt)
    coast = orc.get_edges(st.landfrac, st.icefrac)
    cd_l = orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=9000.0, kwin=1)
    cd_l = np.where(np.abs(cd_l) < 12000.0, np.sign(cd_l) * np.minimum(np.abs(cd_l), 179.0), cd_l).astype(dt)
    inner = lambda a, h: np.ascontiguousarray(a[..., hl - h:a.shape[-2] - (hl - h), hl - h:a.shape[-1] - (hl - h)])
    return st, cd_l, inner


def um_ghost_cell(isband, radius, hs):
    """(Y, X) of a ghost cell of the (hs-wide) frame inside the final window of a band cell on the interior's edge"""
    ny, nx = isband.shape
    for x in range(hs, nx - hs):
        if isband[0, x] and 1 <= radius[0, x] <= hs:
            return hs - 1, x + hs
    for y in range(hs, ny - hs):
        if isband[y, 0] and 1 <= radius[y, 0] <= hs:
            return y + hs, hs - 1
    raise AssertionError("no band cell on the edge of the interior")
