"""numpy restatement of the UM vn10.7 copy's coast setup (UM/vn10.7/sea_breeze_diag.F90: get_edges :328-446,
get_dist :448-601), written from the algorithm, for the tests of sb_get_edges_um_* / sb_get_dist_um_*.

The UM file cannot be compiled outside the UM, so this parity is unpinned by nature (as for seabreeze_diag_um): the
restatement follows the text -- tdims_l layout with halo_i x halo_j ghost cells, 2-D true_latitude/true_longitude,
the +-halo_i x +-halo_j window, interior-only sources and targets (the scatter's halo writes are discarded by
swap_bounds), the two longitude corrections, the sweep-order reset |cdist| > 2*maxdist -> 12000, signs from
landfrac > 0 -- in the working precision (float32 or float64 throughout, the UM's constants rounded to it).
Its one pinned anchor is the regular-grid oracle (tests/test_um_setup_gpu.py::test_dist_um_regular_anchor).

Arrays are C-order numpy (rows, cols): fields with ghost cells are (ny + 2*halo_j, nx + 2*halo_i).

Two forms of get_dist:
  dist_um_literal    the scatter over interior coast cells in sweep order (rows outer, columns inner) with the reset
                     inside the loop, as the UM writes it -- for small grids;
  dist_um_vectorised the minimum over coast sources swept at or before each target, reset, then the minimum with the
                     sources swept after it -- one pass per window offset over the coast cells, for large grids.
"""
from __future__ import annotations

import numpy as np


def constants(dt):
    """R, pi, r2d, d2r of the UM's get_dist in precision dt (UM :509-512)."""
    dt = np.dtype(dt).type
    pi = dt(3.1415926)
    return dt(6370.9989), pi, dt(180.0) / pi, pi / dt(180.0)


def land_um(landfrac_l, icefrac_l):
    """The ice-aware land rule (UM :390-403) on every cell of the field: 0/1 int array."""
    dt = np.dtype(landfrac_l.dtype).type
    lf, ci = landfrac_l, icefrac_l
    return np.where(ci <= dt(0.2), lf >= dt(0.5), (lf + ci) >= dt(0.5)).astype(np.int64)


def edges_um(landfrac_l, icefrac_l, halo_i, halo_j, out=None):
    """get_edges on the tdims_l layout: the rule on the interior and its one-cell ghost ring, the binary 3x3 Sobel
    (weight = reshape((/-1,-2,-1, 0,0,0, 1,2,1/),(3,3))), 0/1 into the interior; the ghost cells of `out` stay."""
    assert halo_i >= 1 and halo_j >= 1
    m = land_um(landfrac_l, icefrac_l)
    NY, NX = m.shape
    ny, nx = NY - 2 * halo_j, NX - 2 * halo_i
    y0, x0 = halo_j, halo_i
    M = lambda dy, dx: m[y0 + dy:y0 + dy + ny, x0 + dx:x0 + dx + nx]
    w = (1, 2, 1)
    px = sum(w[i + 1] * (M(i, 1) - M(i, -1)) for i in (-1, 0, 1))      # d/d(lon), rows weighted 1,2,1
    py = sum(w[j + 1] * (M(1, j) - M(-1, j)) for j in (-1, 0, 1))      # d/d(lat), columns weighted 1,2,1
    coast = np.zeros_like(landfrac_l) if out is None else out.copy()
    coast[y0:y0 + ny, x0:x0 + nx] = np.where((px == 0) & (py == 0), 0, 1).astype(coast.dtype)
    return coast


def _cell_terms(true_lat, true_lon):
    """phi1, the source longitude l1 (UM :552-556) and the target longitude l2 (UM :560-564) of every cell."""
    dt = np.dtype(true_lat.dtype).type
    _, _, r2d, d2r = constants(dt)
    phi = true_lat * d2r
    lam1 = true_lon * d2r
    l1 = np.where(true_lon > dt(180), d2r * (true_lon - dt(360.)), d2r * true_lon)
    x = r2d * lam1
    l2 = np.where(x > dt(180.), d2r * (x - dt(360.)), lam1)
    return phi, l1.astype(true_lat.dtype), l2.astype(true_lat.dtype)


def _pair_c(phis, l1s, phit, l2t):
    """c of source -> target, as UM :565-567 writes it (vectorised over pairs)."""
    dt = np.dtype(phis.dtype).type
    R = constants(dt)[0]
    dphi = phis - phit
    dlam = l1s - l2t
    a = np.sin(dphi / dt(2)) ** 2 + (np.cos(phis) * (np.cos(phit) * np.sin(dlam / dt(2)) ** 2))
    return R * dt(2) * np.arctan2(np.sqrt(a), np.sqrt(dt(1) - a)) + dt(0.5)


def _interior(coast_l, halo_i, halo_j, ny, nx):
    return coast_l[halo_j:halo_j + ny, halo_i:halo_i + nx]


def dist_um_literal(coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, maxdist=180.0, out=None):
    """The UM's scatter: for every interior cell in sweep order, a coast cell lowers |cdist| of the interior cells in its
    window; then the cell's own |cdist| > 2*maxdist resets it to 12000.  Returns the tdims_l field (ghost cells from
    `out`, zeros without it)."""
    dt = np.dtype(landfrac.dtype).type
    ny, nx = landfrac.shape
    co = _interior(coast_l, halo_i, halo_j, ny, nx)
    phi, l1, l2 = _cell_terms(true_lat, true_lon)
    cd = np.full((ny, nx), dt(12000.), dtype=landfrac.dtype)
    big2 = dt(2) * dt(maxdist)
    for j in range(ny):
        for i in range(nx):
            if co[j, i] > 0:
                j0, j1, i0, i1 = max(j - halo_j, 0), min(j + halo_j, ny - 1) + 1, max(i - halo_i, 0), min(i + halo_i, nx - 1) + 1
                c = _pair_c(phi[j, i], l1[j, i], phi[j0:j1, i0:i1], l2[j0:j1, i0:i1])
                win = cd[j0:j1, i0:i1]
                upd = c < np.abs(win)
                win[upd] = np.where(landfrac[j0:j1, i0:i1] > 0, c, -c)[upd]
            if abs(cd[j, i]) > big2:
                cd[j, i] = dt(12000.)
    res = np.zeros_like(coast_l) if out is None else out.copy()
    _interior(res, halo_i, halo_j, ny, nx)[...] = cd
    return res


def dist_um_vectorised(coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, maxdist=180.0, out=None):
    """The same field from the minimum over coast sources swept at or before each target (reset by the 2*maxdist rule)
    and the minimum over those swept after it: one pass per window offset over the interior coast cells."""
    dt = np.dtype(landfrac.dtype).type
    ny, nx = landfrac.shape
    co = _interior(coast_l, halo_i, halo_j, ny, nx)
    phi, l1, l2 = _cell_terms(true_lat, true_lon)
    sj, si = np.nonzero(co > 0)
    ps, ls = phi[sj, si], l1[sj, si]
    big = dt(12000.)
    early = np.full(ny * nx, big, dtype=landfrac.dtype)
    late = np.full(ny * nx, big, dtype=landfrac.dtype)
    phf, l2f = phi.ravel(), l2.ravel()
    for jj in range(-halo_j, halo_j + 1):
        tj = sj + jj
        okj = (tj >= 0) & (tj < ny)
        for ii in range(-halo_i, halo_i + 1):
            ti = si + ii
            ok = okj & (ti >= 0) & (ti < nx)
            t = tj[ok] * nx + ti[ok]                  # distinct targets for one offset: plain fancy indexing is safe
            c = _pair_c(ps[ok], ls[ok], phf[t], l2f[t])
            acc = early if (jj > 0 or (jj == 0 and ii >= 0)) else late     # source swept at or before the target
            acc[t] = np.minimum(acc[t], c)
    early[early > dt(2) * dt(maxdist)] = big
    m = np.minimum(early, late).reshape(ny, nx)
    cd = np.where(m >= big, big, np.where(landfrac > 0, m, -m)).astype(landfrac.dtype)
    res = np.zeros_like(coast_l) if out is None else out.copy()
    _interior(res, halo_i, halo_j, ny, nx)[...] = cd
    return res


def dist_plain_min(coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, maxdist=180.0):
    """The same without the sweep-order reset (a plain minimum over the window, capped at 12000): the tests show that
    the reset changes the field."""
    return dist_um_vectorised(coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, maxdist=1.0e30)


def rotated_grid(nx, ny, dlon=0.11, dlat=0.11, centre_lon=180.0, centre_lat=-35.0, twist=25.0, convention="0-360",
                 dtype=np.float64):
    """true_lat, true_lon (degrees, (ny, nx)) of a rotated-pole limited-area grid: a regular grid of spacing dlon x dlat
    around the rotated equator's origin, turned by `twist` degrees about its centre and carried to (centre_lon,
    centre_lat).  convention "0-360": longitudes in [0, 360) (a domain round 180 crosses it, so both branches of the
    UM's longitude corrections are taken); "-180-180": longitudes in (-180, 180].  Deterministic: float64 throughout,
    rounded to dtype at the end."""
    rlon = np.deg2rad((np.arange(nx) - (nx - 1) / 2.0) * dlon)
    rlat = np.deg2rad((np.arange(ny) - (ny - 1) / 2.0) * dlat)
    RL, RP = np.meshgrid(rlon, rlat)
    p = np.stack([np.cos(RP) * np.cos(RL), np.cos(RP) * np.sin(RL), np.sin(RP)])
    g, b, a = np.deg2rad(twist), -np.deg2rad(centre_lat), np.deg2rad(centre_lon)
    rx = np.array([[1, 0, 0], [0, np.cos(g), -np.sin(g)], [0, np.sin(g), np.cos(g)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    q = np.einsum("ij,jkl->ikl", rz @ ry @ rx, p)
    lat = np.rad2deg(np.arcsin(np.clip(q[2], -1.0, 1.0)))
    lon = np.rad2deg(np.arctan2(q[1], q[0]))
    if convention == "0-360":
        lon = np.mod(lon, 360.0)
    elif convention == "-180-180":
        lon = np.where(lon <= -180.0, lon + 360.0, lon)
    else:
        raise ValueError(convention)
    return np.ascontiguousarray(lat, dtype), np.ascontiguousarray(lon, dtype)


GRIDS = {
    # across the date line in the 0-360 convention: both longitude branches, and the jump of 2*pi between them
    "dateline": dict(centre_lon=180.0, centre_lat=-35.0, twist=25.0, convention="0-360"),
    # negative longitudes
    "west": dict(centre_lon=-60.0, centre_lat=20.0, twist=-40.0, convention="-180-180"),
    # round the geographic pole: longitudes of neighbours far apart, latitudes not monotone along a row
    "polar": dict(centre_lon=30.0, centre_lat=88.0, twist=10.0, convention="0-360"),
}


def grid_named(name, nx, ny, dtype=np.float64, dlon=0.11, dlat=0.11):
    return rotated_grid(nx, ny, dlon=dlon, dlat=dlat, dtype=dtype, **GRIDS[name])


def pad_edge(a, halo_i, halo_j):
    """Ghost cells by edge replication (what a caller's swap_bounds might leave at a domain edge)."""
    return np.ascontiguousarray(np.pad(a, ((halo_j, halo_j), (halo_i, halo_i)), mode="edge"))


def noise_mask(nx, ny, seed, dt, frac=False):
    """Land fraction with coast cells everywhere (blobs of a few cells) and patches of sea ice, as the regular-grid setup
    tests build them (tests/test_setup_gpu.py)."""
    from seabreeze_param_amd import synth
    r = synth.hash_uniform((ny, nx), 3, seed)
    s = r + np.roll(r, 1, 1) + np.roll(r, 1, 0) + np.roll(r, -1, 1)
    land = (s > 2.2).astype(np.float64)
    if frac:
        land = np.round(np.clip((s - 1.6) / 1.2, 0, 1) * 8) / 8
    ice = np.where(synth.hash_uniform((ny, nx), 4, seed) > 0.9, 0.35, 0.0)
    return np.ascontiguousarray(land, dt), np.ascontiguousarray(ice, dt)


def sparse_mask(nx, ny, seed, dt):
    """A few isolated islands, some on the first and last columns: most windows empty, some with one far hit."""
    from seabreeze_param_amd import synth
    r = synth.hash_uniform((ny, nx), 5, seed)
    land = (r > 0.995).astype(np.float64)
    land[:, 0] = (r[:, 0] > 0.9)
    land[:, -1] = (r[:, -1] > 0.93)
    return np.ascontiguousarray(land, dt), np.zeros((ny, nx), dt)


def coast_of(land, ice, halo_i, halo_j):
    """Interior land / ice -> (padded landfrac_l, padded icefrac_l, coast_l by edges_um) with edge-replicated ghosts."""
    lf_l, ci_l = pad_edge(land, max(halo_i, 1), max(halo_j, 1)), pad_edge(ice, max(halo_i, 1), max(halo_j, 1))
    co = edges_um(lf_l, ci_l, max(halo_i, 1), max(halo_j, 1))
    hi1, hj1 = max(halo_i, 1), max(halo_j, 1)
    inner = co[hj1:co.shape[0] - hj1, hi1:co.shape[1] - hi1]
    return lf_l, ci_l, np.ascontiguousarray(np.pad(inner, ((halo_j, halo_j), (halo_i, halo_i))))
