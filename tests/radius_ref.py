"""Numpy model of search_radius (include/seabreeze_hip.h): the radius at which a band cell's expanding window first holds a
land-side and a sea-side cell, under the three boundary rules and in a latitude band's frame.

It restates sb_map_cell (csrc/sb_device.hpp) as two index vectors -- a window offset's frame column / frame row, -1 where
the cell does not exist -- and grows every cell's window ring by ring: the ring of radius nn is rows y-nn, y+nn over
|dx| <= nn and columns x-nn, x+nn over |dy| <= nn, each the OR of a plane that is itself grown by two gathers per ring.
So a ring costs O(cells), whatever the radius.  Nothing here measures distances along rows, as the kernels do."""
import numpy as np

BND_WRAPPER, BND_GLOBAL, BND_HALO = 0, 1, 2


def map_x(xs, nx, halo, bnd, band):
    """Frame column of interior column xs (any integer array); -1: no such cell."""
    xs = np.asarray(xs)
    if bnd == BND_HALO:
        if band is not None:
            return np.mod(xs, nx) + halo
        X = xs + halo
        return np.where((X >= 0) & (X < nx + 2 * halo), X, -1)
    if bnd == BND_WRAPPER:
        m = np.mod(xs + 1, nx)                     # kj = max(1, modulo(jj, nlons)), jj = xs + 1
        return np.maximum(m, 1) - 1
    return np.mod(xs, nx)


def map_y(ys, ny, halo, bnd, band):
    """Frame row of interior row ys; -1: no such cell.  band = (south, north) or None."""
    ys = np.asarray(ys)
    if bnd == BND_HALO:
        if band is not None:
            south, north = band
            if south:
                ys = np.maximum(ys, 0)
            if north:
                ys = np.minimum(ys, ny - 1)
        Y = ys + halo
        return np.where((Y >= 0) & (Y < ny + 2 * halo), Y, -1)
    return np.clip(ys, 0, ny - 1)


def classify(mask_f, maxdist, ny, nx, halo, bnd):
    """(band (ny, nx), land (frame)) as k_scan classifies, in mask_f's precision."""
    dt = mask_f.dtype.type
    with np.errstate(invalid="ignore"):
        land = mask_f >= dt(0)
        inner = mask_f[halo:halo + ny, halo:halo + nx]
        band = ~(np.abs(inner) > dt(maxdist))
    if bnd == BND_WRAPPER:
        band = band.copy()
        band[ny - 1, :] = False
    return band, land


def cap_plane(ny, nx, halo, bnd, band):
    cap = np.full((ny, nx), nx + ny, dtype=np.int64)
    if bnd != BND_HALO:
        return cap
    big = 1 << 20
    x = np.arange(nx)[None, :]
    y = np.arange(ny)[:, None]
    if band is None:
        rx = np.minimum(x + halo, nx - 1 - x + halo)
        rs, rn = y + halo, ny - 1 - y + halo
    else:
        south, north = band
        rx = np.full((1, nx), big)
        rs = np.full((ny, 1), big) if south else y + halo
        rn = np.full((ny, 1), big) if north else ny - 1 - y + halo
    return np.minimum(cap, np.minimum(rx, np.minimum(rs, rn)))


def search_radius(mask_f, maxdist=180.0, halo=0, bnd=BND_GLOBAL, band=None):
    """mask_f: (ny + 2*halo, nx + 2*halo).  band = (south, north): the band step's frame (bnd is SB_BND_HALO then).
    Returns radius (ny, nx) int32: 0 off the band, nn >= 1, or -1."""
    if band is not None:
        bnd = BND_HALO
    nyh, nxh = mask_f.shape
    ny, nx = nyh - 2 * halo, nxh - 2 * halo
    isband, land = classify(mask_f, maxdist, ny, nx, halo, bnd)
    cap = cap_plane(ny, nx, halo, bnd, band)
    radius = np.where(isband, -1, 0).astype(np.int32)
    xs, ys = np.arange(nx), np.arange(ny)
    mx = lambda o: map_x(xs + o, nx, halo, bnd, band)
    my = lambda o: map_y(ys + o, ny, halo, bnd, band)
    state = []
    for cls in (land, ~land):
        ext = np.zeros((nyh + 1, nxh + 1), dtype=bool)       # row -1 and column -1: the cell that does not exist
        ext[:nyh, :nxh] = cls
        rowseen = ext[:, mx(0)]                               # (frame row, centre x): the class within |dx| <= nn of x
        colseen = ext[my(0), :]                               # (centre y, frame column): within |dy| <= nn of y
        seen = ext[my(0)[:, None], mx(0)[None, :]]
        state.append([ext, rowseen, colseen, seen])
    top = int(cap[isband].max()) if isband.any() else 0
    xi, yi = xs[None, :], ys[:, None]
    for nn in range(1, top + 1):
        if not ((radius == -1) & (cap >= nn)).any():
            break
        xa, xb, ya, yb = mx(-nn), mx(nn), my(-nn), my(nn)
        for st in state:
            ext, rowseen, colseen, seen = st
            rowseen |= ext[:, xa] | ext[:, xb]
            colseen |= ext[ya, :] | ext[yb, :]
            seen |= rowseen[ya[:, None], xi] | rowseen[yb[:, None], xi] | colseen[yi, xa[None, :]] | colseen[yi, xb[None, :]]
        both = state[0][3] & state[1][3]
        radius[(radius == -1) & both & (cap >= nn)] = nn
    return radius


def summary_of(radius):
    """[band cells, with a radius, with -1, largest radius] from the plane (a band cell is one with radius != 0)."""
    pos = radius[radius > 0]
    return [int((radius != 0).sum()), int(pos.size), int((radius == -1).sum()), int(pos.max()) if pos.size else 0]


def hist_of(radius, nhist):
    h = np.zeros(nhist, dtype=np.int64)
    h[0] = (radius == -1).sum()
    pos = np.minimum(radius[radius > 0], nhist - 1)
    h += np.bincount(pos, minlength=nhist)[:nhist]
    return h


def regimes_of(radius):
    r = radius
    return dict(strip=int(((r >= 1) & (r <= 16)).sum()), wide=int(((r >= 17) & (r <= 32)).sum()),
                table=int(((r >= 33) & (r <= 127)).sum()), beyond=int((r > 127).sum()), none=int((r == -1).sum()))


def brute(mask_f, maxdist, halo, bnd, band, cells):
    """contrast_global's loop, cell by cell (for spot checks of the model itself): {(x, y): radius}."""
    nyh, nxh = mask_f.shape
    ny, nx = nyh - 2 * halo, nxh - 2 * halo
    if band is not None:
        bnd = BND_HALO
    isband, land = classify(mask_f, maxdist, ny, nx, halo, bnd)
    cap = cap_plane(ny, nx, halo, bnd, band)
    out = {}
    for (x, y) in cells:
        if not isband[y, x]:
            out[(x, y)] = 0
            continue
        r = -1
        for nn in range(1, int(cap[y, x]) + 1):
            d = np.arange(-nn, nn + 1)
            X = map_x(x + d, nx, halo, bnd, band)
            Y = map_y(y + d, ny, halo, bnd, band)
            X, Y = X[X >= 0], Y[Y >= 0]
            w = land[np.ix_(Y, X)]
            if w.any() and not w.all():
                r = nn
                break
        out[(x, y)] = r
    return out
