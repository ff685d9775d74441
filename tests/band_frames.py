"""Ghost-celled frames of latitude bands cut from a whole grid with numpy slices, for the tests of the band-local coast setup
(tests/test_band_setup_gpu.py, tests/test_dist_directed_gpu.py): the cut-side ghost rows of a frame are the neighbour's rows
(what swap_bounds would deliver), everything else outside the interior is a fill value that must never be read, and output
frames carry a sentinel that only the interior may lose."""
import numpy as np

SENTINEL = -777.0


def cuts_of(heights):
    r = np.concatenate(([0], np.cumsum(heights)))
    return [(int(r[i]), int(r[i + 1])) for i in range(len(heights))]


def frame(full, r0, r1, h, fill=np.nan):
    """Rows r0 .. r1-1 of `full` in a frame of h ghost cells: the cut-side ghost rows are the neighbour's rows, everything
    else outside the interior is `fill`."""
    ny, nx = full.shape
    f = np.full((r1 - r0 + 2 * h, nx + 2 * h), fill, dtype=full.dtype)
    lo, hi = max(r0 - h, 0), min(r1 + h, ny)
    f[h - (r0 - lo):h + (hi - r0), h:h + nx] = full[lo:hi]
    return f


def frame_lat(lat, r0, r1, h):
    f = np.full(r1 - r0 + 2 * h, np.nan, dtype=lat.dtype)
    lo, hi = max(r0 - h, 0), min(r1 + h, lat.size)
    f[h - (r0 - lo):h + (hi - r0)] = lat[lo:hi]
    return f


def interior(f, h):
    return f[h:f.shape[0] - h, h:f.shape[1] - h] if h else f


def only_interior_written(f, h):
    g = f.copy()
    interior(g, h)[...] = SENTINEL
    return np.all(g == SENTINEL)


def band_dist(ctx, coast, land, lon, lat, bands, h, kwin, maxdist=180.0):
    ny = land.shape[0]
    rows = []
    for r0, r1 in bands:
        out = np.full((r1 - r0 + 2 * h, land.shape[1] + 2 * h), SENTINEL, dtype=land.dtype)
        ctx.band_get_dist(frame(coast, r0, r1, h), frame(land, r0, r1, h), lon, frame_lat(lat, r0, r1, h), h,
                          r0 == 0, r1 == ny, kwin, maxdist=maxdist, out=out)
        assert only_interior_written(out, h), f"band {r0}:{r1}: ghost cells of cdist were written"
        rows.append(interior(out, h).copy())
    return np.concatenate(rows)
