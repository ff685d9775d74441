"""What a changed coast cell can reach inside one latitude band, by brute force (numpy), for the tests of the band's
moving coast (tests/test_band_ice_plan.py, tests/test_band_ice_gpu.py, tests/test_band_runner_ice_gpu.py).

The rule is the distance kernels' and the reference's (oracle/sb_oracle.f90: get_dist; ref sobel.f90:152-191), seen from a
band that owns rows g0 .. g1-1 of a globe of nyg rows: target (xx, yy) reads the coast cells of rows yy-k .. yy+k inside the
globe and of columns (xx - jj) mod nx, jj = -k .. k.  So a changed cell (x, s) -- s a global row, inside the band or in a
neighbour's rows -- reaches the band's own rows within k of s and columns (x + d) mod nx, |d| <= k.  Marks are indexed by
own row (0 .. g1-g0-1).  Nothing here is produced by the library or its headers.
"""
import numpy as np

TILE = 256


def tiles(nx):
    return (nx + TILE - 1) // TILE


def source_rows(g0, g1, nyg, k):
    """The global rows a window of a band's own row can find a coast cell in: (first, last + 1)."""
    return max(g0 - k, 0), min(g1 + k, nyg)


def _reach(nx, g0, g1, k, cells, width):
    m = np.zeros((g1 - g0, tiles(nx)), bool)
    d = np.arange(-width, width + 1)
    cols = {}                                                     # column -> the tiles its reach touches
    for x, s in cells:
        lo, hi = max(s - k, g0), min(s + k, g1 - 1)
        if hi < lo:
            continue
        if x not in cols:
            cols[x] = np.unique(((x + d) % nx) // TILE)
        m[lo - g0:hi - g0 + 1, cols[x]] = True
    return m


def brute_marks(nx, g0, g1, k, cells):
    """(own rows, tiles) bool: the pairs that hold a target of the band whose window holds a changed cell (x, global row)."""
    return _reach(nx, g0, g1, k, cells, k)


def cap_marks(nx, g0, g1, k, cells):
    """Rows +-k and the tile columns covering +-(k + 63) of a changed cell: a 64-cell word is the unit the coast is compared
    in, so a mark may lie up to 63 columns beyond a changed cell's own reach, and no further."""
    return _reach(nx, g0, g1, k, cells, k + 63)


def changed_cells(coast_a, coast_b):
    """[(x, global row)] of the cells where two coast fields differ."""
    ys, xs = np.nonzero(np.asarray(coast_a) != np.asarray(coast_b))
    return list(zip(xs.tolist(), ys.tolist()))
