"""What a changed coast cell can reach, by brute force (numpy), for the tests of the stream's moving coast
(tests/test_ice_plan.py, tests/test_stream_ice_gpu.py).

The rule is the distance kernels' and the reference's (seabreeze_param_amd/csrc/sb_coast_kernels.hip: k_dist's loops;
oracle/sb_oracle.f90: get_dist; ref sobel.f90:152-191): target (xx, yy) reads the coast cells of rows yy-k .. yy+k that lie
inside the grid (rows past it add no sources) and of columns (xx - jj) mod nx, jj = -k .. k -- every column, once, where
2k+1 >= nx.  So a changed cell (x, y) reaches the targets of rows y-k .. y+k, clamped, and columns (x + d) mod nx, d = -k .. k.
Nothing here is produced by the library or its headers.
"""
import numpy as np

TILE = 256


def tiles(nx):
    return (nx + TILE - 1) // TILE


def _reach(nx, ny, k, cells, width):
    m = np.zeros((ny, tiles(nx)), bool)
    d = np.arange(-width, width + 1)
    for x, y in cells:
        cols = np.unique(((x + d) % nx) // TILE)
        m[max(0, y - k):min(ny - 1, y + k) + 1, cols] = True
    return m


def brute_marks(nx, ny, k, cells):
    """(ny, tiles) bool: the (row, tile) pairs that hold a target whose window holds a changed cell."""
    return _reach(nx, ny, k, cells, k)


def cap_marks(nx, ny, k, cells):
    """(ny, tiles) bool: rows +-k and the tile columns covering +-(k + 63) of a changed cell -- a 64-cell word is the unit
    the coast is compared in, so a mark may lie up to 63 columns beyond a changed cell's own reach, and no further."""
    return _reach(nx, ny, k, cells, k + 63)
