"""numpy model of what an ice call of the UM layout marks (sb_um_ice_*; seabreeze_param_amd/csrc/sb_ice_plan.hpp), for
tests/test_um_ice_plan.py, tests/test_um_ice_cases.py and tests/test_um_ice_gpu.py.  Written from the distance kernels'
window rule, not from the header: a target (xx, yy) reads the coast bits of interior rows yy-wj .. yy+wj and interior columns
xx-wi .. xx+wi that exist -- no wrap, no clamp.  The mark plane holds one byte per workgroup of the UM distance kernels:
ROWS target rows x COLS columns from interior cell (0, 0).

  brute_marks   the workgroups that hold a target whose window holds a changed CELL: what must be marked at least
  word_marks    the same for every cell of the 64-cell words that hold the changed cells: what the kernel, which compares
                whole words, marks exactly -- through `reach`, a restatement of the rule in Python
  cap_marks     the workgroups that lie at least partly inside rows y-wj-3 .. y+wj+3 and columns x0-wi-63 .. x0+63+wi+63 of a
                changed word: a mark outside them is over-marking beyond whole words, whole row groups and whole tiles
"""
import numpy as np

ROWS, COLS = 4, 64


def groups(ny):
    return (ny + ROWS - 1) // ROWS


def tiles(nx):
    return (nx + COLS - 1) // COLS


def changed_cells(coast_a, coast_b):
    """[(x, y)] of the interior cells whose coast flag differs (two interior (ny, nx) planes)"""
    ys, xs = np.nonzero((coast_a > 0) != (coast_b > 0))
    return [(int(x), int(y)) for x, y in zip(xs, ys)]


def words_of(cells):
    return sorted({(x & ~63, y) for x, y in cells})


def brute_marks(nx, ny, wi, wj, cells):
    """brute force over targets: every target whose window holds one of `cells` marks its workgroup"""
    yy, xx = np.arange(ny)[:, None], np.arange(nx)[None, :]
    hit = np.zeros((groups(ny) * ROWS, tiles(nx) * COLS), bool)
    for x, y in cells:
        hit[:ny, :nx] |= (np.abs(yy - y) <= wj) & (np.abs(xx - x) <= wi)
    return hit.reshape(groups(ny), ROWS, tiles(nx), COLS).any(axis=(1, 3))


def reach(nx, ny, wi, wj, x0, y, dwi=0, dwj=0, tail=63):
    """the rule restated: inclusive (g0, g1, t0, t1) of the word at columns x0 .. x0+63 of row y.  dwi, dwj, tail narrow it
    on purpose (tests/test_um_ice_plan.py shows that the lower bound catches that)."""
    wi, wj = max(wi + dwi, 0), max(wj + dwj, 0)
    r0, r1 = max(y - wj, 0), min(y + wj, ny - 1)
    c0, c1 = max(x0 - wi, 0), min(x0 + tail + wi, nx - 1)
    return r0 // ROWS, r1 // ROWS, c0 // COLS, c1 // COLS


def word_marks(nx, ny, wi, wj, cells, **narrow):
    m = np.zeros((groups(ny), tiles(nx)), bool)
    for x0, y in words_of(cells):
        g0, g1, t0, t1 = reach(nx, ny, wi, wj, x0, y, **narrow)
        m[g0:g1 + 1, t0:t1 + 1] = True
    return m


def cap_marks(nx, ny, wi, wj, cells):
    m = np.zeros((groups(ny), tiles(nx)), bool)
    for x0, y in words_of(cells):
        for g in range(groups(ny)):
            if ROWS * g + ROWS - 1 < y - wj - 3 or ROWS * g > y + wj + 3:
                continue
            for t in range(tiles(nx)):
                if COLS * t + COLS - 1 < x0 - wi - 63 or COLS * t > x0 + 63 + wi + 63:
                    continue
                m[g, t] = True
    return m


def cells_of_marks(marks, nx, ny):
    """(ny, nx) bool: the interior cells of the marked workgroups"""
    return np.repeat(np.repeat(marks, ROWS, 0), COLS, 1)[:ny, :nx]
