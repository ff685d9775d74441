"""numpy model of what an ice call of one UM tile marks (sb_um_tile_ice_*; seabreeze_param_amd/csrc/sb_ice_plan.hpp), the cuts
and the frames of its tests: tests/test_um_tile_ice_plan.py, tests/test_um_tile_ice_gpu.py, tests/test_fortran_um_tile_ice.py.
Written from the tile distance kernel's window rule, not from the header: a target (xx, yy) of the interior reads the coast
bits of rows yy-wj .. yy+wj and columns xx-wi .. xx+wi that lie inside the tile's SOURCE rectangle [-eW, nx+eE) x [-eS, ny+eN)
(interior coordinates, e* = min(window, domain cells beyond that side)) and nothing else.  The mark plane is the UM layout's
(tests/um_ice_ref.py): one byte per 4 x 64 workgroup of the interior.  The coast bit plane is aligned to the RECTANGLE: the
word of a cell at interior column x starts at rectangle column (x + eW) & ~63.

Cells are (x, y) in INTERIOR coordinates, negative or beyond the interior for ghost cells; words are (x0, s) in rectangle
coordinates.  A tile is (x0, x1, y0, y1), columns [x0, x1) and rows [y0, y1) of the domain, as in tests/um_tile_ref.py.
"""
import functools

import numpy as np

import um_ice_ref as uir

ROWS, COLS = uir.ROWS, uir.COLS

# the cuts of the GPU test's four cases (column bounds, row bounds) and what each is there for
#   a: a 10-column tile (nx < 64), and beside it a tile whose west side lies 10 < 15 cells from the domain's edge: eW = 10,
#      so the first word of its source rectangle straddles the interior's west edge
#   b: um_tile_ref.SPARSE_CUTS' unequal columns (a 13-column tile under a 40-cell window) and rows whose second tile lies
#      6 < 9 rows from the domain's edge
#   c: no window at all;  d: the window wider than the domain, every e* clipped by `beyond`
CASES = {
    "a": dict(nx=200, ny=70, win=(15, 15), cuts=((0, 10, 134, 200), (0, 23, 46, 70)), maxdist=180.0),
    "b": dict(nx=200, ny=70, win=(40, 9), cuts=((0, 70, 83, 200), (0, 6, 15, 70)), maxdist=180.0),
    "c": dict(nx=200, ny=70, win=(0, 0), cuts=((0, 67, 134, 200), (0, 23, 46, 70)), maxdist=180.0),
    "d": dict(nx=130, ny=37, win=(255, 255), cuts=((0, 65, 130), (0, 19, 37)), maxdist=180.0),
}


def beyond_of(tile, nx, ny):
    """the domain cells beyond the tile's west, east, south and north side"""
    x0, x1, y0, y1 = tile
    return (x0, nx - x1, y0, ny - y1)


def sources(win, beyond):
    """(eW, eE, eS, eN)"""
    wi, wj = win
    return (min(wi, beyond[0]), min(wi, beyond[1]), min(wj, beyond[2]), min(wj, beyond[3]))


def halo_for(case, extra=1):
    """the smallest ghost width that serves every tile of a case (e* + 1), and `extra` cells more"""
    c = CASES[case] if isinstance(case, str) else case
    import um_tile_ref as ut
    es = [sources(c["win"], beyond_of(t, c["nx"], c["ny"])) for t in ut.tiles(c["cuts"])]
    return (max(max(e[0], e[1]) for e in es) + 1 + extra, max(max(e[2], e[3]) for e in es) + 1 + extra)


def cut_frame(frame, tile, H, h):
    """the tile's frame with ghost width h = (hi, hj) out of a whole-domain FRAME with ghost width H >= h: in-domain ghost
    cells are the neighbours' cells, out-of-domain ones the whole-domain frame's own ghost cells"""
    x0, x1, y0, y1 = tile
    return np.ascontiguousarray(frame[y0 + H[1] - h[1]:y1 + H[1] + h[1], x0 + H[0] - h[0]:x1 + H[0] + h[0]])


def changed_cells(coast_a, coast_b, tile, e):
    """[(x, y)] in the tile's interior coordinates of the cells of its source rectangle whose coast flag differs between
    two whole-domain interior planes"""
    x0, x1, y0, y1 = tile
    eW, eE, eS, eN = e
    sub = lambda a: a[y0 - eS:y1 + eN, x0 - eW:x1 + eE] > 0
    ys, xs = np.nonzero(sub(coast_a) != sub(coast_b))
    return [(int(x) - eW, int(y) - eS) for x, y in zip(xs, ys)]


def words_of(cells, e):
    """the words (x0, s) of the rectangle's bit plane that hold the cells"""
    return sorted({((x + e[0]) & ~63, y + e[2]) for x, y in cells})


def word_cells(nx, e, x0, s):
    """the cells of a word, interior coordinates"""
    return [(x - e[0], s - e[2]) for x in range(x0, min(x0 + 64, nx + e[0] + e[1]))]


def brute_marks(nx, ny, win, cells):
    """brute force over the interior's targets: every target whose window holds one of `cells` marks its workgroup"""
    return uir.brute_marks(nx, ny, win[0], win[1], cells)


def reach(nx, ny, win, e, x0, s, dwi=0, dwj=0, tail=63, shift=None):
    """the rule restated: inclusive (g0, g1, t0, t1) of the word at rectangle columns x0 .. x0+63 of rectangle row s.  dwi,
    dwj, tail narrow it on purpose; shift=(dx, dy) replaces the origin (eW, eS) -- (0, 0) is sb_um_ice_reach taken as it
    stands, the mistake a tile instance is most likely to make."""
    dx, dy = (e[0], e[2]) if shift is None else shift
    return uir.reach(nx, ny, win[0], win[1], x0 - dx, s - dy, dwi=dwi, dwj=dwj, tail=tail)


def word_marks(nx, ny, win, e, cells, **narrow):
    m = np.zeros((uir.groups(ny), uir.tiles(nx)), bool)
    for x0, s in words_of(cells, e):
        g0, g1, t0, t1 = reach(nx, ny, win, e, x0, s, **narrow)
        m[g0:g1 + 1, t0:t1 + 1] = True
    return m


def cap_marks(nx, ny, win, e, cells):
    """the workgroups that lie at least partly inside rows y-wj-3 .. y+wj+3 and columns x-wi-63 .. x+63+wi+63 of a changed
    word whose first cell is interior (x, y): a mark outside them is over-marking beyond whole words, row groups and tiles"""
    wi, wj = win
    m = np.zeros((uir.groups(ny), uir.tiles(nx)), bool)
    for x0, s in words_of(cells, e):
        x, y = x0 - e[0], s - e[2]
        for g in range(uir.groups(ny)):
            if ROWS * g + ROWS - 1 < y - wj - 3 or ROWS * g > y + wj + 3:
                continue
            for t in range(uir.tiles(nx)):
                if COLS * t + COLS - 1 < x - wi - 63 or COLS * t > x + 63 + wi + 63:
                    continue
                m[g, t] = True
    return m


# ---- the whole-domain inputs the tiles are cut from ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def whole_inputs(case, prec):
    """H, land (ny, nx), landfrac frame, the twelve ice frames of tests/um_ice_cases.py with ghost width H = halo_for(case),
    and the whole-domain coast of every plane (interior, numpy restatement) -- once per case and precision, read-only"""
    import um_ice_cases as uic
    import um_setup_ref as ur
    c = CASES[case]
    H = halo_for(case)
    land, lf_L, planes = uic.make(c["nx"], c["ny"], H, np.float64 if prec == 8 else np.float32)
    co = [np.ascontiguousarray(ur.edges_um(lf_L, ci, *H)[H[1]:H[1] + c["ny"], H[0]:H[0] + c["nx"]]) for ci in planes]
    for a in [land, lf_L] + planes + co:
        a.setflags(write=False)
    return H, land, lf_L, planes, co


# the inputs of tests/test_um_tile_ice_gpu.py::test_only_marked_workgroups_are_written: case, the plane before, the plane
# (indices into the twelve) -- "a sea cell next to the coast becomes land", which lies in the interior of one tile of case a
# and in the ghost cells of its neighbours
WRITTEN = ("a", 2, 3)
