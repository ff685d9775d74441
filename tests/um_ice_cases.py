"""Inputs of the tests of the UM layout's moving coast (tests/test_um_ice_cases.py, tests/test_um_ice_gpu.py,
tests/test_fortran_um_ice.py): the parameter sets, and for each a land fraction and twelve ice frames on the tdims_l layout.
Numpy only; tests/test_um_ice_cases.py asserts from the numpy restatement what each plane is meant to do.

The land is a ragged strip near the west edge (columns 3 .. nx/5 + y mod 3; columns 0 .. 2 are sea, so that a ghost cell
west of the interior can become land), open sea east of it, and in one row of open sea five cells of fractional land that
the rule calls sea until ice joins them: 0.1 (case 3), 0.4 twice and 0.25 twice (case 12).  landfrac's ghost cells are
edge-replicated, icefrac's are zero unless a plane says otherwise.
"""
import numpy as np

#       id   nx   ny   window    halo     maxdist  kernel
SETS = [("a", 200, 70, (15, 15), (15, 15), 180.0, "k_dist_um"),
        ("b", 200, 70, (7, 3), (7, 3), 180.0, "k_dist_um"),              # unequal
        ("c", 200, 70, (40, 33), (2, 1), 180.0, "k_dist_um_wide"),       # two passes: 33 > 30
        ("d", 200, 70, (0, 0), (1, 1), 180.0, "k_dist_um_wide"),
        ("e", 130, 37, (255, 255), (1, 1), 180.0, "k_dist_um_wide"),     # the window wider than the grid
        ("f", 200, 70, (15, 15), (15, 15), 30.0, "k_dist_um"),           # the reset fires
        ("g64", 64, 4, (15, 15), (15, 15), 180.0, "k_dist_um"),          # one workgroup
        ("g65", 65, 5, (15, 15), (15, 15), 180.0, "k_dist_um")]          # one ragged column and row more
GRIDS = ("dateline", "polar")       # um_setup_ref.GRIDS: across 180 degrees in the 0-360 convention, round the pole

PLANES = ["1 no ice", "2 the same plane", "3 values move, no class flips", "4 a sea cell next to the coast becomes land",
          "5 the same at interior cells (0, 0) and (nx-1, ny-1)", "6 a flip in the ghost ring, column -1",
          "7 a flip two cells out in the ghost frame", "8 a block of ice in open sea", "9 the block's edge moved by a row",
          "10 back to 1", "11 one more iced cell in every 4 x 64 tile", "12 knife edges of the rule"]
UNCHANGED = (1, 2, 6)               # indices of the planes that leave every word alone (cases 2, 3 and 7)


def kernel_of(win, halo):
    """sb_launch_dist_um_win's choice, restated"""
    return "k_dist_um" if win == halo and win[0] <= 31 and win[1] <= 31 else "k_dist_um_wide"


def layout(nx, ny):
    """where the planes put things (interior rows and columns)"""
    sr = 0 if ny < 8 else 2                                       # the row of the fractional cells
    c0 = nx // 5 + 6
    r0, r1 = ny // 3, 2 * ny // 3 + 1                             # the block's rows [r0, r1) ...
    b0, b1 = int(0.35 * nx), int(0.9 * nx)                        # ... and columns [b0, b1)
    return dict(sr=sr, lf01=(sr, c0), lf04=((sr, c0 + 4), (sr, c0 + 8)), lf025=((sr, c0 + 12), (sr, c0 + 16)),
                patch=(slice(ny - 1, ny), slice(nx // 2, nx // 2 + 9)), mid=(ny // 2, nx // 5 + (ny // 2) % 3 + 1),
                ring_row=min(ny - 1, ny // 2 + 1), block=(r0, r1, b0, b1), edge_cols=(b0 + 3, min(b0 + 103, b1)))


def land_of(nx, ny, dt):
    lay = layout(nx, ny)
    land = np.zeros((ny, nx), np.float64)
    for y in range(ny):
        land[y, 3:nx // 5 + y % 3 + 1] = 1.0 if y % 2 else 0.75
    land[lay["lf01"]] = 0.1
    for c in lay["lf04"]:
        land[c] = 0.4
    for c in lay["lf025"]:
        land[c] = 0.25
    return np.ascontiguousarray(land, dt)


def tile_cells(land):
    """one open-sea cell (landfrac 0, no fractional neighbour) per 4 x 64 tile, away from the tile's rim where it can be"""
    ny, nx = land.shape
    cells = []
    for g in range((ny + 3) // 4):
        for t in range((nx + 63) // 64):
            ys, xs = range(4 * g, min(4 * g + 4, ny)), range(64 * t, min(64 * t + 64, nx))
            pref = sorted(((y, x) for y in ys for x in xs), key=lambda c: (abs(c[0] - (4 * g + 1)), abs(c[1] - (64 * t + 40))))
            for y, x in pref:
                if not land[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].any():
                    cells.append((y, x))
                    break
            else:
                raise AssertionError(f"tile ({g}, {t}) has no open sea")
    return cells


def make(nx, ny, halo, dt):
    """-> land (ny, nx), landfrac_l, [12 icefrac_l frames] on the (ny + 2*hj, nx + 2*hi) layout"""
    hi, hj = halo
    dt = np.dtype(dt).type
    lay = layout(nx, ny)
    land = land_of(nx, ny, dt)
    lf_l = np.ascontiguousarray(np.pad(land, ((hj, hj), (hi, hi)), mode="edge"))
    zero = np.zeros_like(lf_l)

    def at(frame, y, x, v):                                       # interior coordinates; negative ones are ghost cells
        frame[y + hj, x + hi] = v

    p1 = zero.copy()
    p3 = p1.copy()
    p3[hj:hj + ny, hi:hi + nx][lay["patch"]] = dt(0.10)
    at(p3, *lay["lf01"], dt(0.3))
    base = p1.copy()                                              # what the later planes stand on: the patch moved on
    base[hj:hj + ny, hi:hi + nx][lay["patch"]] = dt(0.15)
    at(base, *lay["lf01"], dt(0.3))
    p4 = base.copy()
    at(p4, *lay["mid"], dt(0.6))
    p5 = p4.copy()
    at(p5, 0, 0, dt(0.6))
    at(p5, ny - 1, nx - 1, dt(0.6))
    p6 = p5.copy()
    at(p6, lay["ring_row"], -1, dt(0.6))
    p7 = p6.copy()
    if hi >= 2:
        at(p7, lay["ring_row"] - 1 if lay["ring_row"] else 0, -2, dt(0.6))
    elif hj >= 2:
        at(p7, -2, nx // 2, dt(0.6))                              # (else the frame has no such cell: the plane is plane 6)
    r0, r1, b0, b1 = lay["block"]
    p8 = p7.copy()
    p8[hj + r0:hj + r1, hi + b0:hi + b1] = dt(0.6)
    p9 = p8.copy()
    e0, e1 = lay["edge_cols"]
    p9[hj + r1, hi + e0:hi + e1] = dt(0.6)                        # (r1 <= ny - 1: 2 ny / 3 + 1 < ny for ny >= 4)
    p10 = p1.copy()
    p11 = p10.copy()
    for y, x in tile_cells(land):
        at(p11, y, x, dt(0.6))
    p12 = p1.copy()
    (a, b), (c, d) = lay["lf04"], lay["lf025"]
    at(p12, *a, dt(0.2))                                          # c <= 0.2: landfrac 0.4 alone decides -> sea
    at(p12, *b, np.nextafter(dt(0.2), dt(1)))                     # c > 0.2: 0.4 + c >= 0.5 -> land
    at(p12, *c, dt(0.25))                                         # 0.25 + 0.25 == 0.5 -> land
    at(p12, *d, np.nextafter(dt(0.5), dt(0)) - dt(0.25))          # 0.25 + c is one ulp below 0.5, exactly -> sea
    return land, lf_l, [p1, p1.copy(), p3, p4, p5, p6, p7, p8, p9, p10, p11, p12]
