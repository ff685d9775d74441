"""Inputs of the tests of a band's moving coast (tests/test_band_ice_gpu.py, tests/test_band_runner_ice_gpu.py): the shapes,
one per distance kernel, and for each a fractional land field and twelve ice planes on the whole grid, which the tests cut
into three latitude bands.  Numpy only; the tests assert from the oracle what each plane is meant to do.

The land is tests/test_band_setup_gpu.py's (fractional blobs, so that the two land rules differ), with open sea in the 5 x 5
cells round every cell a plane toggles (a toggled cell is then an island: the coast moves whatever the rule) and in one box
north of the middle band, so that the coast plane 5 makes at the outermost source row is the nearest one of the band's last
own row.  Rows below are rows of the globe; (r0, r1) is the middle band.
"""
import numpy as np

from seabreeze_param_amd import synth

#        id              nx  kwin halo  band heights        kernel
CASES = [("BITS32",      320, 15, 16, (33, 33, 33), "BITS32"),
         ("BITS32-halo", 320, 15, 19, (33, 33, 33), "BITS32"),        # halo > kwin + 1: the frame offset is not the window
         ("BITS64",      320, 20, 21, (31, 36, 32), "BITS64"),
         ("BITS_SMALL",   96, 15, 16, (33, 33, 33), "BITS_SMALL"),
         ("BYTES",        24, 15, 16, (17, 21, 19), "BYTES"),         # no bit plane: the whole path
         ("WIDE",        320, 40, 41, (50, 50, 50), "WIDE"),
         ("WIDE-odd",    320, 40, 41, (49, 51, 50), "WIDE"),
         ("BITS32-700",  700, 15, 16, (33, 33, 33), "BITS32"),        # three tiles, a ragged last word, the seam
         # a last word of 6 cells whose reach spans up to 31 rows: the delta kernel's mark loop takes more than one stride
         ("SMALL-70",     70, 15, 16, (33, 33, 33), "BITS_SMALL")]

PLANES = ["1 initial ice", "2 the same plane", "3 values changed, no cell crosses a threshold", "4 one interior cell crosses",
          "5 cells at rows r0-(k+1) and r1+k", "6 a cell at row r0-(k+2)", "7 cells at column 0 and nx-1",
          "8 a cell in the last word", "9 cells in the pole rows", "10 an ice edge moved across a cut", "11 back to 1",
          "12 half the grid iced"]


def land_flags(land, ci, rule):
    """EdgesGrid::land in numpy, in the fields' precision (ref: sobel.f90:51,69; generic :325-336)."""
    if rule == 0:
        return land + ci > land.dtype.type(0.4)
    return np.where(ci <= land.dtype.type(0.2), land >= land.dtype.type(0.5), land + ci >= land.dtype.type(0.5))


def toggles(nx, k, bands):
    """plane -> [(row, column)] of the cells it toggles"""
    ny = bands[-1][1]
    r0, r1 = bands[1]
    small = nx < 64
    c_a, c_s, c_9 = (4, 8, 19) if small else (nx // 4, nx // 2, nx // 8)
    c_n = nx // 2 if small else 5 * nx // 8
    row = r0 + 2                                                  # (its ring lies outside the windows of row r1-1)
    return {0: [(r0 - 6, c_9)],                                   # never toggled: ice of 0.45 over open sea, land under rule 0 alone
            4: [(row, c_a)], 5: [(r0 - (k + 1), c_s), (r1 + k, c_n)], 6: [(r0 - (k + 2), c_s + 6)],
            7: [(row, 0), (row, nx - 1)], 8: [(row, nx - 3)], 9: [(0, c_9), (ny - 1, c_9)]}


def sheet_columns(nx):
    return (10, 16) if nx < 64 else (nx // 4 + 8, nx // 4 + 8 + min(30, nx // 6))


def make(nx, k, bands, dt, level):
    """-> land (ny, nx), [12 ice planes]"""
    ny = bands[-1][1]
    r0, r1 = bands[1]
    r = synth.hash_uniform((ny, nx), 3, 8)
    s = r + np.roll(r, 1, 1) + np.roll(r, 1, 0)
    land = np.round(np.clip((s - level) / 0.4, 0, 1) * 8) / 8
    ice = np.where(synth.hash_uniform((ny, nx), 4, 8) > 0.93, 0.35, 0.0)
    tg = toggles(nx, k, bands)
    cols = np.arange(nx)
    for cells in tg.values():
        for y, x in cells:
            near = np.minimum((cols - x) % nx, (x - cols) % nx) <= 2
            land[max(0, y - 2):y + 3, near] = 0
            ice[max(0, y - 2):y + 3, near] = 0
    # the box: every source row and column of the windows of (r1-1, c_n), and one more each way
    c_n = tg[5][1][1]
    near = np.minimum((cols - c_n) % nx, (c_n - cols) % nx) <= k + 1
    land[r1 - 1 - k - 1:min(ny, r1 + k + 3), near] = 0
    ice[r1 - 1 - k - 1:min(ny, r1 + k + 3), near] = 0
    land, ice = np.ascontiguousarray(land, dt), np.ascontiguousarray(ice, dt)
    # an ice sheet over the sea of band 0's last three rows; plane 10 moves its edge into the middle band's first row
    x0, x1 = sheet_columns(nx)
    sheet = np.zeros((ny, nx), bool)
    sheet[r0 - 3:r0, x0:x1] = True
    p1 = np.where(sheet & (land == 0), dt(0.6), ice).astype(dt)
    p1[tg[0][0]] = dt(0.45)

    def toggled(p, n):
        q = p.copy()
        for y, x in tg[n]:
            assert land[y, x] == 0
            q[y, x] = dt(0.0) if q[y, x] > 0.3 else dt(0.6)
        return q

    # plane 3: other values wherever that leaves the land flag of both rules alone
    cand = np.where(p1 > 0, p1 * dt(0.9), dt(0.1) * (land == 0)).astype(dt)
    keep = np.ones((ny, nx), bool)
    for rule in (0, 1):
        keep &= land_flags(land, cand, rule) == land_flags(land, p1, rule)
    p3 = np.where(keep, cand, p1).astype(dt)
    p4 = toggled(p3, 4)
    p5 = toggled(p4, 5)
    p6 = toggled(p5, 6)
    p7 = toggled(p6, 7)
    p8 = toggled(p7, 8)
    p9 = toggled(p8, 9)
    p10 = p9.copy()
    edge = np.zeros((ny, nx), bool)
    edge[r0, x0:x1] = True
    p10[edge & (land == 0)] = dt(0.6)
    p12 = p1.copy()
    p12[:, :nx // 2][land[:, :nx // 2] == 0] = dt(0.7)
    return land, [p1, p1.copy(), p3, p4, p5, p6, p7, p8, p9, p10, p1.copy(), p12]
