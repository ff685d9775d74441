"""Directed fields for the coast-distance kernels (k_dist, k_dist_bits_small, k_dist_bits<32|64>, k_dist_wide): coast planes
written cell by cell, so that the window edge, the reset, the own-row seam split, the row stop and k_dist_wide's pass
boundaries are reached on purpose.  tests/test_dist_cases.py holds them to the numpy model (tests/dist_ref.py), the oracle
and the launch plan on the CPU, tests/test_dist_directed_gpu.py holds the kernels to them.

Shapes (SHAPES): the smallest that reach each kernel of sb_dist_kernel(nx, k) and each of its bounds (nx = 2k + 256 | 2k + 257,
2k | 2k + 1, k = 15 | 16, 31 | 32; k_dist_wide also narrower than its window), 600 columns where a workgroup column must be whole, ragged and end in a bit word of 24
bits; ny is odd (the last two-row workgroup holds one row) and at least 2k + 3.

Coordinate sets: 1 the full circle in order, 38 N + 0.25 degrees a row (a farther row often holds the nearer cell: the
meridians converge); 2 a regional frame that does not close; 3 every longitude twice, latitudes descending; 4 set 1 with
the latitudes permuted.  What the host may cut under each (cuts_claim) is written down here by hand and checked against
sb_dist_plan.hpp by the CPU module.

Families: A lone cells, more than 2k + 1 apart both ways (every target sees at most one source), packed greedily into as
many fields as it takes; each field once with 2 maxdist inside the window's reach and once with the reset out of reach.
B clusters of two or three sources in one target's window.  C the own row across the seam, maxdist of about a column.
V values: coast and mask hold negative numbers, both zeros and fractions."""
import functools
from collections import namedtuple

import numpy as np

import dist_ref

NEAREST, CIRCLE, INNER, ROWS = 1, 2, 4, 8
BIG = dist_ref.BIG
FAR = 5900.0                                                     # maxdist with the reset out of every window's reach

Shape = namedtuple("Shape", "kernel k nx")
SHAPES = [Shape("BITS32", 15, 600), Shape("BITS32", 15, 287), Shape("BITS32", 1, 600), Shape("BITS32", 0, 600),
          Shape("BITS64", 16, 600), Shape("BITS64", 31, 600), Shape("BITS64", 31, 319),
          Shape("BITS_SMALL", 31, 318), Shape("BITS_SMALL", 31, 63), Shape("BITS_SMALL", 15, 286),
          Shape("BYTES", 31, 62), Shape("BYTES", 20, 30),
          Shape("WIDE", 32, 600), Shape("WIDE", 40, 600), Shape("WIDE", 62, 600), Shape("WIDE", 63, 600), Shape("WIDE", 40, 100),
          Shape("WIDE", 63, 100)]                                # (a window of 127 columns on 100: every column once, some bits twice)
KERNELS = ("BYTES", "BITS_SMALL", "BITS32", "BITS64", "WIDE")

Case = namedtuple("Case", "name family shape k nx ny cset maxdist coast mask lon lat kernel cuts")


def shape_id(s):
    return f"{s.kernel}-k{s.k}-nx{s.nx}"


def ny_of(k):
    return (3 * k + 4) | 1 if k >= 15 else 33


def kernel_claim(nx, k):
    """which kernel serves (nx, k)."""
    if k >= 32:
        return "WIDE"
    if 2 * k + 1 > nx:
        return "BYTES"
    if nx < 2 * k + 257:
        return "BITS_SMALL"
    return "BITS32" if k <= 15 else "BITS64"


def coords(cset, nx, ny):
    lon = 360.0 * np.arange(nx) / nx
    lat = 38.0 + 0.25 * np.arange(ny)
    if cset == 2:
        lon = 100.0 + 0.3 * np.arange(nx)                        # folds at 180 degrees inside the frame
    if cset == 3:
        lon = np.repeat(720.0 * np.arange((nx + 1) // 2) / nx, 2)[:nx]
        lat = lat[::-1].copy()
    if cset == 4:
        lat = np.random.default_rng(4).permutation(lat)
    return lon, lat


def cuts_claim(cset, nx, k):
    """What the coordinates allow a kernel to leave out, by hand."""
    short = k * 360.0 / nx < 170.0                               # the window spans less than half the circle
    if cset == 1:
        return NEAREST | CIRCLE | INNER | ROWS if short else ROWS
    if cset == 2:                                                # the closing step is 360 - 0.3 (nx - 1) degrees
        return NEAREST | CIRCLE | INNER | ROWS if k == 0 else INNER | ROWS
    if cset == 3:                                                # a step of zero degrees: in no order
        return ROWS
    return CIRCLE | INNER if short else 0


def maxdist_inside(k):
    """2 maxdist inside the window's reach (a row is 27.8 km): 180 km from k = 15 on.  With k = 0 the only distance is 0.5."""
    return 180.0 if k >= 15 else {0: 0.2, 1: 15.0}.get(k, 10.0 * k)


def sign_mask(nx, ny):
    return ((np.add.outer(np.arange(ny), np.arange(nx)) % 7) < 3).astype(np.float64)


def _cdx(a, b, nx):
    d = abs(a - b) % nx
    return min(d, nx - d)


def pack(groups, nx, k):
    """Groups of sources [(row, col), ...] into fields, first fit: two groups share a field when every pair of their sources is
    more than 2k + 1 apart in rows or in columns (round the seam), so no target sees both."""
    fields = []
    for g in groups:
        for f in fields:
            if all(abs(y - v) > 2 * k + 1 or _cdx(x, u, nx) > 2 * k + 1 for h in f for (v, u) in h for (y, x) in g):
                f.append(g)
                break
        else:
            fields.append([g])
    return [[cell for g in f for cell in g] for f in fields]


def lone_sources(nx, ny, k):
    """Family A's sources: every column residue mod 64 (every column of a grid narrower than that) spread over the 64-column
    spans, the seams by name, a source in every span; rows of both parities, the named rows, and rows with k rows on both sides."""
    # a residue's source stands k columns clear of the seam, so that its whole window keeps the residue's alignment (the
    # targets of a window that wraps lie at other residues unless nx is a multiple of 64); where a grid is too narrow for
    # that, every column holds a source in some field
    clear = [[c for c in range(r, nx, 64) if k <= c <= nx - 1 - k] for r in range(64)]
    if all(clear):
        cols = [cs[(5 * r) % len(cs)] for r, cs in enumerate(clear)]
        cols += [0, 1, k - 1, k, k + 1, nx - 1, nx - 2, nx - k - 1, nx - k, 63, 64, 255, 256, 64 * (nx // 64)]
        cols += list(range(32, nx, 64))
    else:
        cols = list(range(nx))
    cols = list(dict.fromkeys(c for c in cols if 0 <= c < nx))
    rows = [k, 0, k + 1, ny - 1, ny - 1 - k, 1, ny - 2 - k, ny - 2, ny // 2, ny // 2 + 1]
    rows = list(dict.fromkeys(r for r in rows if 0 <= r < ny))
    # (the row list and the column list have lengths without a common cycle that would tie a seam column to one row only)
    return [[(rows[n % len(rows)], c)] for n, c in enumerate(cols)] + [[(r, (37 * n + 5) % nx)] for n, r in enumerate(rows)]


def clusters(nx, ny, k):
    """Family B's clusters, as offsets (rows, columns) from an anchor."""
    pats = [((0, 0), (0, 1)), ((0, 0), (0, k)), ((0, 0), (0, k + 1)), ((0, 0), (0, 2 * k)), ((0, 0), (1, 0)), ((0, 0), (2, 0)),
            ((0, 0), (-1, k)), ((0, 0), (-3, k // 2)), ((0, 0), (-(k // 2), 3)), ((0, 0), (-(k - 1), 1)), ((0, 0), (-2, -k)),
            ((0, 0), (-1, -3), (-4, 2))]
    if k >= 32:
        pats += [((0, 0), (31, 0)), ((0, 0), (32, 0)), ((0, 0), (-31, 2), (32, -2))]
    out = []
    for n, p in enumerate(pats):
        y0 = max(k, 4) + n % 2                                   # (anchors of both row parities; the first ones across the seam)
        x0 = (nx - 4 + 71 * n) % nx
        g = sorted({(y0 + dy, (x0 + dx) % nx) for dy, dx in p})
        assert all(0 <= y < ny for y, _ in g), (nx, ny, k, p)
        out.append(g)
    return out


def seam_rows(nx, ny, k):
    """Family C: the own row across the seam.  Fields of one or two rows (2k + 2 apart), each row with the named columns."""
    fields = []
    for cols in ((nx - 3, 0, 7), (nx - 3, 0, 7), (nx - 1,), (k + 2,)):
        r = k + len(fields) % 2
        rows = [r] + ([r + 2 * k + 2] if r + 2 * k + 2 < ny else [])
        fields.append([(y, c % nx) for y in rows for c in cols])
    return fields


def _plane(cells, nx, ny):
    coast = np.zeros((ny, nx))
    for y, x in cells:
        coast[y, x] = 1.0
    return coast


def _settle(coast, lon, lat, k, maxdist):
    """Nudge maxdist until no early-class minimum lies within 1e-4 relative of 2 maxdist: a reset must not hang on rounding."""
    early, _ = dist_ref.dist_planes(coast, lon, lat, k)
    e = early[np.isfinite(early)]
    for _ in range(50):
        if not np.any(np.abs(e / (2 * maxdist) - 1.0) < 1e-4):
            return maxdist
        maxdist *= 1.0007
    raise AssertionError("no maxdist away from every early-class minimum")


def column_km(cset, nx, lat_deg):
    step = {1: 360.0 / nx, 2: 0.3}[cset]
    return step * D2R_KM * np.cos(np.radians(lat_deg))


D2R_KM = dist_ref.R_EARTH * dist_ref.D2R


@functools.lru_cache(maxsize=2)                                  # (a shape's planes are released when the tests move on)
def cases_of(shape):
    kern, k, nx = shape
    ny = ny_of(k)
    assert kernel_claim(nx, k) == kern and ny % 2 == 1 and ny >= 2 * k + 3
    mask = sign_mask(nx, ny)
    out = []

    def add(family, label, cells, cset, maxdist):
        lon, lat = coords(cset, nx, ny)
        coast = _plane(cells, nx, ny)
        md = _settle(coast, lon, lat, k, maxdist)
        out.append(Case(f"{shape_id(shape)}-{family}{label}-set{cset}-md{maxdist:g}", family, shape, k, nx, ny, cset, md, coast,
                        mask, lon, lat, kern, cuts_claim(cset, nx, k)))

    for n, cells in enumerate(pack(lone_sources(nx, ny, k), nx, k)):
        for cset in (1, 2):
            for md in (maxdist_inside(k), FAR):
                add("A", n, cells, cset, md)
    if k >= 1:
        for n, cells in enumerate(pack(clusters(nx, ny, k), nx, k)):
            for cset in (1, 2, 3, 4):
                add("B", n, cells, cset, maxdist_inside(k))
        for n, cells in enumerate(seam_rows(nx, ny, k)):
            for cset in (1, 2):
                # 2 maxdist is two and a half columns at the rows' latitude (half a column with k = 1): the class decides
                # most of the own row
                add("C", n, cells, cset, 0.5 * min(2.5, k - 0.5) * column_km(cset, nx, 38.0 + 0.25 * cells[0][0]))
    return tuple(out)


def all_cases():
    return [c for s in SHAPES for c in cases_of(s)]


_expected = {}


def expected(case):
    """The model's fp64 field of a case (computed once; callers must not write to it).  The fields of one shape are kept at a
    time: the tests go shape by shape."""
    if _expected.get("shape") != case.shape:
        _expected.clear()
        _expected["shape"] = case.shape
    if case.name not in _expected:
        e = dist_ref.dist_model(case.coast, case.mask, case.lon, case.lat, case.maxdist, case.k)
        e.setflags(write=False)
        _expected[case.name] = e
    return _expected[case.name]


VALUE_SHAPES = [Shape("BITS32", 15, 600), Shape("BYTES", 20, 30)]


def value_case(shape):
    """coast holds -1, -0.0, 0.25 and 2, mask -0.5, -0.0, 0, 0.3 and 1: the reference's tests are coast > 0 and mask > 0."""
    kern, k, nx = shape
    ny = ny_of(k)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    coast = np.where((yy + xx) % 2 == 0, -1.0, -0.0)
    src = ((yy % 11 == 3) & (xx % 13 == 5))
    coast[src] = np.where((yy + xx)[src] % 3 == 0, 0.25, 2.0)
    mask = np.array([-0.5, -0.0, 0.0, 0.3, 1.0])[(3 * yy + xx) % 5]
    lon, lat = coords(1, nx, ny)
    md = _settle(coast, lon, lat, k, maxdist_inside(k))
    return Case(f"{shape_id(shape)}-V", "V", shape, k, nx, ny, 1, md, coast, mask, lon, lat, kern, cuts_claim(1, nx, k))


def sources_of(case, y, x):
    """The sources whose window holds (y, x): [(i, j, row offset i - y, window bit)], bit b of a target's window being column
    x - k + b (a source met twice, 2k + 1 > nx, is listed twice)."""
    k, nx = case.k, case.nx
    out = []
    for i, j in zip(*np.nonzero(case.coast > 0)):
        if abs(i - y) <= k:
            out += [(int(i), int(j), int(i - y), b) for b in range(2 * k + 1) if (x - k + b) % nx == j]
    return out


def first_difference(case, got, want, rel):
    """None, or a sentence that names the first cell of `got` that breaks the rule of _check_dist against `want`."""
    bad = ((got >= BIG) != (want >= BIG)) | (np.sign(got) != np.sign(want)) | \
          (np.abs(got - want) > rel * np.maximum(np.abs(want), 1.0))
    if not bad.any():
        return None
    y, x = (int(v) for v in np.argwhere(bad)[0])
    err = float(np.max((np.abs(got - want) / np.maximum(np.abs(want), 1.0))[(got < BIG) & (want < BIG)], initial=0.0))
    return (f"{case.name}: {int(bad.sum())} cells differ (max rel err {err:.3e}), first (row {y}, column {x}): got {got[y, x]!r}, "
            f"want {want[y, x]!r}; sources in its window (row, column, row offset, window bit): {sources_of(case, y, x)[:6]}")
