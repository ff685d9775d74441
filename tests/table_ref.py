"""Inputs, the closeness rule and a numpy model of the format for the table contrast (sb_set_table_contrast,
sb_table_kernels.hip): tests/test_table_contrast_gpu.py, tests/test_table_shapes_gpu.py,
tests/test_table_format_model.py.

The shapes follow from the kernels' constants: the row pass walks a row in chunks of 1024 columns, the column pass owns
256 columns x 64 rows per workgroup and keeps eight rows in flight, the sums are wrapping 64-bit fixed point with 36
fractional bits, the tables answer radii up to 127.

`table_thc` is the format restated in plain numpy from DESIGN section 2.4d -- not the kernels' control flow: whole-plane
cumulative sums, one pass over all cells per radius.
"""
from __future__ import annotations

import numpy as np

from conftest import relerr

DT_S = 7200.0
NZ = 2
TABLE_LAUNCHES = 6          # SCAN PREP TABLE_ROWS TABLE_COLS CONTRAST WIND
NAMES = ("ws", "wd", "thc", "sb_con")
TAB_FB = 36                 # fractional bits of the fixed point (SB_TAB_FB)
TAB_REACH = 127             # the largest radius the tables answer (SB_TAB_REACH)
GAMMA = -0.0060956          # ref: generic/sea_breeze_diag.f90:127-138

BIG = (1100, 900)           # nx, ny: two row chunks (76 ragged columns), five column blocks, fifteen row blocks, 900 % 8 == 4
BIG_RECT = (984, 790, 80)   # first column, first row, edge of the all-land square: across column 1024 and row 832
BIG_HALO = 8
REACH_GRID = (320, 10)      # nx, ny of the reach cases; the land block starts at column REACH_X0 and crosses the seam
REACH_X0 = 300
BLOCK = (160, 112, 80)      # nx, ny, block edge of the block grid of tests/test_table_contrast_gpu.py
CELSIUS = 290.0             # theta - CELSIUS: t0 of both signs


def close64(a, b, what):
    """|a - b| <= 1e-7 max(|b|, 1e-2); NaN exactly where b has NaN"""
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs"
    e = relerr(a, b, floor=1e-2)
    assert e < 1e-7, f"{what}: rel err {e}"


def mask_of(land, dt):
    return np.where(land, 100.0, -100.0).astype(dt)


def block_land(nx, ny, w, period, dx=0, dy=0, x0=0, y0=0):
    """a w x w block on columns x0 .. x0 + nx - 1 and rows y0 .. y0 + ny - 1 of the plane (period `period` along
    longitude, the block 40 columns before the seam; rows below 0 continue it), moved by dx columns and dy rows (the rows
    it leaves are sea)"""
    x = np.arange(x0, x0 + nx)[None, :] - dx
    y = np.arange(y0, y0 + ny)[:, None] - dy
    land = (((x - (period - 40)) % period) < w) & (y < w)
    return land & (y >= 0) if dy else land


def stripes_land(nx, ny):
    """12-column stripes: radii up to 6"""
    return np.ascontiguousarray(np.broadcast_to((np.arange(nx)[None, :] // 12) % 2 == 0, (ny, nx)))


def big_land():
    """the stripes of the big grid and one all-land square: radii up to 40 in its middle"""
    nx, ny = BIG
    x0, y0, w = BIG_RECT
    land = stripes_land(nx, ny)
    land[y0:y0 + w, x0:x0 + w] = True
    return land


def reach_land(w):
    """REACH_GRID with a land block of w columns over all rows from column REACH_X0 on, across the seam: its middle
    column is (w + 1) // 2 cells from the sea"""
    nx, ny = REACH_GRID
    return np.ascontiguousarray(np.broadcast_to(((np.arange(nx)[None, :] - REACH_X0) % nx) < w, (ny, nx)))


def zeros(n, dt, ny, nx):
    return [np.zeros((ny, nx), dt) for _ in range(n)]


def inputs(nx, ny, land, dt, steps=(1, 2), halo=0, shift=0.0):
    """-> (st, p, {tn: (theta, u, v)}, mask) from seabreeze_param_amd.synth, two levels; every cell in the band.  With
    ghost cells the fields are generated on the frame (land: the frame's) and p, u, v cut to its interior; theta is
    lowered by `shift` K."""
    from seabreeze_param_amd import synth
    st = synth.static_fields(nx + 2 * halo, ny + 2 * halo, dt)
    core = (slice(None), slice(halo, halo + ny), slice(halo, halo + nx))
    p = np.ascontiguousarray(synth.pressure_3d(st, NZ, dt)[core])
    per = {}
    for tn in steps:
        u, v = (np.ascontiguousarray(a[core]) for a in synth.wind_step(st, NZ, tn, dt))
        per[tn] = ((synth.theta_step(st, tn, np.float64) - shift).astype(dt), u, v)
    assert land.shape == (ny + 2 * halo, nx + 2 * halo)
    return st, p, per, mask_of(land, dt)


def t0_of(oracle, theta, z, sigma, halo=0):
    """t0 as every kernel forms it (ref: generic/sea_breeze_diag.f90:466-479, :186): the logistic's scalars from the
    interior of sigma (the oracle's), applied to ghost cells too"""
    ny, nx = sigma.shape
    inner = np.ascontiguousarray(sigma[halo:ny - halo, halo:nx - halo])
    sd, r = oracle.sigmoid_scalars(inner)
    return theta - (GAMMA * z) * (1 / (1 + np.exp(-sd * (sigma - r))))


def fixed_point(t0):
    """t0 rounded once to TAB_FB fractional bits (ties to even, as the fma of the row pass): int64"""
    return np.rint(np.asarray(t0, np.float64) * float(1 << TAB_FB)).astype(np.int64)


def frame_sum_over_2_64(t0):
    """the exact sum of the fixed-point frame -- the last entry of table A before it wraps -- over 2^64"""
    rows = fixed_point(t0).sum(axis=1)                   # (a row of a few thousand cells below 2^11 K fits 63 bits)
    return sum(int(v) for v in rows) / float(1 << 64)


def _prefix(v, dt):
    """inclusive 2-D prefix sums, wrapping in dt, with a zero row and column in front"""
    with np.errstate(over="ignore"):
        return np.pad(np.cumsum(np.cumsum(v.astype(dt), axis=0, dtype=dt), axis=1, dtype=dt), ((1, 0), (1, 0)))


def _rect(P, xa, xb, ya, yb):
    """sum over columns xa .. xb and rows ya .. yb (empty where xb < xa), wrapping"""
    with np.errstate(over="ignore"):
        return (P[yb + 1, xb + 1] - P[ya, xb + 1]) - (P[yb + 1, xa] - P[ya, xa])


def _window(P, bnd_global, nx, ny, h, y, x, r):
    """the sum of table P over the square of radius r round interior cells (y, x): DESIGN section 2.4d, index rules"""
    if not bnd_global:                                   # SB_BND_HALO: no wrap, no clamp
        return _rect(P, x + h - r, x + h + r, y + h - r, y + h + r)
    lo, hi = x - r, x + r
    west, east = lo < 0, hi >= nx                        # periodic: at most two column ranges while 2 r + 1 <= nx
    xa0 = np.where(west, lo + nx, lo)
    xb0 = np.where(west | east, nx - 1, hi)
    xa1 = np.zeros_like(x)
    xb1 = np.where(west, hi, np.where(east, hi - nx, -1))
    ya, yb = np.maximum(y - r, 0), np.minimum(y + r, ny - 1)
    below = np.maximum(r - y, 0).astype(P.dtype)         # a row beyond a pole is the edge row again, once per repetition
    above = np.maximum(y + r - (ny - 1), 0).astype(P.dtype)
    first, last = np.zeros_like(y), np.full_like(y, ny - 1)
    with np.errstate(over="ignore"):
        s = 0
        for xa, xb in ((xa0, xb0), (xa1, xb1)):
            s = s + _rect(P, xa, xb, ya, yb) + below * _rect(P, xa, xb, first, first) + above * _rect(P, xa, xb, last, last)
    return s


def table_thc(t0, land, bnd_global=True, halo=0):
    """-> (thc, nn) per interior cell from the tables of DESIGN section 2.4d: A, L (uint64, wrapping) and C (uint32) over
    the whole frame; the smallest radius whose square holds both classes from C; the two window sums, reinterpreted as
    signed; the means in float64.  NaN and 0 where the tables do not answer: no mixed square within TAB_REACH, the circle
    ((nx - 1) // 2) or the frame.  t0, land: the frame, (ny + 2 halo, nx + 2 halo)."""
    nyh, nxh = t0.shape
    ny, nx = nyh - 2 * halo, nxh - 2 * halo
    fx = fixed_point(t0).view(np.uint64)
    land = np.asarray(land, bool)
    A = _prefix(fx, np.uint64)
    L = _prefix(np.where(land, fx, np.uint64(0)), np.uint64)
    Cn = _prefix(land, np.uint32)
    yy, xx = np.mgrid[0:ny, 0:nx]
    yy, xx = yy.ravel(), xx.ravel()
    if bnd_global:
        assert halo == 0
        cap = np.full(yy.shape, min(TAB_REACH, (nx - 1) // 2))
    else:
        cap = np.minimum(TAB_REACH, np.minimum(np.minimum(xx, nx - 1 - xx), np.minimum(yy, ny - 1 - yy)) + halo)
    nn = np.zeros(yy.shape, np.int64)
    nl = np.zeros(yy.shape, np.int64)
    for r in range(1, int(cap.max()) + 1):
        todo = np.flatnonzero((nn == 0) & (cap >= r))
        if todo.size == 0:
            break
        c = _window(Cn, bnd_global, nx, ny, halo, yy[todo], xx[todo], r).astype(np.int64)
        hit = (c > 0) & (c < (2 * r + 1) ** 2)
        nn[todo[hit]] = r
        nl[todo[hit]] = c[hit]
    thc = np.full(yy.shape, np.nan)
    f = np.flatnonzero(nn > 0)
    y, x, r = yy[f], xx[f], nn[f]
    with np.errstate(over="ignore"):
        tl = _window(L, bnd_global, nx, ny, halo, y, x, r)
        ts = _window(A, bnd_global, nx, ny, halo, y, x, r) - tl
    ml = tl.view(np.int64).astype(np.float64) / nl[f]
    ms = ts.view(np.int64).astype(np.float64) / ((2 * r + 1) ** 2 - nl[f])
    mul = np.where(land[y + halo, x + halo], 1.0, -1.0)
    thc[f] = mul * ((ml - ms) / float(1 << TAB_FB))
    return thc.reshape(ny, nx), nn.reshape(ny, nx)
