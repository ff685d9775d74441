"""get_dist as a numpy gather in fp64, written from the reference's scatter (oracle/sb_oracle.f90:451-507, sobel.f90:91-193)
and not from the kernels: for tests/dist_cases.py, tests/test_dist_cases.py and tests/test_dist_directed_gpu.py.

The reference sweeps the grid row by row, column by column.  A coast cell (coast > 0) at (i, j) writes
c = R 2 atan2(sqrt a, sqrt(1 - a)) + 0.5 into every cell of its window -- rows i-k .. i+k clamped to the grid (a clamped row is a
row the window holds anyway: nothing new), columns (j-k .. j+k) mod nx (some twice when 2k + 1 > nx) -- where c is smaller than
what stands there; and every cell, at the moment the sweep passes it, is put back to 12000 when it holds more than 2 maxdist.
As a gather per target: the minimum over the sources swept at or before the target (a row above, or the own row with
j <= x on wrapped indices: "early") is thrown away when it exceeds 2 maxdist; the minimum over the later sources is not.

`mutate` names one deliberate error (MUTANTS): what tests/test_dist_cases.py uses to show that the directed fields would
notice it."""
import numpy as np

BIG = 12000.0
R_EARTH = 6370.9989
D2R = 3.1415926 / 180.0                                          # the reference's own pi

MUTANTS = ("k-1", "k+1", "noreset", "reset_after_min", "side_class", "rowstop", "index_nearest")


def windows(coast, lon, lat, k, side_class=False):
    """For every source (i, j): the rows ys and columns xs of its window, the column offsets off (xs = (j + off) mod nx), the
    distances c[ys, xs] and whether the source is swept at or before each of those targets."""
    ny, nx = coast.shape
    phi = D2R * np.asarray(lat, np.float64)
    lon = np.asarray(lon, np.float64)
    lam = D2R * np.where(lon > 180, lon - 360.0, lon)
    off = np.arange(-k, k + 1)
    for i, j in zip(*np.nonzero(coast > 0)):
        ys = i + off
        ys = ys[(ys >= 0) & (ys < ny)]
        xs = (j + off) % nx
        dphi = phi[i] - phi[ys][:, None]
        dlam = lam[j] - lam[xs][None, :]
        a = np.sin(dphi / 2) ** 2 + (np.cos(phi[i]) * (np.cos(phi[ys])[:, None] * np.sin(dlam / 2) ** 2))
        c = R_EARTH * 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a)) + 0.5
        own_row = (off >= 0) if side_class else (j <= xs)        # the mutant: by the side of the window, not the wrapped index
        early = (i < ys)[:, None] | ((i == ys)[:, None] & own_row[None, :])
        yield int(i), int(j), ys, xs, off, c, early


def _grids(ys, xs, off, shape):
    Y = np.broadcast_to(ys[:, None], shape)
    X = np.broadcast_to(xs[None, :], shape)
    O = np.broadcast_to(off[None, :], shape)
    return Y, X, O


def _keep_rowstop(coast, lon, lat, k):
    """Each class keeps the own row and the nearest other row that holds a hit."""
    ny, nx = coast.shape
    near = np.full((2, ny, nx), 1 << 20)
    for i, j, ys, xs, off, c, early in windows(coast, lon, lat, k):
        Y, X, _ = _grids(ys, xs, off, c.shape)
        D = np.abs(Y - i)
        for cls, sel in ((0, early & (D > 0)), (1, ~early & (D > 0))):
            np.minimum.at(near[cls], (Y[sel], X[sel]), D[sel])

    def keep(i, j, Y, X, O, early):
        D = np.abs(Y - i)
        return (D == 0) | (D == near[np.where(early, 0, 1), Y, X])
    return keep


def _keep_index_nearest(coast, lon, lat, k):
    """Per sweep class, source row and side of the target's own column (the own column counts as left), only the hit nearest
    by column index."""
    ny, nx = coast.shape
    near = np.full((2 * k + 1, 2, 2, ny, nx), 1 << 14, np.int16)

    def key(i, Y, O, early):
        return (i - Y) + k, (O < 0).astype(np.intp), np.where(early, 0, 1)     # O < 0: the source lies right of the target

    for i, j, ys, xs, off, c, early in windows(coast, lon, lat, k):
        Y, X, O = _grids(ys, xs, off, c.shape)
        r, s, cls = key(i, Y, O, early)
        np.minimum.at(near, (r.ravel(), s.ravel(), cls.ravel(), Y.ravel(), X.ravel()), np.abs(O).astype(np.int16).ravel())

    def keep(i, j, Y, X, O, early):
        r, s, cls = key(i, Y, O, early)
        return np.abs(O) == near[r, s, cls, Y, X]
    return keep


def dist_planes(coast, lon, lat, k, mutate=None):
    """-> (early, late): the minimum distance per sweep class, inf where a class holds no hit."""
    ny, nx = coast.shape
    kk = max(k + {"k-1": -1, "k+1": 1}.get(mutate, 0), 0)
    keep = {"rowstop": _keep_rowstop, "index_nearest": _keep_index_nearest}.get(mutate)
    keep = keep(coast, lon, lat, kk) if keep else None
    early_p, late_p = np.full((ny, nx), np.inf), np.full((ny, nx), np.inf)
    for i, j, ys, xs, off, c, early in windows(coast, lon, lat, kk, side_class=mutate == "side_class"):
        Y, X, O = _grids(ys, xs, off, c.shape)
        ok = keep(i, j, Y, X, O, early) if keep else np.ones(c.shape, bool)
        e, l = early & ok, ~early & ok
        np.minimum.at(early_p, (Y[e], X[e]), c[e])
        np.minimum.at(late_p, (Y[l], X[l]), c[l])
    return early_p, late_p


def dist_model(coast, mask, lon, lat, maxdist, k, mutate=None):
    assert mutate is None or mutate in MUTANTS, mutate
    early, late = dist_planes(np.asarray(coast), lon, lat, k, mutate)
    early, late = np.minimum(early, BIG), np.minimum(late, BIG)
    if mutate == "reset_after_min":
        m = np.minimum(early, late)
        m[m > 2 * maxdist] = BIG
    else:
        if mutate != "noreset":
            early[early > 2 * maxdist] = BIG
        m = np.minimum(early, late)
    return np.where(m >= BIG, BIG, np.where(np.asarray(mask) > 0, m, -m))


def moved(a, b, rel=1e-9):
    """How many cells differ between two fields: another reach, another sign, or more than `rel` of max(|b|, 1 km)."""
    return int(np.count_nonzero(((a >= BIG) != (b >= BIG)) | (np.sign(a) != np.sign(b))
                                | (np.abs(a - b) > rel * np.maximum(np.abs(b), 1.0))))
