"""A plain extended-precision reference of sigma's statistics and of what every contrast kernel derives from them
(ref: generic/sea_breeze_diag.f90:466-480): CPU only, numpy only, no project code.

The kernels reduce the interior of sigma to (n, mean, M2, min, max) in double -- by shifted sums about the FIRST INTERIOR
VALUE c, S1 = sum (x - c), S2 = sum (x - c)^2, M2 = S2 - S1^2/n, or by Chan merges of such sums -- and form from them, in
the working precision, std = 2/sqrt(M2/n) and r = (max - min)/4.  Here the same quantities come from two passes in
np.longdouble over the field AS THE KERNEL SEES IT (values already rounded to the working precision).

Error bounds (u = 2^-53; forward bounds of summation in double that hold for ANY order of adding; every quantity on the
right-hand side comes from this reference, never from the code under test):

  n, min, max   exact
  mean          |mean - ref| <= 2 u (S1abs + |mean|)         S1abs = sum |x - c|
                  (mean = c + S1/n: the sum of n terms errs by at most n u S1abs -- divided by n, u S1abs -- the
                  subtractions x - c are exact or err by u |x - c| each, and the final division and addition round once
                  each, relative to a result of at most |mean| + S1abs/n)
  M2            |M2 - ref| <= 4 n u S2
                  (M2 = S2 - S1^2/n.  S2 sums n non-negative terms: n u S2, their squares another u S2.  S1 errs by
                  n u S1abs, so S1^2/n by 2 |S1| n u S1abs / n = 2 u |S1| S1abs <= 2 n u S2, because |S1| S1abs / n <= S2
                  (Cauchy-Schwarz: S1abs^2 <= n S2, and |S1| <= S1abs).  Sum: < 4 n u S2.)

Relative to M2 the second bound is 4 n u kappa with kappa = S2/M2 >= 1: how badly the shift suits the sample.  The project's
tolerances for what follows from the scalars (1e-7 in double) can be asked only of inputs with 4 n u kappa <= 1e-7:
`assert_tame` states that about an input BEFORE the code under test sees it, so that a field that is too hostile fails
as a mistake of the test.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
GAMMA = -0.0060956                    # ref: generic/sea_breeze_diag.f90:166


@dataclass
class RefMoments:
    n: int
    mean: LD
    M2: LD
    mn: LD
    mx: LD
    c: LD                             # the shift: the first interior value
    S1abs: LD
    S2: LD
    kappa: float                      # S2 / M2 (0 where both vanish: a constant field)

    # ------------------------------------------------------------------ the bounds of the module docstring
    def mean_bound(self, u=U):
        return 2 * LD(u) * (self.S1abs + abs(self.mean))

    def m2_bound(self, u=U):
        return 4 * LD(self.n) * LD(u) * self.S2

    def tameness(self):
        """4 n u kappa: the bound of M2 relative to M2."""
        return 4.0 * self.n * U * self.kappa


def ref_moments(x) -> RefMoments:
    """Two passes in long double over `x`, an array that holds the interior in the working precision (any shape: the first
    element in C order is the first interior value)."""
    x = np.asarray(x)
    assert x.size > 0 and x.dtype in (np.float32, np.float64)
    w = x.astype(LD).ravel()
    n = w.size
    mean = w.sum(dtype=LD) / LD(n)
    M2 = ((w - mean) ** 2).sum(dtype=LD)
    c = w[0]
    S1abs = np.abs(w - c).sum(dtype=LD)
    S2 = ((w - c) ** 2).sum(dtype=LD)
    kappa = float(S2 / M2) if M2 > 0 else (0.0 if S2 == 0 else float("inf"))
    return RefMoments(n, mean, M2, w.min(), w.max(), c, S1abs, S2, kappa)


def ref_merge(a, b):
    """(n, mean, M2, min, max) of the union of two samples from those of each, in long double (Chan et al.)."""
    na, nb = LD(a[0]), LD(b[0])
    if nb == 0:
        return tuple(a)
    if na == 0:
        return tuple(b)
    n = na + nb
    d = LD(b[1]) - LD(a[1])
    return (n, LD(a[1]) + d * nb / n, LD(a[2]) + LD(b[2]) + d * d * na * nb / n, min(LD(a[3]), LD(b[3])), max(LD(a[4]), LD(b[4])))


def ref_scalars(m: RefMoments, dtype):
    """(std, r) as sigmoid_scalars in sb_device.hpp forms them from double moments: every operand rounded to the working
    precision T first, every operation in T."""
    T = np.dtype(dtype).type
    with np.errstate(divide="ignore"):
        std = T(2) / np.sqrt(T(np.float64(m.M2)) / T(m.n))
    r = (T(np.float64(m.mx)) - T(np.float64(m.mn))) / T(4)
    return T(std), T(r)


def ref_sigmoid(x, std, r):
    """1 / (1 + exp(-std (x - r))) in long double from scalars of the working precision (ref :480)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return 1 / (1 + np.exp(-LD(std) * (np.asarray(x).astype(LD) - LD(r))))


def ref_t0(theta, z, sigma, std, r, dtype):
    """t0 = theta - (gamma z) sigmoid(sigma) in long double (ref :167); gamma is the working precision's."""
    g = LD(np.dtype(dtype).type(GAMMA))
    return np.asarray(theta).astype(LD) - (g * np.asarray(z).astype(LD)) * ref_sigmoid(sigma, std, r)


def assert_tame(m: RefMoments, what=""):
    """The input allows the project's tolerances: 4 n u kappa <= 1e-7 (module docstring)."""
    assert m.tameness() <= 1e-7, f"test bug: {what} is too hostile a field, 4 n u kappa = {m.tameness():.3g} (kappa {m.kappa:.3g})"


def assert_moments(got5, m: RefMoments, what=""):
    """Five doubles (n, mean, M2, min, max) of the code under test against the bounds of the module docstring."""
    n, mean, m2, mn, mx = (float(v) for v in got5)
    assert n == m.n, f"{what}: n {n} != {m.n}"
    assert mn == float(m.mn) and mx == float(m.mx), f"{what}: min/max {mn} {mx} != {float(m.mn)} {float(m.mx)}"
    e_mean, e_m2 = abs(LD(mean) - m.mean), abs(LD(m2) - m.M2)
    assert e_mean <= m.mean_bound(), f"{what}: mean off by {float(e_mean):.3g}, bound {float(m.mean_bound()):.3g}"
    assert e_m2 <= m.m2_bound(), f"{what}: M2 off by {float(e_m2):.3g}, bound {float(m.m2_bound()):.3g}"
    return float(e_mean / m.mean_bound()) if m.mean_bound() > 0 else 0.0, float(e_m2 / m.m2_bound()) if m.m2_bound() > 0 else 0.0


# ---------------------------------------------------------------------------------------- the field families
FAMILIES = ("plain", "outlier_first", "negative", "orography", "tight_far", "constant")
PLACES = ("first", "row0_last", "last", "seg_end", "seg_start", "ragged_end")
HI, LO = 7.5, -2.5                    # the placed extremes: outside plain's [0, 5), exact in both precisions


def place(where, ny, nx):
    """(row, column) of a placed cell: the first cell, the last cell of the first row, the last cell of the last row, the
    cell at interior column 64 k - 1 (the last lane of a 64-cell segment that lies inside a row) and the cell after it in
    memory, the last cell of a row's ragged final segment -- rows in the middle of the grid for the last three."""
    mid = ny // 2
    k64 = 64 * ((nx - 1) // 64) - 1 if nx > 64 else min(nx, 64) - 1
    flat = min(mid * nx + k64 + 1, ny * nx - 1)
    return {"first": (0, 0), "row0_last": (0, nx - 1), "last": (ny - 1, nx - 1), "seg_end": (mid, k64),
            "seg_start": divmod(flat, nx), "ragged_end": (mid, nx - 1)}[where]


def family(name, ny, nx, seed=0, where=None, swapped=False):
    """One field of a family in float64, shape (ny, nx), from a seeded generator; the caller rounds it to the working
    precision.  `extreme_at` takes `where` from PLACES: the maximum sits there and the minimum at the next place of the
    list (the other way round with `swapped`)."""
    rng = np.random.default_rng(seed)
    plain = 5.0 * rng.random((ny, nx))
    if name == "plain":
        return plain
    if name == "outlier_first":
        plain[0, 0] = 800.0
        return plain
    if name == "negative":
        return plain - 1000.0
    if name == "orography":
        x = np.where(rng.random((ny, nx)) < 0.03, 500.0 * rng.random((ny, nx)), 0.0)
        x[0, 0] = 0.0
        return x
    if name == "tight_far":
        x = 1000.0 + 0.01 * rng.standard_normal((ny, nx))
        x[0, 0] = 1010.0
        return x
    if name == "constant":
        return np.full((ny, nx), 3.25)
    if name == "extreme_at":
        a = place(where, ny, nx)
        b = place(PLACES[(PLACES.index(where) + 1) % len(PLACES)], ny, nx)
        hi, lo = (LO, HI) if swapped else (HI, LO)
        if a != b:
            plain[b] = lo
        plain[a] = hi
        return plain
    raise ValueError(name)
