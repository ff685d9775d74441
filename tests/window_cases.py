"""Distance fields that put the deciding cell of the expanding-window search where the LDS contrast kernels' hand-unrolled
radius searches have their seams, with the radius every band cell must get stated in closed form beside the numpy model
(radius_ref.search_radius).  Pure numpy; tests/test_window_cases.py holds the fields to the model and the oracle on the CPU,
tests/test_contrast_window_gpu.py runs the kernels on them.

The grid is 160 x 96 (nx x ny): five 32-column strips, six 16-row blocks, five tile columns -- wide enough for the tile
kernel's fast column wrap at an LDS halo of 24 (nx > 82) and of 32 (nx > 98).

Family A, a lone cell of the other class: the background is +-12000 (off the band, all of one class); the interior cells
within Chebyshev distance W = L + 2 of (y0, x0) are band cells of the background's class (+-50); (y0, x0) itself has the
other sign.  L is the largest radius the kernel under test answers from LDS (16, 24, 31, 32).  A patch cell at distance d
gets radius max(1, d): every radius 1 .. L + 2 occurs, at radius r every one of the 8 r border offsets occurs -- the four
corners, where the lone cell enters through ONE entry of a summed-area table, among them -- and the land-side count of the
deciding window is 1 (a land cell in the sea) or area - 1 (a sea cell in land).

Family B, lattices: every cell in the band, the other class at [1::p, 2::p] for odd pitches p -- small radii at every owned
column of a strip and every row of a block.

Rules: `global` (longitude wraps, latitude clamps: a pole row is read with multiplicity), `wrapper` (the f2py rule: column
nx - 1 is never read, column 0 is read in its place; the f2py flavour does not process row ny - 1) and `halo` (a ghost-celled frame, no wrap:
the lone cell may lie in the rim; with a frame narrower than W the patch is cut to the cells whose window stays inside it,
which is what the reference's unbounded search needs and what the kernels' `limited` branch serves)."""
import functools
from dataclasses import dataclass

import numpy as np

import radius_ref
from seabreeze_param_amd import synth

NX, NY = 160, 96
FAR, NEAR = 12000.0, 50.0
MAXDIST = 180.0
LIMITS = (16, 24, 31, 32)
GMMA = -0.0060956

GLOBAL_PLACEMENTS = ((40, 70), (47, 95), (48, 96), (0, 31), (95, 0), (16, 159), (0, 0))
# the wrapper rule never reads column nx - 1: a lone cell there leaves every patch cell without a window
WRAPPER_PLACEMENTS = ((40, 70), (47, 95), (48, 96), (0, 31), (95, 0), (15, 158), (0, 0))
RIM_PLACEMENTS = ((-3, 50), (40, -2), (NY + 2, NX + 1))
NARROW_PLACEMENTS = RIM_PLACEMENTS + ((3, 3),)
PITCHES = (3, 5, 9, 13, 17, 21, 25, 29, 33)
INTERIOR = (40, 70)
SEAM_PLACEMENTS = (INTERIOR, (47, 95), (48, 96))       # the interior, and both sides of a block seam and a strip seam at once

_BND = {"wrapper": radius_ref.BND_WRAPPER, "global": radius_ref.BND_GLOBAL, "halo": radius_ref.BND_HALO}


def narrow_halo(L):
    """The frame narrower than the kernel's limit."""
    return 12 if L == 24 else 7


@dataclass(frozen=True, eq=False)
class Case:
    family: str          # "A" or "B"
    L: int               # largest radius the kernel under test answers from LDS
    W: int               # largest radius in the case by construction (0: a lattice, the model says)
    rule: str            # "global", "wrapper", "halo"
    halo: int            # ghost frame width (0 unless rule == "halo")
    lone_is_land: bool   # the lone cell / the lattice points are land side
    lone: tuple          # (y0, x0) in interior coordinates, or None
    mask: np.ndarray     # (NY + 2 halo, NX + 2 halo) float64: the distance field
    band: np.ndarray     # (NY, NX) bool: cells the call processes
    radius: np.ndarray   # (NY, NX) int32: expected radius, 0 off the band
    closed: bool         # `radius` is the closed form (else the model's: the closed form does not apply)

    @property
    def bnd(self):
        return _BND[self.rule]

    @property
    def max_radius(self):
        return int(self.radius.max())

    def view(self, flavour):
        """(band, radius) as the flavour sees them: the f2py flavour does not process row ny - 1."""
        if flavour != "f2py":
            return self.band, self.radius
        band, radius = self.band.copy(), self.radius.copy()
        band[NY - 1], radius[NY - 1] = False, 0
        return band, radius

    def beyond(self, flavour="generic"):
        """Band cells whose window outgrows the tables of the kernel under test."""
        return int((self.view(flavour)[1] > self.L).sum())


def model_radius(mask, halo, rule, f2py=False):
    """radius_ref.search_radius for a case's field.  The model speaks of the f2py flavour under the wrapper rule, which does
    not process row ny - 1; the host-model signature with that rule does, so the model runs on the field with its last row
    repeated (the latitude clamp reads the same values) and the added row is dropped."""
    if rule == "wrapper" and not f2py:
        return radius_ref.search_radius(np.vstack([mask, mask[-1:]]), MAXDIST, 0, radius_ref.BND_WRAPPER)[:-1]
    return radius_ref.search_radius(mask, MAXDIST, halo, _BND[rule])


def frame_reach(halo):
    """(NY, NX): the largest window radius that stays inside a ghost frame of `halo` cells."""
    x, y = np.arange(NX)[None, :], np.arange(NY)[:, None]
    return np.minimum(np.minimum(x + halo, NX - 1 - x + halo), np.minimum(y + halo, NY - 1 - y + halo))


def lone_cell(L, place, rule, lone_is_land, W=None, halo=0):
    """Family A.  The closed form: radius = max(1, Chebyshev distance to the lone cell), longitude wrapping unless in a frame."""
    W = L + 2 if W is None else W
    y0, x0 = place
    bg = -1.0 if lone_is_land else 1.0
    y, x = np.arange(NY)[:, None], np.arange(NX)[None, :]
    dx = np.abs(x - x0)
    if rule != "halo":
        dx = np.minimum(dx, NX - dx)
    d = np.maximum(np.abs(y - y0), dx)
    patch = d <= (np.minimum(W, frame_reach(halo)) if rule == "halo" else W)
    mask = np.full((NY + 2 * halo, NX + 2 * halo), bg * FAR)
    inner = mask[halo:halo + NY, halo:halo + NX]
    inner[patch] = bg * NEAR
    mask[y0 + halo, x0 + halo] = -bg * NEAR
    band = patch.copy()
    inside = 0 <= y0 < NY and 0 <= x0 < NX
    if inside:
        band[y0, x0] = True
    # under the wrapper rule column 0 is read twice: no closed form for a lone cell there
    closed = not (rule == "wrapper" and x0 == 0)
    radius = np.where(band, np.maximum(d, 1), 0).astype(np.int32) if closed else model_radius(mask, halo, rule)
    return Case("A", L, W, rule, halo, lone_is_land, place, mask, band, radius, closed)


def lattice(L, p, lone_is_land):
    """Family B: the model's radii (no closed form: the pitch divides neither 160 nor 96, and the pole rows repeat)."""
    bg = -1.0 if lone_is_land else 1.0
    mask = np.full((NY, NX), bg * NEAR)
    mask[1::p, 2::p] = -bg * NEAR
    radius = radius_ref.search_radius(mask, MAXDIST, 0, radius_ref.BND_GLOBAL)
    return Case("B", L, 0, "global", 0, lone_is_land, None, mask, np.ones((NY, NX), bool), radius, False)


class Spec(tuple):
    """What builds a case, cheap enough to list at collection time: (family, L, place or pitch, rule, lone_is_land, W, halo)."""
    __slots__ = ()

    @property
    def name(self):
        fam, L, key, rule, land, W, halo = self
        pol = "land-in-sea" if land else "sea-in-land"
        if fam == "B":
            return f"B-p{key}-{pol}"
        return f"A-W{W}-{rule}{halo or ''}-y{key[0]}x{key[1]}-{pol}"


def _a(L, place, rule, land, W=None, halo=0):
    return Spec(("A", L, place, rule, land, L + 2 if W is None else W, halo))


@functools.lru_cache(maxsize=96)
def build(spec):
    fam, L, key, rule, land, W, halo = spec
    return lattice(L, key, land) if fam == "B" else lone_cell(L, key, rule, land, W=W, halo=halo)


def global_specs(L):
    """The cases the coverage assertion speaks of: Family A at the global placements and the lattices, both polarities."""
    out = [_a(L, pl, "global", pol) for pl in GLOBAL_PLACEMENTS for pol in (True, False)]
    out += [Spec(("B", L, p, "global", pol, 0, 0)) for p in PITCHES if (p - 1) // 2 <= L for pol in (True, False)]
    return out


def wrapper_specs(L):
    return [_a(L, pl, "wrapper", pol) for pl in WRAPPER_PLACEMENTS for pol in (True, False)]


def frame_specs(L):
    W = L + 2
    out = [_a(L, pl, "halo", pol, halo=W) for pl in RIM_PLACEMENTS for pol in (True, False)]
    out += [_a(L, pl, "halo", pol, halo=narrow_halo(L)) for pl in NARROW_PLACEMENTS for pol in (True, False)]
    return out


def full_tables_specs(L):
    """W = L: nothing beyond the tables, the largest radius they answer at every border offset."""
    return [_a(L, pl, "global", pol, W=L) for pl in SEAM_PLACEMENTS for pol in (True, False)]


def all_specs(L):
    return global_specs(L) + wrapper_specs(L) + frame_specs(L) + full_tables_specs(L)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def statics(case, dtype=np.float64):
    return synth.static_fields(NX + 2 * case.halo, NY + 2 * case.halo, dtype)


def theta(case, tn, dtype=np.float64):
    """280 + 40 U[0, 1) per cell, a fresh stream every call; 30 K less at the lone cell.  The amplitude makes one border cell
    dropped, or a radius off by one, move thc far beyond any tolerance (test_window_cases.py: the sensitivity condition)."""
    th = 280.0 + 40.0 * synth.hash_uniform(case.mask.shape, 7000 + tn)
    if case.lone is not None:
        th[case.lone[0] + case.halo, case.lone[1] + case.halo] -= 30.0
    return np.ascontiguousarray(th, dtype=dtype)


def core(case, a):
    """The interior of a frame array (last two axes)."""
    h = case.halo
    return np.ascontiguousarray(a[..., h:h + NY, h:h + NX]) if h else a


# ---- coverage ---------------------------------------------------------------------------------------------------------------
def coverage(cases, L):
    """(column of the strip 0..31, radius) and (row of the block 0..15, radius) pairs the cases visit, radii 1 .. L:
    two bool tables, (32, L + 1) and (16, L + 1), column 0 unused."""
    cols, rows = np.zeros((32, L + 1), bool), np.zeros((16, L + 1), bool)
    for c in cases:
        y, x = np.nonzero((c.radius >= 1) & (c.radius <= L))
        r = c.radius[y, x]
        cols[x % 32, r] = True
        rows[y % 16, r] = True
    return cols, rows


# ---- the window means, in numpy --------------------------------------------------------------------------------------------
def t0_of(case, th, st):
    """theta - gmma z sigmoid(sigma), the sigmoid's two scalars from the interior (generic/sea_breeze_diag.f90:166-167, :457-481)."""
    sg = core(case, st.sigma).astype(np.float64)
    sd = 2.0 / np.sqrt(np.mean((sg - sg.mean()) ** 2))
    r = (sg.max() - sg.min()) / 4.0
    return th.astype(np.float64) - GMMA * st.z.astype(np.float64) / (1.0 + np.exp(-sd * (st.sigma.astype(np.float64) - r)))


def window_contrast(case, t0, radius):
    """Land mean minus sea mean (times the cell's own sign) of every band cell's window of `radius` (a plane: per cell), in
    fp64 from summed-area tables over the plane laid out by the rule's index maps.  NaN off the band, where the radius is
    not positive, where the window leaves a frame and where it holds one class."""
    h, bnd = case.halo, case.bnd
    P = int(radius.max()) + 1
    Y = radius_ref.map_y(np.arange(-P, NY + P), NY, h, bnd, None)
    X = radius_ref.map_x(np.arange(-P, NX + P), NX, h, bnd, None)
    ok = (Y >= 0)[:, None] & (X >= 0)[None, :]
    land = case.mask >= 0
    g = lambda a: np.where(ok, a[np.maximum(Y, 0)[:, None], np.maximum(X, 0)[None, :]], 0)
    planes = [g(np.where(land, t0, 0.0)), g(np.where(land, 0.0, t0)), g(land.astype(np.int64)), g((~land).astype(np.int64)),
              (~ok).astype(np.int64)]
    sat = []
    for a in planes:
        s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), a.dtype)
        s[1:, 1:] = a.cumsum(0).cumsum(1)
        sat.append(s)
    y, x = np.nonzero(case.band & (radius > 0))
    r = radius[y, x]
    r0, r1, c0, c1 = y + P - r, y + P + r + 1, x + P - r, x + P + r + 1
    tl, ts, nl, ns, bad = [s[r1, c1] - s[r0, c1] - s[r1, c0] + s[r0, c0] for s in sat]
    own = np.where(land[y + h, x + h], 1.0, -1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = own * (tl / nl - ts / ns)
    v[(bad > 0) | (nl == 0) | (ns == 0)] = np.nan
    out = np.full((NY, NX), np.nan)
    out[y, x] = v
    return out


# ---- a call sequence on a case -------------------------------------------------------------------------------------------------
NZ, STEPS, MARKER = 2, (1, 2, 3), 3.25
TIMESTEP_S = 7200.0          # host-model signature: the third call refreshes the wind direction
TIMESTEP_MIN = 360.0         # f2py flavour: every call refreshes, so the carried state shows each call's winds


def inputs(case, tn, dtype, flavour):
    """(statics, p, u, v, theta) of call tn: z, sigma, winds and pressure from synth as elsewhere, the interior of the frame's."""
    st = statics(case, dtype)
    u, v = (core(case, a) for a in synth.wind_step(st, NZ, tn, dtype))
    p = synth.pressure_1d(NZ, dtype) if flavour == "f2py" else core(case, synth.pressure_3d(st, NZ, dtype))
    return st, p, u, v, theta(case, tn, dtype)


def run_sequence(side, case, flavour, dtype, sdtype=None):
    """Three calls on the case's distance field, fresh theta each, state carried (every state plane starts at MARKER).
    `side`: a hip.Context or an oracle (the same call signatures); flavour "generic" (the host-model signature under the
    case's rule) or "f2py" (the diag call: wrapper rule, t0 plane).  sdtype: the precision the side works in (the fp64
    oracle on fp32-representable inputs).  -> per call: the planes [ws, wd, thc, sb_con] after it (f2py: [ws, wd, thc]
    and the (4, NY, NX) output), and whatever `side.last_nn_max` says (None where the side has none)."""
    sdtype = dtype if sdtype is None else sdtype
    c = lambda a: np.ascontiguousarray(a, dtype=sdtype)
    state = [np.full((NY, NX), MARKER, sdtype) for _ in range(3 if flavour == "f2py" else 4)]
    mask = c(case.mask.astype(dtype))
    calls = []
    for tn in STEPS:
        st, p, u, v, th = inputs(case, tn, dtype, flavour)
        out = None
        if flavour == "f2py":
            out = side.diag(tn, c(p), c(st.z), c(st.sigma), c(th), c(v), c(u), mask, *state, timestep=TIMESTEP_MIN)
        else:
            side.seabreeze_diag(TIMESTEP_S, tn, c(p), c(u), c(v), c(th), mask, c(st.z), c(st.sigma), *state,
                                halo=case.halo, bnd=case.bnd)
        calls.append(dict(state=[a.copy() for a in state], out=None if out is None else out.copy(),
                          nn_max=getattr(side, "last_nn_max", None),
                          counters=side.last_counters() if hasattr(side, "last_counters") else None))
    return calls
