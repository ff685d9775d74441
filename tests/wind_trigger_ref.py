"""Plain numpy restatement of the second half of a diag call -- the pressure-level choice, the wind, the four
thresholds, the scaling and the carried state -- and the directed inputs the tests of k_wind / sb_trigger_update feed
(tests/test_wind_trigger_ref.py on the CPU, tests/test_wind_trigger_gpu.py on the device).

What is restated, each written as the obvious loop or expression in the working precision `dtype`:
  nearest_level   generic/sea_breeze_diag.f90:223          minloc(abs(p - target)): the FIRST of equal minima
  um_walk_level   UM/vn10.7/sea_breeze_diag.F90:265-274    upwards from 1e6 while the difference does not grow
  trigger         generic/sea_breeze_diag.f90:225-266      (f2py=True: seabreeze_diag_python.f90:236-280)
  refresh         generic/sea_breeze_diag.f90:264          fmod(real(tn)*timestep, 21600) < 1e-4

The directed inputs are built so that every intermediate of a threshold comparison is exact in single and in double
precision; the expected outcome at a knife edge then does not depend on rounding:
  contrast   one-column stripes of land and sea written into the distance field as +-50 km, z = 0 (t0 is theta bit for
             bit), theta constant per class inside blocks of rows: an interior row of a block has
             n_thc = +-(L - S) exactly under any summation order (n*L/n is exact for dyadic L of few bits);
  wind       axis-aligned or Pythagorean (u, v): sqrt is exact; the carried state is preset by the test and the call
             runs at tn = 2 between refreshes, so dws, mws and dwd are under per-cell control.
Arrays are C-order numpy, (ny, nx) and (nz, ny, nx), as everywhere in the tests.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

RAD2DEG = 57.2957                 # generic/sea_breeze_diag.f90:128 (sic: truncated)
TARGET_PLEV = 70000.0
THRESHOLDS = dict(thresh_wind=11.0, thresh_winddir=90.0, thresh_windch=5.0, thresh_thc=0.75)
PERIOD_S = 21600.0


def _t(dtype):
    return np.dtype(dtype).type


# ----------------------------------------------------------------------------------------------------------------
# pressure level
# ----------------------------------------------------------------------------------------------------------------
def nearest_level(p, target, dtype):
    """First index of the minimum of |p - target| down each column (axis 0), arithmetic in dtype."""
    p = np.asarray(p, dtype=dtype)
    return np.argmin(np.abs(p - _t(dtype)(target)), axis=0)          # argmin: the first of equal minima


def um_walk_level(p, target, dtype):
    """The UM copy's walk, column by column.  Returns (level, defined): where even the first level is further than
    1e6 from the target the UM leaves p_lev undefined (level 0 is reported, defined = False)."""
    dt = _t(dtype)
    p = np.asarray(p, dtype=dtype)
    nz = p.shape[0]
    cols = p.reshape(nz, -1)
    lev = np.zeros(cols.shape[1], np.int64)
    defined = np.zeros(cols.shape[1], bool)
    for c in range(cols.shape[1]):
        diff = dt(1000000.0)
        for k in range(nz):
            a = abs(dt(cols[k, c] - dt(target)))
            if a <= diff:
                lev[c] = k
                diff = a
                defined[c] = True
            else:
                break
    return lev.reshape(p.shape[1:]), defined.reshape(p.shape[1:])


# ----------------------------------------------------------------------------------------------------------------
# thresholds, scaling, carried state
# ----------------------------------------------------------------------------------------------------------------
def fortran_modulo(a, p):
    """MODULO(a, p) for reals, p > 0: fmod (exact), folded into [0, p)."""
    r = np.fmod(a, p)
    return np.where(r < 0, r + p, r).astype(a.dtype)


Trig = namedtuple("Trig", "sb_con ws wd dws mws dwd n_ws n_wd")


def trigger(dtype, tn, refresh_now, n_thc, ws_old, wd_old, u, v, thresholds=None, f2py=False):
    """Cell by cell, u and v taken at the chosen level already.  Returns sb_con, the state (ws, wd) after the call and
    the intermediates.  f2py=False: the host-model rule (ws every call, wd when refreshing); f2py=True: the Python
    surface's rule (ws and wd when refreshing only) -- its output planes 3 and 4 are this state."""
    dt = _t(dtype)
    th = dict(THRESHOLDS)
    th.update(thresholds or {})
    thr_wind, thr_dir = dt(th["thresh_wind"]), dt(th["thresh_winddir"])
    thr_ch, thr_thc = dt(th["thresh_windch"]), dt(th["thresh_thc"])
    n_thc = np.asarray(n_thc, dtype=dtype)
    u = np.asarray(u, dtype=dtype)
    v = np.asarray(v, dtype=dtype)
    ws = np.array(ws_old, dtype=dtype)
    wd = np.array(wd_old, dtype=dtype)
    n_ws = np.sqrt(u * u + v * v)
    n_wd = (np.arctan2(dt(-1) * u, dt(-1) * v) * dt(RAD2DEG)).astype(dtype)
    if tn < 2:
        ws, wd = n_ws.copy(), n_wd.copy()
    thc_abs = np.abs(n_thc)
    mws = (ws + n_ws) / dt(2)
    dws = np.abs(ws - n_ws)
    dwd = np.abs(fortran_modulo((wd - n_wd) + dt(180), dt(360)) - dt(180))
    fire = (dwd < thr_dir) & (dws < thr_ch) & (mws < thr_wind) & (thc_abs > thr_thc)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale_wind = (thr_wind - mws) / np.maximum(dt(1), mws)
        scale_thc = (thc_abs - thr_thc) / n_thc
        sb = np.where(fire, scale_thc * scale_wind, dt(0)).astype(dtype)
    if f2py:
        if refresh_now:
            ws, wd = n_ws.copy(), n_wd.copy()
    else:
        ws = n_ws.copy()
        if refresh_now:
            wd = n_wd.copy()
    return Trig(sb, ws, wd, dws, mws, dwd, n_ws, n_wd)


def refresh(dtype, tn, timestep, period=PERIOD_S):
    """Host-model flavour: timestep in seconds."""
    dt = _t(dtype)
    return bool(np.fmod(dt(tn) * dt(timestep), dt(period)) < dt(1e-4))


def refresh_f2py(dtype, tn, timestep_min, target_time_h=6.0):
    """Python surface: timestep in minutes, target_time in hours, converted in dtype (:146-148)."""
    dt = _t(dtype)
    return bool(np.fmod(dt(tn) * (dt(timestep_min) * dt(60)), dt(target_time_h) * dt(3600)) < dt(1e-4))


# (timestep s, tn): exact products, a product that rounds differently in the two precisions, one that always
# refreshes, and three whose product falls just below a multiple of 21600 in both precisions (found on the CPU,
# asserted in test_wind_trigger_ref.py)
REFRESH_PAIRS = [(1800.0, 12), (1800.0, 11), (7200.0, 3), (21600.0 / 7.0, 7), (0.1, 216000), (1e-5, 1),
                 (0.3, 216000), (0.7, 30857), (2699.99, 8), (0.07, 1542857)]


# ----------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------
SEA_T = 288.0
EPS = 2.0 ** -10
CONTRASTS = {            # name -> L - S of the block (K)
    "edge": 0.75,                    # |thc| == thresh_thc: never fires
    "above": 0.75 + EPS,             # fires
    "neg": -(0.75 + EPS),            # fires; on land n_thc < 0: scale_thc and sb_con negative
    "half": 0.5,
}
BLOCKS = ("edge", "above", "neg", "half")          # south to north

Case = namedtuple("Case", "name ws_old wd_old u v contrast fires")
# `fires` is written by hand from the rule (strict <, <, <, >), never computed.  n_wd of the winds used:
#   u = 0, v < 0 -> atan2(-0, +) = -0 deg;   u = 0, v > 0 -> atan2(-0, -) = -pi -> -179.99975 deg;
#   u = -0.0, v > 0 -> atan2(+0, -) = +pi -> +179.99975 deg;   u < 0, v = 0 -> atan2(+, -0) = pi/2 -> 89.99988 deg.
# The wrap rows reach +-179.99975 instead of +-179.9, which no axis-aligned wind gives; their dwd is about 0.1 deg.
CASES = [
    #    name               ws_old  wd_old     u     v    contrast fires
    Case("all_pass",          4.0,    0.0,   0.0, -4.0,   "above", True),
    Case("dws_at_5",          8.0,    0.0,   0.0, -3.0,   "above", False),    # dws = 5, mws = 5.5
    Case("dws_4.75",          7.75,   0.0,   0.0, -3.0,   "above", True),
    Case("dws_at_5_pyth",    10.0, -143.0,   3.0,  4.0,   "above", False),    # n_ws = 5 (3-4-5), n_wd = -143.13
    Case("dws_4.75_pyth",     9.75, -143.0,  3.0,  4.0,   "above", True),
    Case("mws_at_11",        12.0,    0.0,   0.0, -10.0,  "above", False),    # mws = 11, dws = 2
    Case("mws_10.75",        11.5,    0.0,   0.0, -10.0,  "above", True),
    Case("mws_below_1",       0.5,    0.0,   0.0, -0.5,   "above", True),     # divisor max(1, 0.5) = 1
    Case("calm_opposed",      0.0,    0.0,   0.0,  0.0,   "above", False),    # n_wd = -179.99975: dwd = 179.99975
    Case("calm_aligned",      0.0, -179.0,   0.0,  0.0,   "above", True),     # dwd = 0.99975, divisor 1
    Case("turn_exact_90",     4.0,    0.0,  -4.0,  0.0,   "above", True),     # dwd = 89.99988 < 90 (rad2deg sic)
    Case("turn_90_state",     4.0,   90.0,   0.0, -4.0,   "above", False),    # dwd = 90 exactly, from the carried state
    Case("turn_-90_state",    4.0,  -90.0,   0.0, -4.0,   "above", False),
    Case("turn_91",           4.0,   91.0,   0.0, -4.0,   "above", False),
    Case("turn_89",           4.0,   89.0,   0.0, -4.0,   "above", True),
    Case("turn_-91",          4.0,  -91.0,   0.0, -4.0,   "above", False),
    Case("turn_-89",          4.0,  -89.0,   0.0, -4.0,   "above", True),
    Case("wrap_forward",      4.0,  179.9,   0.0,  4.0,   "above", True),     # a = 539.9: 360 <= a < 720
    Case("wrap_reverse",      4.0, -179.9,  -0.0,  4.0,   "above", True),     # a = -179.9: negative a
    Case("wrap_ge_360_near",  4.0,  170.0,   0.0,  4.0,   "above", True),     # wd_old - n_wd = 350: dwd = 10.00025
    Case("wrap_ge_360_far",   4.0,   80.0,   0.0,  4.0,   "above", False),    # wd_old - n_wd = 260: dwd = 100.00025
    Case("state_past_720",    4.0,  725.0,   0.0, -4.0,   "above", True),     # a = 905: the fmod branch, dwd = 5
    Case("state_past_-720",   4.0, -725.0,   0.0, -4.0,   "above", True),     # a = -545: fmod and fold, dwd = 5
    Case("edge_all_pass",     4.0,    0.0,   0.0, -4.0,   "edge",  False),    # only thc fails: |thc| == 0.75
    Case("edge_mws_10.75",   11.5,    0.0,   0.0, -10.0,  "edge",  False),
    Case("neg_all_pass",      4.0,    0.0,   0.0, -4.0,   "neg",   True),
    Case("neg_mws_below_1",   0.5,    0.0,   0.0, -0.5,   "neg",   True),
    Case("neg_dws_at_5",      8.0,    0.0,   0.0, -3.0,   "neg",   False),
    Case("half_all_pass",     4.0,    0.0,   0.0, -4.0,   "half",  False),
    Case("half_turn_91",      4.0,   91.0,   0.0, -4.0,   "half",  False),
]
# non-default thresholds for the runs that check that the kernel reads them from the job: the first puts the knife
# edge of the contrast on the "half" block and tightens the three wind rules, the second loosens all four
TUNABLE_SETS = [dict(thresh_wind=8.0, thresh_winddir=45.0, thresh_windch=2.0, thresh_thc=0.5),
                dict(thresh_wind=12.0, thresh_winddir=100.0, thresh_windch=6.0, thresh_thc=0.25)]

# rows between two blocks hold a wind that fails every wind rule: their contrast mixes two blocks and is not exact
BORDER = Case("border", 30.0, 0.0, 0.0, -30.0, None, False)

_ROWS = max(sum(1 for c in CASES if c.contrast == b) for b in BLOCKS)      # interior rows of a block
MARGIN = 2                                   # border rows on either side of a block's interior rows
BLOCK_H = _ROWS + 2 * MARGIN

TriggerGrid = namedtuple("TriggerGrid", "nx ny nz p u v theta mask z sigma ws_old wd_old case_id directed n_thc land")


def trigger_grid(nx, dtype):
    """The table tiled over an (ny, nx) grid, nx even.  Block b covers rows [b*BLOCK_H, (b+1)*BLOCK_H); on its interior
    row r (0-based inside the block) column c holds the block's case number (c + r) mod n_b, so every case of a block
    meets every column -- every lane of every 64-cell segment, whole or ragged -- and both classes.  case_id indexes
    CASES (-1: border row); n_thc is the exact contrast of a directed cell, sign included.  Two border rows on either
    side keep a window of radius 2 inside the block: the Python surface's longitude rule (max(1, modulo(jj, nlons)),
    seabreeze_diag_python.f90:202) never reads the last column from a neighbour, so the cells of that column find
    their sea only at radius 2."""
    assert nx % 2 == 0
    dt = _t(dtype)
    ny, nz = BLOCK_H * len(BLOCKS), 2
    land = (np.arange(nx) % 2 == 0)[None, :].repeat(ny, 0)
    mask = np.where(land, 50.0, -50.0).astype(dtype)
    theta = np.empty((ny, nx), dtype)
    case_id = np.full((ny, nx), -1, np.int64)
    n_thc = np.zeros((ny, nx), dtype)
    for b, name in enumerate(BLOCKS):
        rows = slice(b * BLOCK_H, (b + 1) * BLOCK_H)
        d = CONTRASTS[name]
        theta[rows] = np.where(land[rows], dt(SEA_T + d), dt(SEA_T))
        assert float(dt(SEA_T + d)) == SEA_T + d                       # dyadic: exact in dtype
        ids = [i for i, c in enumerate(CASES) if c.contrast == name]
        for r in range(_ROWS):
            y = b * BLOCK_H + MARGIN + r
            case_id[y] = [ids[(c + r) % len(ids)] for c in range(nx)]
            n_thc[y] = np.where(land[y], dt(d), dt(-d))
    directed = case_id >= 0
    pick = lambda f: np.array([getattr(CASES[i] if i >= 0 else BORDER, f) for i in case_id.ravel()],
                              dtype=dtype).reshape(ny, nx)
    u = np.empty((nz, ny, nx), dtype)
    v = np.empty((nz, ny, nx), dtype)
    u[0], v[0] = pick("u"), pick("v")
    u[1], v[1] = dt(99.0), dt(-99.0)                                   # the wrong level: nothing passes with it
    p = np.empty((nz, ny, nx), dtype)
    p[0], p[1] = dt(70250.0), dt(50000.0)
    z = np.zeros((ny, nx), dtype)
    sigma = (np.arange(ny * nx).reshape(ny, nx) % 7).astype(dtype)       # any spread: z = 0 switches it off
    return TriggerGrid(nx, ny, nz, p, u, v, theta, mask, z, sigma, pick("ws_old"), pick("wd_old"), case_id,
                       directed, n_thc, land)


def expected_fires(tg):
    """The hand-written column, cell by cell (border rows: False)."""
    f = np.array([c.fires for c in CASES] + [False])
    return f[tg.case_id]


# ----------------------------------------------------------------------------------------------------------------
# pressure columns for the level tests.  Values are 70000 +- multiples of 250 Pa: exact in single precision.
# UNS: SB_WIND_UN (double) and SB_WIND_UN_F32 (single) of seabreeze_param_amd/csrc/sb_launch.hpp -- the batch sizes of
# k_wind's column walk; NZ_LIST covers one level, one below / at / above a batch and ragged second and third batches
# for both.  Revisit both if those constants change.
# ----------------------------------------------------------------------------------------------------------------
UNS = (8, 14)
NZ_LIST = (1, 7, 8, 9, 13, 14, 15, 17, 29)
STEP = 250.0


def _col(d, sign=None):
    d = np.asarray(d, dtype=np.float64)
    s = np.where(np.arange(d.size) % 2 == 0, 1.0, -1.0) if sign is None else np.asarray(sign, dtype=np.float64)
    return TARGET_PLEV + STEP * d * s


def generic_columns(nz):
    """[(name, column(nz), expected level written by hand)] for the first-minimum rule."""
    k = np.arange(nz)
    last = nz - 1
    out = [("min_at_0", _col(k), 0),
           ("min_at_last", _col(last - k + 1), last),
           ("constant", _col(np.full(nz, 3)), 0)]
    for un in UNS:
        a, b = min(un - 1, last), min(un, last)
        out.append((f"min_at_UN-1[{un}]", _col(np.abs(k - a) + 1), a))
        out.append((f"min_at_UN[{un}]", _col(np.abs(k - b) + 1), b))
        # equal minima on both sides of the batch boundary (or at the last two levels): the first wins
        a2 = a if b > a else max(a - 1, 0)
        out.append((f"tie_UN-1_UN[{un}]", _col(np.minimum(np.abs(k - a2), np.abs(k - b)) + 1, np.ones(nz)), a2))
        # the target midway between two adjacent levels (70250 above, 69750 below it): a tie of opposite signs
        sgn = np.where(k <= a2, 1.0, -1.0)
        out.append((f"midway[{un}]", _col(2 * np.minimum(np.abs(k - a2), np.abs(k - b)) + 1, sgn), a2))
        # two local minima, the later one global (in the last batch where there is more than one)
        lo, hi = min(2, last), max(min(un + 2, last), 0)
        d = np.minimum(np.abs(k - lo) + 2, np.abs(k - hi) + 1)
        out.append((f"two_minima[{un}]", _col(d), hi))
    return out


def um_columns(nz):
    """[(name, column(nz), expected level written by hand, defined)] for the UM walk."""
    k = np.arange(nz)
    last = nz - 1
    out = [("never_stops", _col(last - k + 1), last, True),                       # the padded re-read must not matter
           ("constant", _col(np.full(nz, 3)), last, True),                        # ties move on, to the top
           ("beyond_1e6", _col(np.full(nz, 6000) - k), 0, False)]                  # 1.5e6 Pa away: undefined in the UM
    # stops at a local minimum below a later global one
    s = min(2, last)
    d = np.abs(k - s) + 3
    if last >= s + 2:
        d[last] = 0
    out.append(("local_then_global", _col(d), s, True))
    # a plateau of equal differences: the last of the run
    d = np.where(k < 1, 5, np.where(k <= 3, 4, 5 + k))
    out.append(("plateau", _col(d, np.ones(nz)), min(3, last), True))
    for un in UNS:
        a, b = min(un - 1, last), min(un, last)
        d = np.abs(k - a) + 3
        d[k > a + 1] = 0                                                       # nearer levels in the next batch
        out.append((f"stops_at_UN-1[{un}]", _col(d), a, True))
        d = np.abs(k - b) + 3
        d[k > b + 1] = 0
        out.append((f"stops_at_UN[{un}]", _col(d), b, True))
        # a plateau across the batch boundary
        d = np.where(k < a, 9 + a - k, np.where(k <= b, 4, 5 + k))
        out.append((f"plateau_UN-1_UN[{un}]", _col(d, np.ones(nz)), b, True))
    return out


def level_grid(columns, nx, ny, dtype):
    """The columns cycled along longitude, shifted by one per row: p (nz, ny, nx), the pattern number of every cell,
    u = 0 and v[k] = -(k+1)/4, so that ws after a tn = 1 call is (level+1)/4 exactly."""
    nz = columns[0][1].size
    pat = (np.arange(nx)[None, :] + np.arange(ny)[:, None]) % len(columns)
    cols = np.stack([c[1] for c in columns], axis=1)                            # (nz, npat)
    p = np.ascontiguousarray(cols[:, pat], dtype=dtype)
    assert np.array_equal(p.astype(np.float64), cols[:, pat])                  # exact in dtype
    u = np.zeros((nz, ny, nx), dtype)
    v = np.ascontiguousarray(np.broadcast_to((-(np.arange(nz) + 1) / 4.0)[:, None, None], (nz, ny, nx)), dtype=dtype)
    return p, u, v, pat


def striped_mask(nx, ny, dtype):
    return np.where(np.arange(nx) % 2 == 0, 50.0, -50.0).astype(dtype)[None, :].repeat(ny, 0)
