"""Directed tests of the second half of a diag call on the device: k_wind's pressure-level choice (first minimum and UM
walk, across the batches of its column walk), the four thresholds at their knife edges, the scaling, the carried state,
the six-hourly refresh rule evaluated on the host, and the contrast kernels on negative and far-off-range temperatures.

The inputs and the plain reference are those of tests/wind_trigger_ref.py; tests/test_wind_trigger_ref.py proves on the
CPU that the hand-written expectations, the reference functions and the oracle agree on them.  No band cell is masked:
the knife-edge cells are exact by construction in both precisions.  Two exclusions, both counted and printed: columns
of the UM walk whose first level lies more than 1e6 Pa from the target (the UM leaves the level undefined) and refresh
pairs on which the oracle's MODULO and numpy's fmod disagree (none on the build this was written on).

Tolerances are the project's: double precision by test_parity_gpu._assert_close64 (1e-7 relative, 1e-9 absolute floor);
single precision 2e-6 relative for the winds, 2e-3 K for thc, 5e-3 for sb_con.
"""
import contextlib
import functools

import numpy as np
import pytest

import wind_trigger_ref as wr
from conftest import relerr
from seabreeze_param_amd import hip, synth
from test_parity_gpu import _assert_close64

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
# (oracle precision, dtype, radius hint): the strip kernel (<= 16), the tile kernel (17..24, double), k_strip32 (single)
VARIANTS = [(8, F64, 16), (8, F64, 24), (4, F32, 16), (4, F32, 30)]
VARIANT_IDS = ["f64-strip", "f64-tiles24", "f32-strip", "f32-strip32"]
PRECS = [(8, F64), (4, F32)]
TS_S, TS_MIN, TN = 1800.0, 30.0, 2           # tn = 2, 3600 s: between refreshes in both flavours


@contextlib.contextmanager
def _hint(hipctx, r):
    hipctx.set_search_radius_hint(r)
    try:
        yield
    finally:
        hipctx.set_search_radius_hint(16)


def _close(a, b, dt, what, kind):
    """kind: 'ws' | 'wd' | 'thc' | 'sb_con'."""
    if dt == F64:
        _assert_close64(a, b, what)
    elif kind in ("ws", "wd"):
        e = relerr(a, b, floor=1e-3 if kind == "ws" else 1e-1)
        assert e < 2e-6, f"{what}: rel err {e}"
    else:
        e = float(np.max(np.abs(a.astype(F64) - b.astype(F64))))
        assert e < (2e-3 if kind == "thc" else 5e-3), f"{what}: abs err {e}"


@functools.lru_cache(maxsize=None)
def _grid(nx, dt):
    return wr.trigger_grid(nx, dt)


# ----------------------------------------------------------------------------------------
# a. the trigger table
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [130, 192])
@pytest.mark.parametrize("prec,dt,hint", VARIANTS, ids=VARIANT_IDS)
def test_trigger_table_generic(hipctx, oracles, prec, dt, hint, nx):
    """Every row of the table on lanes 0 and 63, in the first, the last and (nx = 130) a ragged 64-cell segment, on land
    and on sea: the fire pattern is the hand-written column and the oracle's, thc is +-(L - S) to the bit."""
    tg = _grid(nx, dt)
    so = [tg.ws_old.copy(), tg.wd_old.copy(), np.full_like(tg.z, -5.0), np.full_like(tg.z, np.nan)]
    sh = [a.copy() for a in so]
    oracles[prec].seabreeze_diag(TS_S, TN, tg.p, tg.u, tg.v, tg.theta, tg.mask, tg.z, tg.sigma, *so, halo=0, bnd=1)
    with _hint(hipctx, hint):
        hipctx.seabreeze_diag(TS_S, TN, tg.p, tg.u, tg.v, tg.theta, tg.mask, tg.z, tg.sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
    d = tg.directed
    bad = np.argwhere(d & (sh[2] != tg.n_thc))
    print(f"thc: {len(bad)} directed cells differ from +-(L - S); first: "
          f"{[(int(y), int(x), float(sh[2][y, x]).hex(), float(tg.n_thc[y, x]).hex()) for y, x in bad[:3]]}")
    fired = sh[3] != 0
    wrong = np.argwhere(fired != wr.expected_fires(tg))
    print("fire pattern: cells that differ from the table:",
          sorted({wr.CASES[tg.case_id[y, x]].name if tg.case_id[y, x] >= 0 else "border" for y, x in wrong}))
    assert len(bad) == 0
    assert len(wrong) == 0
    assert np.array_equal(fired, so[3] != 0)
    for a, b, nm in zip(sh, so, ("ws", "wd", "thc", "sb_con")):
        _close(a, b, dt, f"table nx={nx} {nm}", nm)
    ref = wr.trigger(dt, TN, False, tg.n_thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0])
    _close(sh[3][d], ref.sb_con[d], dt, "sb_con against the plain reference", "sb_con")
    assert np.array_equal(sh[0], ref.ws) and np.array_equal(sh[1], tg.wd_old)        # exact winds, carried direction


@pytest.mark.parametrize("prec,dt,hint", VARIANTS, ids=VARIANT_IDS)
def test_trigger_table_f2py(hipctx, oracles, prec, dt, hint):
    """The Python surface on the same cells: the trigger plane follows the table, the state and the ws / wd planes keep
    the preset values between refreshes (seabreeze_diag_python.f90:268-280), t0 is theta (z = 0)."""
    tg = _grid(130, dt)
    p1 = tg.p[:, 0, 0].copy()
    so = [tg.ws_old.copy(), tg.wd_old.copy(), np.full_like(tg.z, -5.0)]
    sh = [a.copy() for a in so]
    oo = oracles[prec].diag(TN, p1, tg.z, tg.sigma, tg.theta, tg.v, tg.u, tg.mask, *so, timestep=TS_MIN)
    with _hint(hipctx, hint):
        oh = hipctx.diag(TN, p1, tg.z, tg.sigma, tg.theta, tg.v, tg.u, tg.mask, *sh, timestep=TS_MIN)
    d = tg.directed[:-1]
    assert np.array_equal(sh[2][:-1][d], tg.n_thc[:-1][d])
    assert np.array_equal(oh[0, :-1] != 0, wr.expected_fires(tg)[:-1])
    assert np.array_equal(oh[0, :-1] != 0, oo[0, :-1] != 0)
    for k, nm in enumerate(("sb_con", "ws", "ws", "wd")):
        _close(oh[k, :-1], oo[k, :-1], dt, f"f2py table plane {k}", nm)
    _close(sh[2], so[2], dt, "f2py table thc", "thc")
    assert np.array_equal(oh[1, :-1], tg.theta[:-1])
    for plane, state, preset in ((oh[2], sh[0], tg.ws_old), (oh[3], sh[1], tg.wd_old)):
        assert np.array_equal(plane[:-1], preset[:-1]) and np.array_equal(state, preset)


@pytest.mark.parametrize("th", wr.TUNABLE_SETS, ids=["tight", "loose"])
@pytest.mark.parametrize("prec,dt", PRECS, ids=["f64", "f32"])
def test_trigger_table_non_default_thresholds(hipctx, oracles, prec, dt, th):
    """The kernel reads the four thresholds from the job: the table under other values, against the plain reference
    with the same values (host-model flavour) and against the oracle, which takes them as arguments (Python surface)."""
    tg = _grid(130, dt)
    tun = hip.Tunables(target_plev_pa=70000.0, target_time_s=21600.0, maxdist_km=180.0, **th)
    sh = [tg.ws_old.copy(), tg.wd_old.copy(), np.full_like(tg.z, -5.0), np.full_like(tg.z, np.nan)]
    hipctx.seabreeze_diag(TS_S, TN, tg.p, tg.u, tg.v, tg.theta, tg.mask, tg.z, tg.sigma, *sh, halo=0,
                          bnd=hip.SB_BND_GLOBAL, tunables=tun)
    ref = wr.trigger(dt, TN, False, tg.n_thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0], th)
    dflt = wr.trigger(dt, TN, False, tg.n_thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0])
    assert not np.array_equal(ref.sb_con != 0, dflt.sb_con != 0)
    assert np.array_equal(sh[3] != 0, ref.sb_con != 0)               # (border rows: n_thc = 0 here, and no wind rule passes)
    _close(sh[3][tg.directed], ref.sb_con[tg.directed], dt, "sb_con under other thresholds", "sb_con")
    p1 = tg.p[:, 0, 0].copy()
    so3 = [tg.ws_old.copy(), tg.wd_old.copy(), np.full_like(tg.z, -5.0)]
    sh3 = [a.copy() for a in so3]
    oo = oracles[prec].diag(TN, p1, tg.z, tg.sigma, tg.theta, tg.v, tg.u, tg.mask, *so3, timestep=TS_MIN, **th)
    oh = hipctx.diag(TN, p1, tg.z, tg.sigma, tg.theta, tg.v, tg.u, tg.mask, *sh3, timestep=TS_MIN, **th)
    assert np.array_equal(oh[0, :-1] != 0, oo[0, :-1] != 0) and np.array_equal(oh[0, :-1] != 0, (ref.sb_con != 0)[:-1])
    _close(oh[0, :-1], oo[0, :-1], dt, "f2py sb_con under other thresholds", "sb_con")


# ----------------------------------------------------------------------------------------
# b. level choice, first-minimum rule.  wr.NZ_LIST is built around SB_WIND_UN = 8 and SB_WIND_UN_F32 = 14
# (seabreeze_param_amd/csrc/sb_launch.hpp), the levels k_wind holds in flight per batch: revisit wr.UNS and the list if
# they change.
# ----------------------------------------------------------------------------------------
def _level_fields(nx, ny, dt):
    mask = wr.striped_mask(nx, ny, dt)
    theta = np.where(mask > 0, 289.0, 288.0).astype(dt)
    return mask, theta, np.zeros((ny, nx), dt), (np.arange(ny * nx).reshape(ny, nx) % 5).astype(dt)


@pytest.mark.parametrize("nz", wr.NZ_LIST)
@pytest.mark.parametrize("prec,dt", PRECS, ids=["f64", "f32"])
def test_level_choice_generic(hipctx, oracles, prec, dt, nz):
    nx, ny = 130, 3
    mask, theta, z, sigma = _level_fields(nx, ny, dt)
    columns = wr.generic_columns(nz)
    p, u, v, pat = wr.level_grid(columns, nx, ny, dt)
    lev = wr.nearest_level(p, wr.TARGET_PLEV, dt)
    assert np.array_equal(lev, np.array([c[2] for c in columns])[pat])
    so, sh = ([np.zeros((ny, nx), dt) for _ in range(4)] for _ in range(2))
    oracles[prec].seabreeze_diag(TS_S, 1, p, u, v, theta, mask, z, sigma, *so, halo=0, bnd=1)
    hipctx.seabreeze_diag(TS_S, 1, p, u, v, theta, mask, z, sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
    got = sh[0] * 4 - 1
    wrong = sorted({columns[i][0] for i in pat[got != lev]})
    print(f"nz={nz}: patterns with a wrong level: {wrong}")
    assert np.array_equal(got, lev.astype(dt)), wrong
    assert np.array_equal(sh[0], so[0])


@pytest.mark.parametrize("nz", wr.NZ_LIST)
@pytest.mark.parametrize("prec,dt", PRECS, ids=["f64", "f32"])
def test_level_choice_f2py_1d(hipctx, oracles, prec, dt, nz):
    """The Python surface's 1-D p, each pattern in a call of its own.  One level serves the whole grid; the host-pointer
    entry point picks it on the host (pick_level in sb_ctx.hpp, the same strict first-minimum loop) and uploads that
    level's u / v planes only, so this pins the host loop; k_wind's own 1-D loop runs only for device-pointer callers
    with more than one level, which the Python binding does not expose."""
    nx, ny = 66, 3
    mask, theta, z, sigma = _level_fields(nx, ny, dt)
    u = np.zeros((nz, ny, nx), dt)
    v = np.ascontiguousarray(np.broadcast_to((-(np.arange(nz) + 1) / 4.0)[:, None, None], (nz, ny, nx)), dtype=dt)
    for name, col, hand in wr.generic_columns(nz):
        p1 = col.astype(dt)
        assert int(wr.nearest_level(p1, wr.TARGET_PLEV, dt)) == hand
        so, sh = ([np.zeros((ny, nx), dt) for _ in range(3)] for _ in range(2))
        oo = oracles[prec].diag(1, p1, z, sigma, theta, v, u, mask, *so, target_plev=700.0)
        oh = hipctx.diag(1, p1, z, sigma, theta, v, u, mask, *sh, target_plev=700.0)
        assert np.all(oh[2, :-1] * 4 - 1 == hand), (name, float(oh[2, 0, 0]) * 4 - 1, hand)
        assert np.array_equal(oh[2, :-1], oo[2, :-1]), name


# ----------------------------------------------------------------------------------------
# c. level choice, UM walk
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", wr.NZ_LIST)
@pytest.mark.parametrize("prec,dt", PRECS, ids=["f64", "f32"])
def test_level_choice_um_walk(hipctx, oracles, prec, dt, nz):
    """seabreeze_diag_um with SB_UM_LEVEL_WALK (UM layout: small halo 2, large halo 5): the walk stops at the first
    increase, moves on over ties, keeps `done` from one batch of levels to the next and is not disturbed by the padded
    re-read of the last level."""
    nx, ny, hs, hl = 130, 3, 2, 5
    mask_l, _, _, _ = _level_fields(nx + 2 * hl, ny + 2 * hl, dt)
    inner = lambda a, h: np.ascontiguousarray(a[hl - h:a.shape[0] - (hl - h), hl - h:a.shape[1] - (hl - h)])
    mask_s = inner(mask_l, hs)
    theta_s = np.where(mask_s > 0, 289.0, 288.0).astype(dt)
    z_s = np.zeros_like(theta_s)
    sg_s = (np.arange(theta_s.size).reshape(theta_s.shape) % 5).astype(dt)
    columns = wr.um_columns(nz)
    p, u, v, pat = wr.level_grid(columns, nx, ny, dt)
    lev, defined = wr.um_walk_level(p, wr.TARGET_PLEV, dt)
    assert np.array_equal(lev[defined], np.array([c[2] for c in columns])[pat][defined])
    so, sh = ([np.zeros((ny, nx), dt) for _ in range(4)] for _ in range(2))
    oracles[prec].seabreeze_diag(TS_S, 1, p, u, v, theta_s, mask_s, z_s, sg_s, *so, halo=hs, bnd=2, level_rule=1)
    err = hipctx.seabreeze_diag_um(TS_S, 1, p, u, v, theta_s.copy(), z_s, sg_s, mask_l, *sh, halo_s=hs, halo_l=hl,
                                   flags=hip.SB_UM_LEVEL_WALK)
    assert err == 0
    print(f"nz={nz}: {int((~defined).sum())} of {defined.size} columns left out (first level beyond 1e6 Pa)")
    assert (~defined).sum() == (pat == [c[0] for c in columns].index("beyond_1e6")).sum()
    got = sh[0] * 4 - 1
    wrong = sorted({columns[i][0] for i in pat[defined & (got != lev)]})
    print(f"nz={nz}: patterns with a wrong level: {wrong}")
    assert np.array_equal(got[defined], lev[defined].astype(dt)), wrong
    assert np.array_equal(sh[0][defined], so[0][defined])


# ----------------------------------------------------------------------------------------
# d. the six-hourly refresh rule
# ----------------------------------------------------------------------------------------
# (1e-5, 1) cannot tell the outcomes apart (at tn = 1 the state takes this call's winds anyway): later steps of that
# timestep are added
PAIRS = wr.REFRESH_PAIRS + [(1e-5, 2), (1e-5, 7)]


@pytest.mark.parametrize("prec,dt", PRECS, ids=["f64", "f32"])
def test_refresh_rule(hipctx, oracles, prec, dt):
    """modulo(real(tn)*timestep, 21600) < 1e-4 in the working precision, on the host: wd (host-model flavour), ws and
    wd (Python surface) take this call's values exactly when it holds.  This call's winds (4 m/s, -0 deg) differ from
    the preset state (1, 1)."""
    nx, ny = 66, 4
    mask, theta, z, sigma = _level_fields(nx, ny, dt)
    p = np.full((1, ny, nx), 70000.0, dt)
    u = np.zeros((1, ny, nx), dt)
    v = np.full((1, ny, nx), -4.0, dt)
    one = lambda n: [np.full((ny, nx), 1.0, dt) for _ in range(n)]
    dropped, seen = 0, set()
    for ts, tn in PAIRS:
        so = one(4)
        oracles[prec].seabreeze_diag(ts, tn, p, u, v, theta, mask, z, sigma, *so, halo=0, bnd=1)
        want = wr.refresh(dt, tn, ts)
        if bool(so[1][0, 0] != 1.0) != want:
            dropped += 1                                        # the oracle's MODULO and numpy's fmod disagree
            continue
        sh = one(4)
        hipctx.seabreeze_diag(ts, tn, p, u, v, theta, mask, z, sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
        assert np.all(sh[0] == 4.0), (ts, tn)                 # ws: every call
        assert np.all(sh[1] == (0.0 if want or tn < 2 else 1.0)), (ts, tn, want, float(sh[1][0, 0]))
        assert np.array_equal(sh[1], so[1])
        seen.add(want)
        # Python surface: minutes and hours
        want3 = wr.refresh_f2py(dt, tn, ts / 60.0)
        so3 = one(3)
        oo = oracles[prec].diag(tn, p[:, 0, 0].copy(), z, sigma, theta, v, u, mask, *so3, timestep=ts / 60.0)
        if bool(so3[0][0, 0] != 1.0) != (want3 or tn < 2):
            dropped += 1
            continue
        sh3 = one(3)
        oh = hipctx.diag(tn, p[:, 0, 0].copy(), z, sigma, theta, v, u, mask, *sh3, timestep=ts / 60.0)
        new = want3 or tn < 2
        for plane, state, (fresh, kept) in ((oh[2], sh3[0], (4.0, 1.0)), (oh[3], sh3[1], (0.0, 1.0))):
            assert np.all(plane[:-1] == (fresh if new else kept)), (ts, tn, want3)
            assert np.all(state[:-1] == (fresh if new else kept)) and np.all(state[-1] == 1.0), (ts, tn, want3)
        assert np.array_equal(oh[2:, :-1], oo[2:, :-1])
    print(f"refresh pairs dropped (oracle and numpy disagree), real*{prec}: {dropped} of {2 * len(PAIRS)}")
    assert seen == {True, False} and dropped == 0


# ----------------------------------------------------------------------------------------
# e. negative and far-off-range temperatures through the contrast kernels
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(dt, kwin):
    from oracle.pyoracle import Oracle
    nx, ny, nz = 256, 192, 2
    st = synth.static_fields(nx, ny, dt)
    orc = Oracle(8)
    f8 = lambda a: np.ascontiguousarray(a, dtype=F64)
    coast = orc.get_edges(f8(st.landfrac), f8(st.icefrac))
    cdist = orc.get_dist(coast, f8(st.landfrac), st.lon, st.lat, maxdist=20000.0, kwin=kwin)
    cdist = np.where(np.abs(cdist) < 12000.0, np.sign(cdist) * np.minimum(np.abs(cdist), 179.0), cdist).astype(dt)
    return st, cdist, synth.pressure_3d(st, nz, dt), nz


def _three_steps(hipctx, orc, dt, hint, kwin, shift):
    st, cdist, p, nz = _synthetic(dt, kwin)
    so, sh = ([np.zeros((st.ny, st.nx), dt) for _ in range(4)] for _ in range(2))
    lo, hi = np.inf, -np.inf
    with _hint(hipctx, hint):
        for tn in (1, 2, 3):
            th = (synth.theta_step(st, tn, F64) + shift).astype(dt)
            lo, hi = min(lo, float(th.min())), max(hi, float(th.max()))
            u, v = synth.wind_step(st, nz, tn, dt)
            orc.seabreeze_diag(7200.0, tn, p, u, v, th, cdist, st.z, st.sigma, *so, halo=0, bnd=1)
            hipctx.seabreeze_diag(7200.0, tn, p, u, v, th, cdist, st.z, st.sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
            yield tn, sh, so
    c = hipctx.last_counters()
    assert c["one_class_cells"] == 0 and c["max_radius"] == orc.last_nn_max and c["max_radius"] > (16 if hint > 16 else 4)
    assert (so[3] != 0).sum() > 100
    assert lo < shift + 300 and hi > shift + 270 and hi - lo > 20, (lo, hi)


@pytest.mark.parametrize("shift", [-273.15, -296.0], ids=["celsius", "around-zero"])
@pytest.mark.parametrize("prec,dt,hint", VARIANTS, ids=VARIANT_IDS)
def test_celsius_temperatures(hipctx, oracles, prec, dt, hint, shift):
    """theta in degrees Celsius (synth's fields then run from about 11 to 40: small, one sign) and shifted by 296 K
    (values on both sides of zero, t0 too), z as synth makes it: 256 x 192, three steps, held to the oracle on the same
    input as the Kelvin runs of test_parity_gpu.py are -- and in single precision without their mask around the 0.75 K
    threshold: sums of values within +-40 instead of near 290 leave the reference's own single-precision window sums
    some ten times less noise, and sb_con moves by at most 11 / 0.75 times the error of thc."""
    st = _synthetic(dt, 10)[0]
    th = synth.theta_step(st, 1, F64) + shift
    assert (th.min() < -5.0 and th.max() > 5.0) if shift < -290.0 else (0.0 < th.min() and th.max() < 45.0)
    for tn, sh, so in _three_steps(hipctx, oracles[prec], dt, hint, 10 if hint == 16 else 20, shift):
        for a, b, nm in zip(sh, so, ("ws", "wd", "thc", "sb_con")):
            if dt == F32 and nm == "wd":
                assert relerr(a, b, floor=1e-1) < 2e-5, tn     # as test_generic_flavour_fp32: libm's atan2f against the chip's
            else:
                _close(a, b, dt, f"shift {shift} hint={hint} tn={tn} {nm}", nm)
        if dt == F64:
            assert np.array_equal(sh[3] != 0, so[3] != 0), tn


@pytest.mark.parametrize("shift", [-288.0 - 1900.0, -288.0 + 1900.0], ids=["minus1900K", "plus1900K"])
def test_temperatures_near_the_fixed_point_range(hipctx, oracles, shift):
    """|t0| up to about 1950 K, inside the |t0| < 2048 K the strip kernel's 64-bit fixed point is documented for: the
    contrast does not change under a shift, so it is held to the oracle by absolute error (_assert_close64's floor)."""
    for tn, sh, so in _three_steps(hipctx, oracles[8], F64, 16, 10, shift):
        for a, b, nm in zip(sh, so, ("ws", "wd", "thc", "sb_con")):
            _assert_close64(a, b, f"shift {shift} tn={tn} {nm}")
        assert np.array_equal(sh[3] != 0, so[3] != 0), tn


@pytest.mark.parametrize("hint", [16, 24])
def test_contrast_is_linear_with_a_negative_slope(hipctx, hint):
    """With z = 0, thc(-1.5 theta - 10) = -1.5 thc(theta): every temperature negative, the contrast's sign turned."""
    st, cdist, p, nz = _synthetic(F64, 10 if hint == 16 else 20)
    th = synth.theta_step(st, 1, F64)
    u, v = synth.wind_step(st, nz, 1, F64)
    z0 = np.zeros_like(st.z)

    def thc_of(theta):
        s = [np.zeros((st.ny, st.nx), F64) for _ in range(4)]
        hipctx.seabreeze_diag(10800.0, 1, p, u, v, theta, cdist, z0, st.sigma, *s, halo=0, bnd=hip.SB_BND_GLOBAL)
        return s[2]

    with _hint(hipctx, hint):
        t1 = thc_of(th)
        t2 = thc_of(-1.5 * th - 10.0)
    assert (-1.5 * th - 10.0).max() < -400.0 and np.abs(t1).max() > 1.0
    assert relerr(t2, -1.5 * t1, floor=1e-2) < 1e-7
