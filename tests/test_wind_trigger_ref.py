"""CPU proof of the expectations of tests/test_wind_trigger_gpu.py: on exactly the directed inputs of
tests/wind_trigger_ref.py the plain reference functions, the hand-written `fires` column and the oracle
(oracle/pyoracle.py: seabreeze_diag with level_rule 0 and 1, diag) agree, and the table is not vacuous.

Double precision: sb_con, ws, wd and thc agree with the oracle bit for bit.  Single precision: ws, thc and sb_con bit
for bit too (every operation in them is one correctly rounded IEEE operation); wd to 4 units in the last place, the
room libm's atan2f and numpy's may differ by.  The fire pattern is the same in both precisions.
"""
import numpy as np
import pytest

import wind_trigger_ref as wr

PRECS = [(8, np.float64), (4, np.float32)]
TS_S, TS_MIN, TN = 1800.0, 30.0, 2           # tn = 2, 3600 s: between refreshes in both flavours


def _ulps(a, b):
    return np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(b), b.dtype.type(1e-3))))


def _oracle_generic(orc, tg, dt):
    ws, wd = tg.ws_old.copy(), tg.wd_old.copy()
    thc, sb = np.full_like(ws, -5.0), np.full_like(ws, np.nan)
    orc.seabreeze_diag(TS_S, TN, tg.p, tg.u, tg.v, tg.theta, tg.mask, tg.z, tg.sigma, ws, wd, thc, sb, halo=0, bnd=1)
    return sb, ws, wd, thc


def _oracle_f2py(orc, tg, dt, **kw):
    ws, wd = tg.ws_old.copy(), tg.wd_old.copy()
    thc = np.full_like(ws, -5.0)
    out = orc.diag(TN, tg.p[:, 0, 0].copy(), tg.z, tg.sigma, tg.theta, tg.v, tg.u, tg.mask, ws, wd, thc, timestep=TS_MIN, **kw)
    return out, ws, wd, thc


@pytest.mark.parametrize("nx", [130, 192])
@pytest.mark.parametrize("prec,dt", PRECS)
def test_table_reference_and_oracle_agree_generic(oracles, nx, prec, dt):
    tg = wr.trigger_grid(nx, dt)
    assert not wr.refresh(dt, TN, TS_S)
    sb, ws, wd, thc = _oracle_generic(oracles[prec], tg, dt)
    d = tg.directed
    # the contrast of every directed cell is exact
    assert np.array_equal(thc[d], tg.n_thc[d])
    assert np.array_equal(tg.theta, tg.theta.astype(np.float64).astype(dt))
    # the hand-written column is what the oracle does, in every directed cell and on the border rows
    assert np.array_equal(sb != 0, wr.expected_fires(tg))
    # the plain reference on the oracle's own contrast (exact where directed) equals the oracle
    ref = wr.trigger(dt, TN, False, thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0])
    assert np.array_equal(ref.sb_con, sb) and np.array_equal(ref.ws, ws) and np.array_equal(ref.wd, wd)
    assert np.array_equal(wd, tg.wd_old)                      # no refresh: the direction is carried
    assert np.array_equal(wr.nearest_level(tg.p, wr.TARGET_PLEV, dt), np.zeros_like(tg.case_id))


@pytest.mark.parametrize("prec,dt", PRECS)
def test_table_reference_and_oracle_agree_f2py(oracles, prec, dt):
    tg = wr.trigger_grid(130, dt)
    assert not wr.refresh_f2py(dt, TN, TS_MIN)
    out, ws, wd, thc = _oracle_f2py(oracles[prec], tg, dt)
    d = tg.directed.copy()
    d[-1] = False                                               # the surface leaves the last row alone (:165)
    assert np.array_equal(thc[d], tg.n_thc[d])
    assert np.array_equal((out[0] != 0)[:-1], wr.expected_fires(tg)[:-1])
    ref = wr.trigger(dt, TN, False, thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0], f2py=True)
    assert np.array_equal(ref.sb_con[:-1], out[0, :-1])
    # between refreshes the state and the output planes keep the preset values
    for a in (ws, out[2]):
        assert np.array_equal(a[:-1], tg.ws_old[:-1]) and np.array_equal(ref.ws, tg.ws_old)
    for a in (wd, out[3]):
        assert np.array_equal(a[:-1], tg.wd_old[:-1]) and np.array_equal(ref.wd, tg.wd_old)
    assert np.array_equal(out[1, :-1], tg.theta[:-1])         # z = 0: t0 is theta bit for bit


@pytest.mark.parametrize("prec,dt", PRECS)
def test_table_at_a_refresh_and_at_the_first_step(oracles, prec, dt):
    """The same cells at a refreshing call (tn = 12: the new direction is stored, where libm's atan2 enters) and at
    tn = 1 (the preset state is ignored: dws = dwd = 0)."""
    tg = wr.trigger_grid(130, dt)
    for tn in (12, 1):
        rf = wr.refresh(dt, tn, TS_S)
        assert rf == (tn == 12)
        ws, wd = tg.ws_old.copy(), tg.wd_old.copy()
        thc, sb = np.zeros_like(ws), np.zeros_like(ws)
        oracles[prec].seabreeze_diag(TS_S, tn, tg.p, tg.u, tg.v, tg.theta, tg.mask, tg.z, tg.sigma, ws, wd, thc, sb, halo=0, bnd=1)
        ref = wr.trigger(dt, tn, rf, thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0])
        assert np.array_equal(ref.ws, ws)
        assert np.array_equal(ref.sb_con, sb)                 # the direction enters it through a comparison only
        if prec == 8:
            assert np.array_equal(ref.wd, wd)
        else:
            assert _ulps(ref.wd, wd) <= 4


def test_fire_pattern_is_the_same_in_both_precisions(oracles):
    pats = []
    for prec, dt in PRECS:
        tg = wr.trigger_grid(130, dt)
        pats.append(_oracle_generic(oracles[prec], tg, dt)[0] != 0)
        ref = wr.trigger(dt, TN, False, tg.n_thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0])
        assert np.array_equal((ref.sb_con != 0)[tg.directed], pats[-1][tg.directed])
    assert np.array_equal(*pats)


@pytest.mark.parametrize("prec,dt", PRECS)
def test_intermediates_are_exact_and_the_table_is_not_vacuous(prec, dt):
    tg = wr.trigger_grid(130, dt)
    # one cell of every case and class
    rows = {}
    for y, x in zip(*np.nonzero(tg.directed)):
        rows.setdefault((int(tg.case_id[y, x]), bool(tg.land[y, x])), (y, x))
    assert len(rows) == 2 * len(wr.CASES)
    ref = wr.trigger(dt, TN, False, tg.n_thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0])
    th = wr.THRESHOLDS
    only = {"dwd": 0, "dws": 0, "mws": 0, "thc": 0}
    for (i, land), (y, x) in rows.items():
        c = wr.CASES[i]
        ok = dict(dwd=ref.dwd[y, x] < th["thresh_winddir"], dws=ref.dws[y, x] < th["thresh_windch"],
                  mws=ref.mws[y, x] < th["thresh_wind"], thc=abs(tg.n_thc[y, x]) > th["thresh_thc"])
        assert all(ok.values()) == c.fires, c.name
        assert (ref.sb_con[y, x] != 0) == c.fires, c.name
        failed = [k for k, v_ in ok.items() if not v_]
        if len(failed) == 1:
            only[failed[0]] += 1
        # dws and mws are exact: the same in both precisions, as the hand values of the table's comments
        assert float(ref.dws[y, x]) == abs(c.ws_old - np.hypot(c.u, c.v)), c.name
        assert float(ref.mws[y, x]) == (c.ws_old + np.hypot(c.u, c.v)) / 2, c.name
        # directions: exact (integers) or at least 1e-3 deg off the threshold, except the one row that is the quirk
        off = abs(float(ref.dwd[y, x]) - 90.0)
        if c.name == "turn_exact_90":
            assert 1e-4 < 90.0 - float(ref.dwd[y, x]) < 1.3e-4
        elif c.name in ("turn_90_state", "turn_-90_state"):
            assert float(ref.dwd[y, x]) == 90.0               # on the edge itself: exact in both precisions
        else:
            assert off >= 1e-3, (c.name, off)
        if c.fires:
            assert (ref.sb_con[y, x] < 0) == (tg.n_thc[y, x] < 0)
    assert all(n >= 2 for n in only.values()), only           # each condition is somewhere the only one that fails
    # both outcomes in every block whose contrast can pass at all (|L - S| > 0.75); the blocks at and below the
    # threshold can only give "no", and do so under winds that pass elsewhere
    for b in wr.BLOCKS:
        outcomes = {c.fires for c in wr.CASES if c.contrast == b}
        assert outcomes == ({True, False} if abs(wr.CONTRASTS[b]) > 0.75 else {False}), b
        assert any(c.contrast == b and (c.ws_old, c.wd_old, c.u, c.v) == (4.0, 0.0, 0.0, -4.0) for c in wr.CASES)
    # hand values of a few rows
    cell = lambda name, land=True: rows[([c.name for c in wr.CASES].index(name), land)]
    eps, one = dt(wr.EPS), dt(1)
    assert ref.sb_con[cell("mws_below_1")] == (eps / dt(0.75 + wr.EPS)) * (dt(10.5) / one)       # divisor 1, not 0.5
    assert ref.sb_con[cell("calm_aligned")] == (eps / dt(0.75 + wr.EPS)) * dt(11)
    assert ref.sb_con[cell("neg_all_pass")] == (eps / dt(-(0.75 + wr.EPS))) * (dt(7) / dt(4))
    assert ref.sb_con[cell("neg_all_pass", False)] == (eps / dt(0.75 + wr.EPS)) * (dt(7) / dt(4))
    # placement: every case on lanes 0 and 63, in the first and the last whole segment and in the ragged one
    for nx in (130, 192):
        g = wr.trigger_grid(nx, dt)
        for x in sorted({0, 63, 64, 127, nx - 2, nx - 1}):
            assert set(g.case_id[:, x][g.directed[:, x]]) == set(range(len(wr.CASES))), (nx, x)


def test_non_default_thresholds_change_the_outcome():
    """The values the GPU test passes as Tunables: other cells fire than under the defaults."""
    dt = np.float64
    tg = wr.trigger_grid(130, dt)
    base = wr.trigger(dt, TN, False, tg.n_thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0]).sb_con != 0
    for th in wr.TUNABLE_SETS:
        alt = wr.trigger(dt, TN, False, tg.n_thc, tg.ws_old, tg.wd_old, tg.u[0], tg.v[0], th).sb_con != 0
        assert (alt & ~base)[tg.directed].any() or (base & ~alt)[tg.directed].any(), th
        assert alt[tg.directed].any(), th


@pytest.mark.parametrize("nz", wr.NZ_LIST)
@pytest.mark.parametrize("prec,dt", PRECS)
def test_level_columns(oracles, nz, prec, dt):
    """The hand-written level of every column pattern equals nearest_level / um_walk_level and the oracle's choice,
    read back as ws = (level + 1) / 4 after a tn = 1 call."""
    nx, ny = 66, 3
    mask = wr.striped_mask(nx, ny, dt)
    theta = np.where(mask > 0, 289.0, 288.0).astype(dt)
    z = np.zeros((ny, nx), dt)
    sigma = (np.arange(ny * nx).reshape(ny, nx) % 5).astype(dt)
    for rule, columns in ((0, wr.generic_columns(nz)), (1, wr.um_columns(nz))):
        p, u, v, pat = wr.level_grid(columns, nx, ny, dt)
        hand = np.array([c[2] for c in columns])[pat]
        if rule == 0:
            lev, defined = wr.nearest_level(p, wr.TARGET_PLEV, dt), np.ones((ny, nx), bool)
        else:
            lev, defined = wr.um_walk_level(p, wr.TARGET_PLEV, dt)
            assert np.array_equal(defined, np.array([c[3] for c in columns])[pat])
            assert (~defined).sum() == (pat == [c[0] for c in columns].index("beyond_1e6")).sum()
        assert np.array_equal(lev[defined], hand[defined]), [c[0] for c in columns]
        st = [np.zeros((ny, nx), dt) for _ in range(4)]
        oracles[prec].seabreeze_diag(TS_S, 1, p, u, v, theta, mask, z, sigma, *st, halo=0, bnd=1, level_rule=rule)
        assert np.array_equal((st[0] * 4 - 1)[defined], lev[defined].astype(dt))
    # the two rules differ on these inputs wherever there is room to
    if nz >= 7:
        g = wr.nearest_level(wr.level_grid(wr.um_columns(nz), nx, ny, dt)[0], wr.TARGET_PLEV, dt)
        assert (g != lev).any()


def test_level_patterns_cross_the_batches():
    """For each batch size the list holds minima at the last level of a batch, at the first of the next, ties across
    that boundary, and levels in a ragged second and third batch."""
    for un in wr.UNS:
        hit = set()
        for nz in wr.NZ_LIST:
            for name, col, lev in wr.generic_columns(nz):
                hit.add((lev % un, lev // un, nz % un != 0))
        assert {(un - 1, 0), (0, 1)} <= {(a, b) for a, b, _ in hit}
        assert any(b >= 1 and ragged for _, b, ragged in hit) and any(b >= 2 for _, b, _ in hit)


@pytest.mark.parametrize("prec,dt", PRECS)
def test_refresh_pairs(oracles, prec, dt):
    """refresh() against the oracle's MODULO on every pair, both flavours; the documented properties of the pairs."""
    nx, ny = 8, 4
    mask = wr.striped_mask(nx, ny, dt)
    theta = np.where(mask > 0, 289.0, 288.0).astype(dt)
    z = np.zeros((ny, nx), dt)
    sigma = (np.arange(ny * nx).reshape(ny, nx) % 5).astype(dt)
    p = np.full((1, ny, nx), 70000.0, dt)
    u = np.zeros((1, ny, nx), dt)
    v = np.full((1, ny, nx), -4.0, dt)
    disagree = 0
    for ts, tn in wr.REFRESH_PAIRS:
        st = [np.full((ny, nx), 1.0, dt) for _ in range(4)]
        oracles[prec].seabreeze_diag(ts, tn, p, u, v, theta, mask, z, sigma, *st, halo=0, bnd=1)
        disagree += bool(st[1][0, 0] != 1.0) != wr.refresh(dt, tn, ts)
        s3 = [np.full((ny, nx), 1.0, dt) for _ in range(3)]
        oracles[prec].diag(tn, p[:, 0, 0].copy(), z, sigma, theta, v, u, mask, *s3, timestep=ts / 60.0)
        disagree += bool(s3[0][0, 0] != 1.0) != wr.refresh_f2py(dt, tn, ts / 60.0)
    print(f"refresh pairs on which oracle and numpy disagree (real*{prec}): {disagree}")
    assert disagree == 0
    r = lambda ts, tn: wr.refresh(dt, tn, ts)
    assert r(1800.0, 12) and not r(1800.0, 11) and r(7200.0, 3) and r(1e-5, 1) and r(0.1, 216000)
    assert r(0.3, 216000) == (prec == 8)                      # the product rounds to 64800.004 in single precision
    for ts, tn in wr.REFRESH_PAIRS[-3:]:
        assert 21599.0 < float(np.fmod(dt(tn) * dt(ts), dt(21600))) < 21600.0 and not r(ts, tn)
