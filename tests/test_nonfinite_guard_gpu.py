"""The opt-in guard for missing and non-finite temperatures (sb_set_nonfinite_guard, sb_guard_kernels.hip,
include/seabreeze_hip.h) on the device, against the oracle (oracle/sb_oracle.f90, which tests/test_guard_oracle_pin.py holds
to the compiled reference on such input).

Grids: 160 x 96 with the synthetic coast (every radius 1) under k_strip (fp64, hint 16, fold on and off), k_strip32 (fp32,
hint 31) and k_thc3 (fp64, hint 24, sb_set_wide_strip(ctx, 0)); 176 x 128 with two 40-cell blocks of land and every cell in
the band (radii up to 60) under the tables, with and without the window cache, and under k_strip, where most cells lie
beyond the kernel's reach; the same blocks with the band cut to 24 cells under the f2py flavour's tables; the UM layout with
halo_s = 2; the f2py flavour on 160 x 96 under k_strip and under its tables.
Three steps, the bad cells present at step 2 only: the strip kernel's stored plan and the stored windows of the table
cache are in use when they appear (l).

What is held, per case:
 1  isnan and signed isinf of thc and sb_con (f2py flavour: thc, output[0:2]) equal the oracle's, cell for cell;
 2  fp64: finite cells within 1e-7 max(|ref|, 1e-2) of the oracle;
 3  fp32: band cells whose final window holds no bad cell go by oracle/fp32_criterion.py against the fp64 oracle; band cells
    whose window holds a FINITE bad value (2e20) have thc within
        2 (2 nn + 1)^2 2^-24 max(sum_l |t0| / n_l, sum_s |t0| / n_s)
    of the fp32 oracle -- the bound on the oracle's own sequential fp32 accumulation of a (2 nn + 1)^2 window, computed
    here from the inputs;
 4  band cells outside the specified taint (tests/guard_ref.py) hold the same bits with the guard on and off on the same
    poisoned field: the cancellation claim, per kernel;
 5  without a bad cell every output is bit for bit the guard-off call's, the report says 0 found, 0 recomputed;
 6  step 3 is bit for bit the step 3 of a run that never saw the bad cell;
 7  guard_report: [0] the bad frame cells, [1] at least the exact affected count -- and exactly the specified taint's;
 8  sb_last_counters identical with the guard on and off;  9  sb_last_step_report: the plan's launches plus four;
10  a band step and a call with gathered moments enqueue what they enqueue without the switch.
"""
import numpy as np
import pytest
import torch

import guard_ref as gr
import radius_ref as rr
import table_ref as tr
from oracle import fp32_criterion as crit
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

DT_S, NZ = 7200.0, 2
f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
NAMES = ("ws", "wd", "thc", "sb_con")

# name -> dtype, setup of the context, the guard's reach as guard_ref states it, launches of the call without the guard
KERNELS = {
    "strip-fp64": (np.float64, dict(hint=16), dict(reach=16), 3),
    "strip-kprep-fp64": (np.float64, dict(hint=16, fold=False), dict(reach=16), 4),
    "strip32-fp32": (np.float32, dict(hint=31), dict(reach=31), 3),
    "tile-fp64": (np.float64, dict(hint=24, wide=False), dict(tile=(32, 32, 24)), 4),
    "table-fp64": (np.float64, dict(hint=16, table=True), dict(reach=127), 6),
    "table-cache-fp64": (np.float64, dict(hint=16, table=True, cache=True), dict(reach=127), 6),
}


def _setup(ctx, hint=16, fold=True, wide=True, table=False, cache=False, f2py=False):
    ctx.set_search_radius_hint(hint)
    ctx.set_fold(fold)
    ctx.set_wide_strip(wide)
    ctx.set_table_contrast(table)
    ctx.set_table_contrast_f2py(f2py)
    ctx.set_table_window_cache(cache)


def _pattern(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN at {np.argwhere(np.isnan(a) != np.isnan(b))[:4].tolist()}"
    for s, nm in ((np.isposinf, "+Inf"), (np.isneginf, "-Inf")):
        assert np.array_equal(s(a), s(b)), f"{what}: {nm} at {np.argwhere(s(a) != s(b))[:4].tolist()}"


def _close64(a, b, what):
    """|a - b| <= 1e-7 max(|b|, 1e-2) on the cells where the oracle is finite"""
    fin = np.isfinite(b)
    e = np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-2)
    assert e.size == 0 or float(e.max()) < 1e-7, f"{what}: rel err {float(e.max())}"


def _same_bits(a, b, what, where=None):
    va, vb = (np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32) for x in (a, b))
    ne = va != vb if where is None else (va != vb) & where
    assert not ne.any(), f"{what}: {int(ne.sum())} cells differ, first {np.argwhere(ne)[:4].tolist()}"


class Field:
    """One grid's inputs in the host-model layout: static fields, p, per step (theta, z, u, v) with the bad cells of `spec` set
    at the steps of `when`, the mask, ghost width and boundary rule."""

    def __init__(self, dt, st, p, mask, per, halo=0, bnd=hip.SB_BND_GLOBAL, sigma=None, z=None, omp=False):
        self.dt, self.st, self.p, self.mask, self.per, self.halo, self.bnd = dt, st, p, mask, per, halo, bnd
        self.omp = omp                  # the oracle's all-core point loop (the same arithmetic per cell): windows of 60 cells and more
        self.refs = {}                  # the oracle's answers per set of bad cells, shared by the kernels that run on this field
        self.sigma = st.sigma if sigma is None else sigma
        self.z = st.z if z is None else z
        self.ny, self.nx = mask.shape[0] - 2 * halo, mask.shape[1] - 2 * halo
        self.obnd = {hip.SB_BND_WRAPPER: 0, hip.SB_BND_GLOBAL: 1, hip.SB_BND_HALO: 2}[bnd]

    def step(self, tn, spec, when):
        th, u, v = self.per[tn]
        if tn in when:
            th, z = gr.poison(th, self.z, spec, self.halo)
        else:
            th, z = th, self.z
        return th, z, u, v


def _global_field(orc, dt, steps=(1, 2, 3)):
    st, cd = gr.global_field(orc, dt)
    per = {tn: (synth.theta_step(st, tn, dt),) + synth.wind_step(st, NZ, tn, dt) for tn in steps}
    return Field(dt, st, synth.pressure_3d(st, NZ, dt), cd.astype(dt), per)


def _table_field(dt, steps=(1, 2, 3)):
    nx, ny = gr.TABLE_GRID
    st, p, per, mask = tr.inputs(nx, ny, gr.table_land(), dt, steps=steps)
    return Field(dt, st, p, mask, per, omp=True)


def _run_hip(ctx, f, spec, when, guard, steps=(1, 2, 3)):
    """-> {tn: (state after the call, last_counters, last_step_report, guard_report)}"""
    ctx.set_nonfinite_guard(guard)
    state = tr.zeros(4, f.dt, f.ny, f.nx)
    out = {}
    for tn in steps:
        th, z, u, v = f.step(tn, spec, when)
        ctx.seabreeze_diag(DT_S, tn, f.p, u, v, th, f.mask, z, f.sigma, *state, halo=f.halo, bnd=f.bnd)
        out[tn] = ([a.copy() for a in state], ctx.last_counters(), ctx.last_step_report(), ctx.guard_report())
    return out


def _omp_oracle(prec):
    import os
    from oracle.pyoracle import Oracle
    os.environ.setdefault("OMP_NUM_THREADS", str(min(16, len(os.sched_getaffinity(0)))))
    return Oracle(prec, omp=True)


def _run_oracle(oracles, prec, f, spec, when, steps=(1, 2, 3), cast=None):
    key = (prec, cast is f8, repr(spec), tuple(when), tuple(steps))
    if key in f.refs:
        return f.refs[key]
    orc = _omp_oracle(prec) if f.omp else oracles[prec]
    cast = cast or (lambda a: a)
    dt = np.float64 if cast is f8 else f.dt
    state = tr.zeros(4, dt, f.ny, f.nx)
    out = {}
    for tn in steps:
        th, z, u, v = f.step(tn, spec, when)
        orc.seabreeze_diag(DT_S, tn, cast(f.p), cast(u), cast(v), cast(th), cast(f.mask), cast(z), cast(f.sigma), *state,
                           halo=f.halo, bnd=f.obnd, omp=f.omp)
        out[tn] = [a.copy() for a in state]
    f.refs[key] = out
    return out


def _window_bound(f, th, z, orc, cells, radius):
    """check 3's bound for the band cells `cells` [(y, x)]: 2 (2nn+1)^2 2^-24 max(sum_l |t0| / n_l, sum_s |t0| / n_s), from the inputs"""
    t0 = np.abs(tr.t0_of(orc, f8(th), f8(z), f8(f.sigma), f.halo))
    land = f.mask >= 0
    out = {}
    for (y, x) in cells:
        nn = int(radius[y, x])
        d = np.arange(-nn, nn + 1)
        X, Y = rr.map_x(x + d, f.nx, f.halo, f.obnd, None), rr.map_y(y + d, f.ny, f.halo, f.obnd, None)
        w, l = t0[np.ix_(Y[Y >= 0], X[X >= 0])], land[np.ix_(Y[Y >= 0], X[X >= 0])]
        out[(y, x)] = 2.0 * (2 * nn + 1) ** 2 * 2.0 ** -24 * max(w[l].sum() / l.sum(), w[~l].sum() / (~l).sum())
    return out


def _hold_case(ctx, oracles, f, spec, kw_reach, base_launches, what, when=(2,)):
    """checks 1 - 4 and 6 - 9 for one field, one kernel, one set of bad cells"""
    prec = np.dtype(f.dt).itemsize
    on = _run_hip(ctx, f, spec, when, True)
    off = _run_hip(ctx, f, spec, when, False)
    clean = _run_hip(ctx, f, spec, (), True)
    ref = _run_oracle(oracles, prec, f, spec, when)
    ref8 = ref if prec == 8 else _run_oracle(oracles, 8, f, spec, when, cast=f8)
    for tn in (1, 2, 3):
        th, z, _, _ = f.step(tn, spec, when)
        bad = gr.bad_plane(th, z)
        exact, radius, isband = gr.affected(bad, f.mask, 180.0, f.halo, f.obnd)
        taint = gr.specified_taint(bad, isband, f.halo, f.obnd, **kw_reach)
        got, counters, launches, rep = on[tn]
        w = f"{what} step {tn}"
        assert (tn in when) == bool(bad.any())
        # 1
        for nm, a, b in zip(NAMES, got, ref[tn]):
            _pattern(a, b, f"{w} {nm}")
        # 2 / 3
        if prec == 8:
            for nm, a, b in zip(NAMES, got, ref[tn]):
                _close64(a, b, f"{w} {nm}")
        else:
            prev_g = on[tn - 1][0] if tn > 1 else tr.zeros(4, f.dt, f.ny, f.nx)
            prev_o = ref8[tn - 1] if tn > 1 else tr.zeros(4, np.float64, f.ny, f.nx)
            res = crit.merge([crit.check_step(tn, prev_g, got, prev_o, ref8[tn], isband & ~exact, timestep=DT_S)])
            assert res["ok"], (w, res)
            fin = exact & np.isfinite(ref[tn][2])
            _, fr = gr.final_radius(f.mask, 180.0, f.halo, f.obnd)
            bound = _window_bound(f, th, z, oracles[8], [tuple(c) for c in np.argwhere(fin)], fr)
            for (y, x), bnd in bound.items():
                d = abs(float(got[2][y, x]) - float(ref[tn][2][y, x]))
                assert d <= bnd, f"{w} thc[{y},{x}]: {d} > {bnd}"
        # 4
        for k in (2, 3):
            _same_bits(got[k], off[tn][0][k], f"{w} {NAMES[k]} outside the taint, guard on against off", where=isband & ~taint)
        _same_bits(got[0], off[tn][0][0], f"{w} ws")
        _same_bits(got[1], off[tn][0][1], f"{w} wd")
        # 7, 8, 9
        assert rep["bad_cells"] == int(bad.sum()), (w, rep)
        assert rep["repaired_cells"] >= int(exact.sum() if radius.max() <= (kw_reach.get("reach") or kw_reach["tile"][2]) else
                                            (exact & gr.within_reach(radius, **kw_reach)).sum()), (w, rep, int(exact.sum()))
        assert rep["repaired_cells"] == int(taint.sum()), (w, rep, int(taint.sum()))
        assert rep["calls"] == tn and rep["calls_with_bad"] == sum(1 for t in when if t <= tn), (w, rep)
        assert counters == off[tn][1], (w, counters, off[tn][1])
        assert launches == dict(off[tn][2], kernel_launches=off[tn][2]["kernel_launches"] + 4), (w, launches)
        assert off[tn][2]["kernel_launches"] == base_launches and off[tn][3] == dict(bad_cells=0, repaired_cells=0, calls_with_bad=0, calls=0)
    # check 1 fails with the guard off: the bad cells leave a finite, wrong thc somewhere
    if spec and any(np.isnan(v) or np.isinf(v) for *_, v in spec):
        with pytest.raises(AssertionError):
            for nm, a, b in zip(NAMES, off[2][0], ref[2]):
                _pattern(a, b, nm)
    # 6
    for nm, a, b in zip(NAMES, on[3][0], clean[3][0]):
        _same_bits(a, b, f"{what} step 3 {nm} against a run that never saw the bad cell")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def global_fields(oracles):
    return {dt: _global_field(oracles[np.dtype(dt).itemsize], dt) for dt in (np.float64, np.float32)}


@pytest.fixture(scope="module")
def table_fields():
    return {np.float64: _table_field(np.float64)}


CASES = ("a_nan_land_coast", "b_inf_sea_centre", "c_missing_off_band", "d_nan_strip_block_corner", "e_nan_pole_row_and_seam",
         "h_nan_in_z_land", "i_inf_land_and_sea", "k_missing_block")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kernel", ["strip-fp64", "strip-kprep-fp64", "strip32-fp32", "tile-fp64"])
def test_directed_cells_on_the_coast_grid(ctx, oracles, global_fields, kernel, case):
    dt, setup, reach, launches = KERNELS[kernel]
    f = global_fields[dt]
    radius = rr.search_radius(f.mask, 180.0, 0, rr.BND_GLOBAL)
    spec = gr.directed(f.mask >= 0, radius != 0, radius)[case]
    _setup(ctx, **setup)
    _hold_case(ctx, oracles, f, spec, reach, launches, f"{kernel} {case}")


# gr.table_land(): the southern block on columns 136 .. 175 (up to the seam) and rows 0 .. 39, the mid-ocean block on columns
# 48 .. 87 and rows 70 .. 109
TABLE_CASES = {
    # a land cell on the west coast of the southern block; the sea cell beside it
    "nan_coast": [("theta", 20, 136, gr.NAN)],
    "inf_sea_centre": [("theta", 20, 135, gr.INF)],
    "inf_land_and_sea": [("theta", 20, 136, gr.INF), ("theta", 20, 135, gr.INF)],
    # (e) the pole rows, which the latitude clamp reads once per row beyond the pole, and the last column, across the seam
    "nan_pole_rows_and_seam": [("theta", 0, 150, gr.NAN), ("theta", 127, 100, gr.NAN), ("theta", 60, 175, gr.NAN)],
    # (k) 40 x 40 missing values across a corner of the mid-ocean block
    "missing_block": [("theta", y, x, gr.MISSING) for y in range(60, 100) for x in range(30, 70)],
}


@pytest.mark.parametrize("case", list(TABLE_CASES))
@pytest.mark.parametrize("kernel", ["table-fp64", "table-cache-fp64", "strip-fp64"])
def test_block_grid_radii_beyond_the_strip_kernels(ctx, oracles, table_fields, kernel, case):
    """The tables answer every cell (reach 127); under k_strip most cells lie beyond the reach and take the global-memory
    search, which the guard leaves alone: right with a finite centre, and a bad centre is always tainted."""
    dt, setup, reach, launches = KERNELS[kernel]
    f = table_fields[dt]
    _setup(ctx, **setup)
    _hold_case(ctx, oracles, f, TABLE_CASES[case], reach, launches, f"{kernel} {case}")


def test_block_grid_land_layout():
    land = gr.table_land()
    assert land[20, 136] and not land[20, 135] and land[0, 150] and not land[127, 100] and land[75, 50] and not land[60, 175]
    assert land[0:40, 136:176].all() and land[70:110, 48:88].all() and int(land.sum()) == 2 * 40 * 40
    assert land[60:100, 30:70].any() and not land[60:100, 30:70].all()


@pytest.mark.parametrize("kernel", ["strip-fp64", "strip32-fp32", "tile-fp64", "table-fp64", "table-cache-fp64"])
def test_no_bad_cell(ctx, oracles, global_fields, table_fields, kernel):
    """(j), check 5: bit for bit the guard-off call, 0 found, 0 recomputed, the calls counted"""
    dt, setup, reach, launches = KERNELS[kernel]
    f = table_fields[dt] if "table" in kernel else global_fields[dt]
    _setup(ctx, **setup)
    on = _run_hip(ctx, f, [], (), True)
    off = _run_hip(ctx, f, [], (), False)
    for tn in (1, 2, 3):
        for nm, a, b in zip(NAMES, on[tn][0], off[tn][0]):
            _same_bits(a, b, f"{kernel} step {tn} {nm}")
        assert on[tn][3] == dict(bad_cells=0, repaired_cells=0, calls_with_bad=0, calls=tn)
        assert on[tn][1] == off[tn][1]
        assert on[tn][2]["kernel_launches"] == launches + 4 and off[tn][2]["kernel_launches"] == launches
    _hold_case(ctx, oracles, f, [], reach, launches, f"{kernel} no bad cell", when=())


def test_stored_windows_in_use_when_the_bad_cell_appears(ctx, oracles, table_fields):
    """(l) with the window cache: step 2, which meets the bad cell, answers every band cell from the windows step 1 stored"""
    f = table_fields[np.float64]
    _setup(ctx, hint=16, table=True, cache=True)
    ctx.set_nonfinite_guard(True)
    state = tr.zeros(4, f.dt, f.ny, f.nx)
    ref = tr.zeros(4, f.dt, f.ny, f.nx)
    for tn in (1, 2):
        th, z, u, v = f.step(tn, TABLE_CASES["nan_coast"], (2,))
        ctx.seabreeze_diag(DT_S, tn, f.p, u, v, th, f.mask, z, f.sigma, *state)
        _omp_oracle(8).seabreeze_diag(DT_S, tn, f.p, u, v, th, f.mask, z, f.sigma, *ref, halo=0, bnd=1, omp=True)
        rep = ctx.table_cache_report()
        assert (rep["stored_cells"] > 0 and rep["searched_cells"] == 0) == (tn == 2), rep
    assert ctx.guard_report()["bad_cells"] == 1
    for nm, a, b in zip(NAMES, state, ref):
        _pattern(a, b, nm)
        _close64(a, b, nm)


# ---- the UM layout ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_um_ghost_cell(oracles, dt):
    """(g) halo_s = 2: a NaN in a ghost cell of theta's frame, inside the windows of band cells on the interior's edge"""
    hs, hl = 2, 6
    orc, orc8 = oracles[np.dtype(dt).itemsize], oracles[8]
    st, cd_l, inner = gr.um_field(orc, dt, hs, hl)
    nx, ny = gr.GRID
    cd_s = inner(cd_l, hs)
    radius = rr.search_radius(cd_s, 180.0, hs, rr.BND_HALO)
    Y, X = gr.um_ghost_cell(radius != 0, radius, hs)
    p, z_s, sg_s = inner(synth.pressure_3d(st, NZ, dt), 0), inner(st.z, hs), inner(st.sigma, hs)
    c = hip.Context(0)
    try:
        c.set_search_radius_hint(16)
        res = {}
        for guard in (True, False):
            c.set_nonfinite_guard(guard)
            state, ref, ref8 = tr.zeros(4, dt, ny, nx), tr.zeros(4, dt, ny, nx), tr.zeros(4, np.float64, ny, nx)
            for tn in (1, 2, 3):
                th = inner(synth.theta_step(st, tn, dt), hs)
                u, v = (inner(a, 0) for a in synth.wind_step(st, NZ, tn, dt))
                if tn == 2:
                    th[Y, X] = np.nan
                bad = gr.bad_plane(th, z_s)
                assert c.seabreeze_diag_um(DT_S, tn, p, u, v, th.copy(), z_s, sg_s, cd_l, *state, halo_s=hs, halo_l=hl) == 0
                orc.seabreeze_diag(DT_S, tn, p, u, v, th, cd_s, z_s, sg_s, *ref, halo=hs, bnd=2)
                orc8.seabreeze_diag(DT_S, tn, f8(p), f8(u), f8(v), f8(th), f8(cd_s), f8(z_s), f8(sg_s), *ref8, halo=hs, bnd=2)
                res[(guard, tn)] = [a.copy() for a in state]
                if not guard:
                    continue
                exact, _, isband = gr.affected(bad, cd_s, 180.0, hs, rr.BND_HALO)
                taint = gr.specified_taint(bad, isband, hs, rr.BND_HALO, reach=16)
                assert exact.any() == (tn == 2)
                rep = c.guard_report()
                assert rep["bad_cells"] == int(bad.sum()) and rep["repaired_cells"] == int(taint.sum()) >= int(exact.sum()), rep
                assert c.last_step_report()["kernel_launches"] == 3 + 4
                for nm, a, b in zip(NAMES, state, ref):
                    _pattern(a, b, f"step {tn} {nm}")
                    if dt == np.float64:
                        _close64(a, b, f"step {tn} {nm}")
                    elif nm == "thc":                    # (oracle/fp32_criterion.py: thc_abs_K against the fp64 oracle, clean windows)
                        fin = np.isfinite(ref8[2]) & isband & ~exact
                        assert np.max(np.abs(a[fin].astype(np.float64) - ref8[2][fin])) < crit.TOL["thc_abs_K"]
        with pytest.raises(AssertionError):
            _pattern(res[(False, 2)][2], res[(True, 2)][2], "thc with the guard off")
    finally:
        c.close()


# ---- the f2py flavour ---------------------------------------------------------------------------------------------------------

def _run_f2py(c, orc, st, cd, nps, steps, spec, guard, dt):
    c.set_nonfinite_guard(guard)
    p = synth.pressure_1d(nps, dt)
    wh, wo = tr.zeros(3, dt, *cd.shape), tr.zeros(3, dt, *cd.shape)
    out = {}
    for tn in steps:
        th = synth.theta_step(st, tn, dt)
        u, v = synth.wind_step(st, nps, tn, dt)
        if tn == 2:
            th, _ = gr.poison(th, st.z, spec)
        oh = c.diag(tn, p, st.z, st.sigma, th, v, u, cd, *wh)
        oo = orc.diag(tn, p, st.z, st.sigma, th, v, u, cd, *wo) if orc is not None else None
        out[tn] = (oh.copy(), [a.copy() for a in wh], oo, [a.copy() for a in wo], c.guard_report(), c.last_step_report())
    return out


@pytest.mark.parametrize("table", [False, True], ids=["strip", "tables"])
def test_f2py_last_column_and_seam(oracles, table):
    """(f) the wrapper's index rule never reads the last column: a NaN there changes no thc (t0, an output of the flavour,
    shows it); a NaN in column 1 changes band cells on both sides of the seam, the last column's included"""
    dt, orc = np.float64, oracles[8]
    st, cd = gr.global_field(orc, dt)
    nx, ny = gr.GRID
    radius = rr.search_radius(cd, 180.0, 0, rr.BND_WRAPPER)
    isband = radius != 0
    y = int(np.flatnonzero(isband[:, nx - 1] | isband[:, 0] | isband[:, 1] | isband[:, nx - 2])[0])
    reach = 127 if table else 16
    c = hip.Context(0)
    try:
        _setup(c, hint=16, table=table, f2py=table)
        clean = _run_f2py(c, None, st, cd, 3, (1, 2, 3), [], True, dt)
        for x, hit in ((nx - 1, False), (0, True)):
            spec = [("theta", y, x, gr.NAN)]
            on = _run_f2py(c, orc, st, cd, 3, (1, 2, 3), spec, True, dt)
            off = _run_f2py(c, None, st, cd, 3, (1, 2, 3), spec, False, dt)
            bad = gr.bad_plane(*gr.poison(synth.theta_step(st, 2, dt), st.z, spec))
            exact, _, _ = gr.affected(bad, cd, 180.0, 0, rr.BND_WRAPPER)
            taint = gr.specified_taint(bad, isband, 0, rr.BND_WRAPPER, reach=reach)
            assert exact.any() == hit and taint.any() == hit
            for tn in (1, 2, 3):
                oh, wh, oo, wo, rep, launches = on[tn]
                assert launches["kernel_launches"] == (6 if table else 5) + 4 and off[tn][5]["kernel_launches"] == (6 if table else 5)
                assert rep["bad_cells"] == (1 if tn == 2 else 0) and rep["repaired_cells"] == (int(taint.sum()) if tn == 2 else 0), rep
                _pattern(wh[2], wo[2], f"column {x} step {tn} thc")
                _close64(wh[2], wo[2], f"column {x} step {tn} thc")
                for k, nm in enumerate(("sb_con", "t0")):
                    _pattern(oh[k, :-1], oo[k, :-1], f"column {x} step {tn} {nm}")
                    _close64(oh[k, :-1], oo[k, :-1], f"column {x} step {tn} {nm}")
                _same_bits(wh[2], off[tn][1][2], f"column {x} step {tn}: thc outside the taint", where=isband & ~taint)
            if not hit:
                _same_bits(on[2][1][2], clean[2][1][2], "NaN in the last column: no thc changes")
                assert np.isnan(on[2][0][1, y, nx - 1]) and np.isnan(on[2][0][1]).sum() == 1
            else:
                cols = np.unique(np.argwhere(np.isnan(on[2][1][2]))[:, 1])
                assert (cols >= nx - 2).any() and (cols <= 1).any(), cols
                with pytest.raises(AssertionError):
                    _pattern(off[2][1][2], on[2][3][2], "thc with the guard off")
            _same_bits(on[3][1][2], clean[3][1][2], "step 3 thc")
            _same_bits(on[3][0][0], clean[3][0][0], "step 3 sb_con")
    finally:
        c.close()


@pytest.mark.parametrize("case", ["nan_coast", "inf_sea_centre", "missing_block"])
def test_f2py_tables_on_the_block_grid(oracles, case):
    """sb_set_table_contrast_f2py: the f2py flavour on the tables, the wrapper's rule across the seam the southern block
    touches.  The band is cut to the cells within 24 cells of a block -- radii up to 24 -- because the flavour's oracle has
    no all-core form and re-sums every window at every radius."""
    dt, orc = np.float64, oracles[8]
    nx, ny = gr.TABLE_GRID
    land = gr.table_land()
    st, _, _, cd = tr.inputs(nx, ny, land, dt, steps=())
    near = np.zeros_like(land)
    for dy in range(-24, 25):
        rows = np.clip(np.arange(ny) + dy, 0, ny - 1)
        for dx in range(-24, 25):
            near |= land[rows][:, (np.arange(nx) + dx) % nx]
    cd = np.where(near, cd, np.sign(cd) * 12000.0).astype(dt)
    radius = rr.search_radius(cd, 180.0, 0, rr.BND_WRAPPER)
    isband = radius != 0
    spec = TABLE_CASES[case]
    c = hip.Context(0)
    try:
        _setup(c, hint=16, table=True, f2py=True)
        on = _run_f2py(c, orc, st, cd, NZ, (1, 2, 3), spec, True, dt)
        off = _run_f2py(c, None, st, cd, NZ, (1, 2, 3), spec, False, dt)
        clean = _run_f2py(c, None, st, cd, NZ, (1, 2, 3), [], True, dt)
        bad = gr.bad_plane(*gr.poison(synth.theta_step(st, 2, dt), st.z, spec))
        exact, _, _ = gr.affected(bad, cd, 180.0, 0, rr.BND_WRAPPER)
        taint = gr.specified_taint(bad, isband, 0, rr.BND_WRAPPER, reach=127)
        assert exact.any() and not (exact & ~taint).any()
        for tn in (1, 2, 3):
            oh, wh, oo, wo, rep, launches = on[tn]
            assert launches["kernel_launches"] == 6 + 4 and off[tn][5]["kernel_launches"] == 6
            assert rep["bad_cells"] == (len(spec) if tn == 2 else 0) and rep["repaired_cells"] == (int(taint.sum()) if tn == 2 else 0), rep
            _pattern(wh[2], wo[2], f"step {tn} thc")
            _close64(wh[2], wo[2], f"step {tn} thc")
            for k, nm in enumerate(("sb_con", "t0")):
                _pattern(oh[k, :-1], oo[k, :-1], f"step {tn} {nm}")
                _close64(oh[k, :-1], oo[k, :-1], f"step {tn} {nm}")
            _same_bits(wh[2], off[tn][1][2], f"step {tn}: thc outside the taint", where=isband & ~(taint if tn == 2 else False))
        _same_bits(on[3][1][2], clean[3][1][2], "step 3 thc")
        _same_bits(on[3][0][0], clean[3][0][0], "step 3 sb_con")
    finally:
        c.close()


# ---- calls the guard does not serve ---------------------------------------------------------------------------------------------

def test_band_step_and_gathered_moments_ignore_the_switch(oracles):
    """check 10: a band step and a whole call with gathered moments on a context with the switch on enqueue what the same
    sequence enqueues on a context that never heard of it, and give the same bits; the report is all zeros after them; a
    whole call on that same context is served"""
    nx, ny, nz, h = 200, 96, 3, 6
    dt, orc = np.float64, oracles[8]
    st = synth.static_fields(nx, ny, dt)
    coast = orc.get_edges(st.landfrac, st.icefrac)
    cdist = orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=900.0, kwin=h - 1)
    cdist[np.abs(cdist) > 180.0] = 12000.0
    p = synth.pressure_3d(st, nz, dt)
    ctxs = {False: hip.Context(0), True: hip.Context(0)}
    c = ctxs[True]
    try:
        for cc in ctxs.values():
            cc.set_search_radius_hint(h)
        stream = torch.cuda.current_stream().cuda_stream

        def frame(a):
            f = torch.zeros((ny + 2 * h, nx + 2 * h), dtype=torch.float64, device="cuda")
            f[h:h + ny, h:h + nx] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            c.swap_bounds_dev(dt, f.data_ptr(), nx, ny, h, stream)
            return f

        z, sg, mk = frame(st.z), frame(st.sigma), frame(cdist)
        pd = torch.from_numpy(p).cuda()
        gath = torch.zeros(5, dtype=torch.float64, device="cuda")
        c.sigma_moments_dev(dt, nx, ny, h, sg.data_ptr(), gath.data_ptr(), stream)
        torch.cuda.synchronize()
        res = {}
        for guard in (False, True):
            c = ctxs[guard]
            if guard:
                c.set_nonfinite_guard(True)
            for kind in ("band", "gathered"):
                state = [torch.zeros((ny, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
                reports = []
                for tn in (1, 2):
                    th = synth.theta_step(st, tn, dt)
                    u, v = synth.wind_step(st, nz, tn, dt)
                    thf, ud, vd = frame(th), torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
                    args = (pd.data_ptr(), ud.data_ptr(), vd.data_ptr(), thf.data_ptr(), mk.data_ptr(), z.data_ptr(), sg.data_ptr(),
                            *[s.data_ptr() for s in state])
                    if kind == "band":
                        c.band_seabreeze_diag_dev(dt, 5400.0, tn, nx, ny, nz, h, *args, stream)
                    else:
                        c.use_gathered_moments(gath.data_ptr(), 1)
                        c.seabreeze_diag_dev(dt, 5400.0, tn, nx, ny, nz, h, hip.SB_BND_HALO, *args, stream)
                        c.use_gathered_moments(None, 0)
                    torch.cuda.synchronize()
                    reports.append(c.last_step_report())
                    assert c.guard_report() == dict(bad_cells=0, repaired_cells=0, calls_with_bad=0, calls=0)
                res[(guard, kind)] = (reports, [s.cpu().numpy() for s in state])
        for kind in ("band", "gathered"):
            assert res[(True, kind)][0] == res[(False, kind)][0], (kind, res[(True, kind)][0], res[(False, kind)][0])
            for nm, a, b in zip(NAMES, res[(True, kind)][1], res[(False, kind)][1]):
                _same_bits(a, b, f"{kind} {nm}")
        # ... and a whole call on the same context is served
        state = tr.zeros(4, dt, ny, nx)
        th = synth.theta_step(st, 1, dt)
        u, v = synth.wind_step(st, nz, 1, dt)
        c.seabreeze_diag(5400.0, 1, p, u, v, th, cdist, st.z, st.sigma, *state, halo=0, bnd=hip.SB_BND_GLOBAL)
        assert c.guard_report() == dict(bad_cells=0, repaired_cells=0, calls_with_bad=0, calls=1)
    finally:
        for cc in ctxs.values():
            cc.close()
