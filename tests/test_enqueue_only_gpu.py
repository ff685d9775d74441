"""The `_dev` entry points on a caller's BUSY stream (include/seabreeze_hip.h: they "enqueue on `stream` ... without
synchronising"), as a GPU-resident host model, BandRunner and bench.py use them: whole sequences of calls enqueued behind
device work of the caller's, no host synchronisation before the end (tests/enqueue_harness.py has the layout of a step and
why stale step inputs show a mis-ordered operation).

Held for every sequence:
  - every step against the CPU oracle run on the same sequence -- fp64: test_parity_gpu._assert_close64 (1e-7 relative, floor
    1e-9); fp32: oracle/fp32_criterion.py against the fp64 oracle on the fp32-representable inputs;
  - bit for bit the same sequence in a fresh context with everything synchronised after every call;
  - steady-state calls (the second and later call of one geometry on one context) return while the filler enqueued ahead
    of them is still running: no hidden synchronisation.  Exempt, as the header says: the first call of a context or of a
    geometry (allocations), sb_get_dist_*_dev with new coordinates or on another stream than the one that uploaded them;
  - the run is not vacuous: the filler ran at least 20 times as long as the host needed to enqueue a step (both printed).

Eight steps of 5400 s: steps 4 and 8 take the six-hourly branch that stores the winds.  Grids: 200 x 96 x 3 with a distance
window of 5 cells (tests/test_launch_sequence_gpu.py) and 256 x 192 x 2 with one of 27 (tests/test_strip32_gpu._case) where
radii beyond 16 are needed.
"""
import numpy as np
import pytest
import torch

import enqueue_harness as eh
from conftest import relerr
from oracle import fp32_criterion as crit
from seabreeze_param_amd import hip, synth
from test_nonfinite_guard_gpu import _close64, _pattern
from test_parity_gpu import _assert_close64
from test_setup_gpu import _check_dist
from test_strip32_gpu import _case as _wide_case

pytestmark = pytest.mark.gpu

NSTEPS, DT_S, KWIN = 8, 5400.0, 5
TNS = list(range(1, NSTEPS + 1))
NAMES = ("ws", "wd", "thc", "sb_con")
f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


# ---- fixtures: streams, the filler, the grids, the oracle's answers (computed once, never modified) ----------------------

@pytest.fixture(scope="module")
def streams():
    return [torch.cuda.Stream(), torch.cuda.Stream()]


@pytest.fixture(scope="module")
def filler():
    return eh.Filler()


@pytest.fixture(scope="module")
def grids(oracles):
    """(grid, dtype) -> static fields, coast distance, nz"""
    out = {}
    for dt in (np.float64, np.float32):
        st = synth.static_fields(200, 96, dt)
        coast = oracles[8].get_edges(f8(st.landfrac), f8(st.icefrac))
        cd = oracles[8].get_dist(coast, f8(st.landfrac), st.lon, st.lat, maxdist=900.0, kwin=KWIN)
        cd[np.abs(cd) > 180.0] = 12000.0
        out["200x96", dt] = (st, cd.astype(dt), 3)
        out["256x192", dt] = _wide_case(oracles[8], 256, 192, 27, dt) + (2,)
    for (nx, ny), k in (((96, 72), 4), ((130, 75), 4)):          # test_alternating_grids_and_contrast_kernels_in_one_context
        st = synth.static_fields(nx, ny, np.float64)
        coast = oracles[8].get_edges(st.landfrac, st.icefrac, rule=1, bnd=1)
        cd = oracles[8].get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=180.0, kwin=k)
        cd[np.abs(cd) > 180.0] = 12000.0
        out[f"{nx}x{ny}", np.float64] = (st, cd, 2)
    return out


def _case(grids, kind, grid, dt, halo=0, hint=None, setup=None, poison=None, tns=TNS):
    """poison = (step index, y, x, value): that cell of theta at that step only"""
    st, cd, nz = grids[grid, dt]
    ny, nx = cd.shape
    theta = [synth.theta_step(st, tn, dt) for tn in tns]
    if poison is not None:
        k, y, x, val = poison
        theta[k] = theta[k].copy()
        theta[k][y, x] = val
    uv = [synth.wind_step(st, nz, tn, dt) for tn in tns]
    p = synth.pressure_1d(nz, dt) if kind == "f2py" else synth.pressure_3d(st, nz, dt)
    fr = (lambda a: eh.frame(a, halo, dt)) if kind == "band" else (lambda a: a)
    beyond = max(tns) + 1
    stale = (fr(synth.theta_step(st, beyond, dt)),) + synth.wind_step(st, nz, beyond, dt)
    return eh.Case(kind=kind, dt=dt, nx=nx, ny=ny, nz=nz, p=p, mask=fr(cd), z=fr(st.z), sigma=fr(st.sigma),
                   theta=[fr(t) for t in theta], u=[a for a, _ in uv], v=[b for _, b in uv], tns=list(tns), stale=stale, halo=halo,
                   timestep=DT_S, setup=setup, hint=hint,
                   extra=dict(key=("f2py" if kind == "f2py" else "generic", grid, np.dtype(dt).name, poison, tuple(tns)),
                              st=st, cd=cd, theta=theta))


_ORACLE, _ORACLE_NN = {}, {}


def _oracle(oracles, case):
    """The fp64 oracle on the case's own (for fp32: fp32-representable) inputs, step by step; a band step owning the globe
    is the single-domain call.  -> per step [ws, wd, thc, sb_con] (f2py: [ws, wd, thc, output])"""
    key = case.extra["key"]
    if key not in _ORACLE:
        orc, st, cd = oracles[8], case.extra["st"], case.extra["cd"]
        out = []
        if key[0] == "generic":
            p3 = synth.pressure_3d(st, case.nz, case.dt)
            so = [np.zeros((case.ny, case.nx)) for _ in range(4)]
            for k, tn in enumerate(case.tns):
                orc.seabreeze_diag(DT_S, tn, f8(p3), f8(case.u[k]), f8(case.v[k]), f8(case.extra["theta"][k]), f8(cd), f8(st.z),
                                   f8(st.sigma), *so, halo=0, bnd=1)
                out.append([a.copy() for a in so])
        else:
            wo = [np.zeros((case.ny, case.nx)) for _ in range(3)]
            for k, tn in enumerate(case.tns):
                oo = orc.diag(tn, f8(case.p), f8(st.z), f8(st.sigma), f8(case.extra["theta"][k]), f8(case.v[k]), f8(case.u[k]), f8(cd),
                              *wo, timestep=DT_S / 60.0)
                out.append([a.copy() for a in wo] + [oo.copy()])
        for step in out:
            for a in step:
                a.setflags(write=False)
        _ORACLE[key], _ORACLE_NN[key] = out, orc.last_nn_max
    return _ORACLE[key]


def _hold_counters(case, cnt, twin_cnt, what):
    """sb_last_counters behind the sequence's last call: the synchronised twin's, and the largest radius the oracle's search
    used.  The counters are read from the block-flag buffers: flags that an earlier call of another geometry left standing,
    because the buffers were not zeroed in stream order, show here even where they change no result."""
    assert cnt == twin_cnt, (what, cnt, twin_cnt)
    assert cnt["max_radius"] == _ORACLE_NN[case.extra["key"]], (what, cnt, _ORACLE_NN[case.extra["key"]])
    if case.kind != "band":                              # (a band's count is its frame's)
        rows = case.ny - 1 if case.kind == "f2py" else case.ny
        assert cnt["band_cells"] == int((np.abs(f8(case.extra["cd"]))[:rows] <= 180.0).sum()), (what, cnt)


# ---- what is held ---------------------------------------------------------------------------------------------------------

def _hold_oracle(case, got, ref, what, nonfinite=False):
    band = np.abs(f8(case.extra["cd"])) <= 180.0
    fp64 = np.dtype(case.dt) == np.float64
    zeros = lambda dt: [np.zeros((case.ny, case.nx), dt) for _ in range(4)]
    if case.kind != "f2py":
        if fp64:
            for k, (g, r) in enumerate(zip(got, ref)):
                for nm, a, b in zip(NAMES, g, r):
                    if nonfinite:                          # (as tests/test_nonfinite_guard_gpu.py holds such input)
                        _pattern(a, b, f"{what} step {k + 1} {nm}")
                        _close64(a, b, f"{what} step {k + 1} {nm}")
                    else:
                        _assert_close64(a, b, f"{what} step {k + 1} {nm}")
            return
        per, gp, op = [], zeros(case.dt), zeros(np.float64)
        for k, (g, r) in enumerate(zip(got, ref)):
            per.append(crit.check_step(case.tns[k], gp, g, op, r, band, timestep=DT_S))
            gp, op = g, r
        res = crit.merge(per)
        assert res["ok"] and res["cells_compared"] > 0, (what, res)
        return
    # the f2py flavour: rows 1 .. nlats - 1; output = sb_con, t0, this step's wind speed and direction
    rows = slice(0, case.ny - 1)
    if fp64:
        for k, (g, r) in enumerate(zip(got, ref)):
            for nm, a, b in zip(NAMES[:3], g, r):
                _assert_close64(a, b, f"{what} step {k + 1} state {nm}")
            for j, nm in enumerate(("sb_con", "t0", "windspeed", "winddir")):
                _assert_close64(g[3][j, rows], r[3][j, rows], f"{what} step {k + 1} output {nm}")
        return
    # fp32.  The flavour stores a step's winds only on the first step and every six hours (ref :268-273; the planes 2, 3 of
    # `output` are that state), so this step's wind speed, which the criterion's mean wind speed needs (ref :243: 0.5 (state
    # before + this step's)), is not among the results.  It follows from the inputs alone: sqrt(u^2 + v^2) at the level
    # nearest 700 hPa -- in double precision for the oracle's side, in single precision for the device's (what k_wind
    # computes up to rounding, which the criterion's own allowance of 2 u 11 m/s on the mean covers).  The winds the device
    # did store are held against the oracle's state below; thc and sb_con are the device's.
    band = band.copy()
    band[case.ny - 1] = False
    lev = int(np.argmin(np.abs(f8(case.p) - 70000.0)))
    per, gp, op = [], zeros(case.dt), zeros(np.float64)
    for k, (g, r) in enumerate(zip(got, ref)):
        u4, v4 = case.u[k][lev], case.v[k][lev]
        u8, v8 = f8(u4), f8(v4)
        gn = [np.sqrt(u4 * u4 + v4 * v4), np.degrees(np.arctan2(-u4, -v4)), g[2], g[3][0]]
        on = [np.sqrt(u8 * u8 + v8 * v8), np.degrees(np.arctan2(-u8, -v8)), r[2], r[3][0]]
        per.append(crit.check_step(case.tns[k], gp, gn, op, on, band, n_wd_o=on[1], timestep=DT_S))
        assert relerr(g[3][1][rows], r[3][1][rows], floor=1.0) < 2e-6, f"{what} step {k + 1} t0"      # (test_strip32_gpu.py)
        for j, tol in ((0, "windspeed_rel"), (1, "winddir_abs_deg")):                                   # the carried winds
            d = np.abs(f8(g[j]) - r[j])[band]
            d = d / np.maximum(np.abs(r[j][band]), 1e-2) if j == 0 else np.minimum(d, 360.0 - d)
            assert d.max() <= crit.TOL[tol], f"{what} step {k + 1} state {NAMES[j]}: {d.max()}"
        gp, op = [g[0], g[1], g[2], g[3][0]], [r[0], r[1], r[2], r[3][0]]
    res = crit.merge(per)
    assert res["ok"] and res["cells_compared"] > 0, (what, res)


def _hold_twin(got, twin, what):
    for k, (g, t) in enumerate(zip(got, twin)):
        for i, (a, b) in enumerate(zip(g, t)):
            assert eh.same_bits(a, b), (f"{what} step {k + 1} array {i}: {int((a != b).sum())} cells differ from the run that "
                                        "synchronised after every call")


def _run_variant(oracles, filler, streams, case, what, nonfinite=False):
    """one fresh context enqueue-only, another one synchronised; the oracle, the twin, then what the run showed of itself"""
    ref = _oracle(oracles, case)
    ctx = hip.Context(0)
    try:
        got, q = eh.run_enqueued(ctx, case, NSTEPS, streams[0], filler, what=what, check=False)
        cnt = ctx.last_counters()
    finally:
        ctx.close()
    ctx = hip.Context(0)
    try:
        twin = eh.run_synchronised(ctx, case, streams[0])
        twin_cnt = ctx.last_counters()
    finally:
        ctx.close()
    _hold_oracle(case, got, ref, what, nonfinite)
    _hold_twin(got, twin, what)
    _hold_counters(case, cnt, twin_cnt, what)
    q.check_busy(what)


def _switches(hint=None, **kw):
    """setup(ctx): Context.set_<name>(value) for every keyword, in order, and the radius hint"""
    def setup(ctx):
        if hint is not None:
            ctx.set_search_radius_hint(hint)
        for name, val in kw.items():
            getattr(ctx, "set_" + name)(val)
    return setup


# ---- 0: the harness sees a call on the wrong stream --------------------------------------------------------------------------

def test_harness_detects_a_call_on_another_stream(oracles, filler, streams, grids):
    """The one deliberately mis-ordered run: filler, input copies and snapshots on s, the library call on a second side
    stream, which does not wait for s.  From step 2 on the call reads theta of the step before (the copy sits behind the
    filler) and thc is not the oracle's; every value involved is valid and finite."""
    case = _case(grids, "generic", "200x96", np.float64, setup=_switches(hint=6))
    ref = _oracle(oracles, case)
    ctx = hip.Context(0)
    try:
        got, q = eh.run_enqueued(ctx, case, NSTEPS, streams[0], filler, call_stream=streams[1], what="self-check", check=False)
    finally:
        ctx.close()
    q.check_busy("self-check", assert_no_sync=False)
    for k in range(1, NSTEPS):
        e = relerr(got[k][2], ref[k][2], floor=1e-2)
        print(f"[enqueue-only] self-check step {k + 1}: thc differs from the oracle by {e:.3g} relative")
        assert e > 1e-7, f"step {k + 1}: a call on another stream went unnoticed"
    for g, r in zip(got, ref):
        for a, b in zip(g, r):
            assert np.isfinite(a[np.isfinite(b)]).all()


# ---- 1: the host-model flavour ----------------------------------------------------------------------------------------------

HOST_MODEL = {
    "fp64-strip-fold": ("200x96", np.float64, dict(hint=6, fold=True)),
    "fp64-strip-kprep": ("200x96", np.float64, dict(hint=6, fold=False)),
    "fp64-tiles": ("200x96", np.float64, dict(hint=24)),
    "fp32-strip32": ("256x192", np.float32, dict(hint=30)),
    "fp32-tiles": ("256x192", np.float32, dict(hint=30, wide_strip=False)),
    "fp64-replan": ("200x96", np.float64, dict(hint=6, plan_cache=False)),
    # 2: the opt-in paths on the same sequence
    "table": ("200x96", np.float64, dict(hint=6, table_contrast=True)),
    "table-window-cache": ("200x96", np.float64, dict(hint=6, table_contrast=True, table_window_cache=True)),
    "guard-clean": ("200x96", np.float64, dict(hint=6, nonfinite_guard=True)),
}


@pytest.mark.parametrize("variant", list(HOST_MODEL))
def test_host_model_flavour(oracles, filler, streams, grids, variant):
    """sb_seabreeze_diag_*_dev, SB_BND_GLOBAL, a fresh context: its very first call, allocations and memsets included, is
    enqueued behind a busy stream."""
    grid, dt, sw = HOST_MODEL[variant]
    _run_variant(oracles, filler, streams, _case(grids, "generic", grid, dt, setup=_switches(**sw)), variant)


def test_guard_with_a_missing_value_in_flight(oracles, filler, streams, grids):
    """sb_set_nonfinite_guard with one 2e20 cell of theta at step 3 only, on a band cell; the oracle is handed the same."""
    _, cd, _ = grids["200x96", np.float64]
    cells = np.argwhere(np.abs(cd) <= 180.0)
    y, x = (int(i) for i in cells[len(cells) // 2])
    case = _case(grids, "generic", "200x96", np.float64, setup=_switches(hint=6, nonfinite_guard=True), poison=(2, y, x, 2.0e20))
    _run_variant(oracles, filler, streams, case, "guard-2e20", nonfinite=True)


# ---- 3: the f2py flavour ------------------------------------------------------------------------------------------------------

F2PY = {
    "fp64": (np.float64, dict(hint=6)),
    "fp32": (np.float32, dict(hint=6)),
    "fp64-table": (np.float64, dict(hint=6, table_contrast=True, table_contrast_f2py=True)),
}


@pytest.mark.parametrize("variant", list(F2PY))
def test_f2py_flavour(oracles, filler, streams, grids, variant):
    """sb_diag_*_dev with a 1-D p: the four planes of `output` (rows 1 .. nlats - 1) and the three state arrays."""
    dt, sw = F2PY[variant]
    _run_variant(oracles, filler, streams, _case(grids, "f2py", "200x96", dt, setup=_switches(**sw)), "f2py-" + variant)


# ---- 4: the band step -----------------------------------------------------------------------------------------------------------

BAND = {
    "fp32-strip32-h30": ("256x192", np.float32, 30, dict(hint=30)),                  # exchange_rows on the second stream
    "fp64-strip-h16": ("200x96", np.float64, 16, dict(hint=16)),
    "fp64-tiles-h24": ("200x96", np.float64, 24, dict(hint=24)),                     # the whole swap_bounds on the second stream
    "fp64-table-bands": ("200x96", np.float64, 16, dict(hint=16, table_contrast=True, table_contrast_bands=True)),
    "fp64-guard-bands": ("200x96", np.float64, 16, dict(hint=16, nonfinite_guard=True, nonfinite_guard_bands=True)),
    "fp64-static-sigma": ("200x96", np.float64, 16, dict(hint=16, static_sigma=True)),
}


@pytest.mark.parametrize("variant", list(BAND))
def test_band_step(oracles, filler, streams, grids, variant):
    """sb_band_seabreeze_diag_*_dev on a one-rank context owning the globe.  The statics' ghost cells are filled once by
    sb_swap_bounds_*_dev, enqueued on s ahead of the first step and not waited for.  The next step's input copy rewrites
    the WHOLE frame of theta, ghost cells included, right behind the call: a branch on the context's second stream that was
    not joined back would read -- or have its ghost fill overwritten by -- that rewrite."""
    grid, dt, halo, sw = BAND[variant]
    _run_variant(oracles, filler, streams, _case(grids, "band", grid, dt, halo=halo, setup=_switches(**sw)), "band-" + variant)


# ---- 5: setup feeding the calls -------------------------------------------------------------------------------------------------

def _setup_chain(ctx, grids, streams, filler, sync_each):
    """get_edges -> get_dist -> 2 x diag -> sigmoid on another field -> 2 x diag, all on s; then get_dist once more with the
    same coordinates on the other side stream (ordered behind get_edges by an event)"""
    dt = np.float64
    st, _, nz = grids["200x96", dt]
    nx, ny = st.nx, st.ny
    s, s2 = streams
    case = _case(grids, "generic", "200x96", dt, setup=_switches(hint=6), tns=[1, 2, 3, 4])
    q = eh.Sequence(ctx, case, s, filler=filler, sync_each=sync_each)
    q.upload()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    lsm, ci, other = up(st.landfrac), up(st.icefrac), up(st.z * 3.0 + 11.0)
    coast, cdist, cdist2, sm = (torch.zeros((ny, nx), dtype=torch.float64, device="cuda") for _ in range(4))
    q.mask = cdist                                       # the calls read the distance field enqueued just ahead of them
    ev_edges = torch.cuda.Event()
    torch.cuda.synchronize()

    def step(fn):
        fn()
        if sync_each:
            s.synchronize()
            s2.synchronize()

    with torch.cuda.stream(s):
        if filler is not None:
            filler.enqueue()
        step(lambda: ctx.get_edges_dev(dt, nx, ny, lsm.data_ptr(), ci.data_ptr(), coast.data_ptr(), rule=1, bnd=hip.SB_BND_GLOBAL,
                                       stream=s.cuda_stream))
        ev_edges.record(s)
        step(lambda: ctx.get_dist_dev(dt, nx, ny, coast.data_ptr(), lsm.data_ptr(), st.lon, st.lat, cdist.data_ptr(), maxdist=180.0,
                                      kwin=KWIN, stream=s.cuda_stream))
    q.enqueue_step(0)
    q.enqueue_step(1)
    step(lambda: ctx.sigmoid_dev(dt, nx, ny, other.data_ptr(), sm.data_ptr(), stream=s.cuda_stream))     # the shared statistics scratch
    q.enqueue_step(2)
    q.enqueue_step(3)
    s2.wait_event(ev_edges)
    step(lambda: ctx.get_dist_dev(dt, nx, ny, coast.data_ptr(), lsm.data_ptr(), st.lon, st.lat, cdist2.data_ptr(), maxdist=180.0,
                                  kwin=KWIN, stream=s2.cuda_stream))
    s.synchronize()
    s2.synchronize()
    return dict(coast=coast.cpu().numpy(), cdist=cdist.cpu().numpy(), cdist2=cdist2.cpu().numpy(), sm=sm.cpu().numpy(),
                steps=q.collect(), other=other.cpu().numpy()), q, case


def test_setup_feeding_the_calls(oracles, filler, streams, grids):
    """One stream, nothing waited for: the coastline, the coast distance made from it and four diag steps that read that
    distance field, with a stand-alone sigmoid (it shares the statistics scratch, tests/test_comm_gpu.py) between steps 2 and
    3.  The second get_dist, same coordinates, on ANOTHER stream than the one its coordinate tables were uploaded on, waits
    for that stream once (include/seabreeze_hip.h) and gives the same field bit for bit."""
    orc = oracles[8]
    st, _, nz = grids["200x96", np.float64]
    ctx = hip.Context(0)
    try:
        got, q, case = _setup_chain(ctx, grids, streams, filler, False)
    finally:
        ctx.close()
    ctx = hip.Context(0)
    try:
        twin, _, _ = _setup_chain(ctx, grids, streams, None, True)
    finally:
        ctx.close()
    q.report("setup chain")
    coast = orc.get_edges(st.landfrac, st.icefrac, rule=1, bnd=1)
    assert np.array_equal(got["coast"], coast)
    _check_dist(got["cdist"], orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=180.0, kwin=KWIN), "cdist", 1e-12)
    assert eh.same_bits(got["cdist2"], got["cdist"]), "get_dist on the second stream"
    _assert_close64(got["sm"], orc.sigmoid(got["other"]), "sigmoid")
    so = [np.zeros((st.ny, st.nx)) for _ in range(4)]
    p3 = synth.pressure_3d(st, nz, np.float64)
    for k, tn in enumerate(case.tns):                    # the oracle on the distance field the calls were handed
        orc.seabreeze_diag(DT_S, tn, p3, case.u[k], case.v[k], case.theta[k], got["cdist"], st.z, st.sigma, *so, halo=0, bnd=1)
        for nm, a, b in zip(NAMES, got["steps"][k], so):
            _assert_close64(a, b, f"setup chain step {tn} {nm}")
    for nm in ("coast", "cdist", "cdist2", "sm"):
        assert eh.same_bits(got[nm], twin[nm]), nm
    _hold_twin(got["steps"], twin["steps"], "setup chain")
    q.check_busy("setup chain")


# ---- 6: geometry changes in flight ------------------------------------------------------------------------------------------------

def _alternating(ctx, cases, order, stream, filler, sync_each):
    seqs = [eh.Sequence(ctx, c, stream, filler=filler, sync_each=sync_each) for c in cases]
    return eh.run_interleaved(seqs, order), seqs


@pytest.mark.parametrize("third", [False, True], ids=["two-grids", "third-grid-at-call-7"])
def test_geometry_changes_in_flight(oracles, filler, streams, grids, third):
    """Commit 38de1a5's scenario without a single host synchronisation: twenty calls on one context that alternate between
    96 x 72 on the strip kernel (hint 16) and 130 x 75 on the tile kernel (hint 24) -- every switch re-sizes and zeroes the
    block-flag buffers --, and again with 256 x 192 (tile kernel, halo 32) entering at call 7, so that every scratch buffer
    grows while earlier calls are still queued.  A call that reallocates synchronises (hipFree): the no-synchronisation
    assertion is off, the stream must still have been busy ahead of every call, and every number must be right."""
    names = [("96x72", 16), ("130x75", 24)] + ([("256x192", 30)] if third else [])
    order, nsteps = [], [0] * len(names)
    for call in range(20):
        i = call % 2 if (not third or call < 6) else (2, 0, 1)[(call - 6) % 3]
        order.append((i, nsteps[i]))
        nsteps[i] += 1
    cases = [_case(grids, "generic", g, np.float64, hint=h, tns=list(range(1, n + 1))) for (g, h), n in zip(names, nsteps)]
    refs = [_oracle(oracles, c) for c in cases]
    ctx = hip.Context(0)
    try:
        got, seqs = _alternating(ctx, cases, order, streams[0], filler, False)
        cnt = ctx.last_counters()
    finally:
        ctx.close()
    ctx = hip.Context(0)
    try:
        twin, _ = _alternating(ctx, cases, order, streams[0], None, True)
        twin_cnt = ctx.last_counters()
    finally:
        ctx.close()
    times = [seqs[i].t_enqueue[k] for i, k in order]
    enqueue_s = float(np.median(times[3:]))
    print(f"[enqueue-only] geometry changes ({len(names)} grids): filler {filler.ms:.2f} ms per call, host enqueue {1e3 * enqueue_s:.3f} ms "
          f"per call (median), slowest {1e3 * max(times):.3f} ms")
    for c, g, r, t in zip(cases, got, refs, twin):
        _hold_oracle(c, g, r, f"{c.nx}x{c.ny}")
        _hold_twin(g, t, f"{c.nx}x{c.ny}")
    _hold_counters(cases[order[-1][0]], cnt, twin_cnt, "the last call's counters")
    idle = [(i, k) for i, k in order if not seqs[i].pending_before[k]]
    if idle:
        raise eh.VacuousRun(f"the filler had finished before the calls {idle} were made")
    eh.check_ratio(filler, enqueue_s, "geometry changes")


# ---- 7: two contexts, two streams ---------------------------------------------------------------------------------------------------

def test_two_contexts_interleaved(oracles, filler, streams, grids):
    """A1 B1 A2 B2 ...: context A on 200 x 96 fp64, context B on 256 x 192 fp32 (k_strip32), each behind its own filler on its
    own stream, one synchronisation at the end.  The kernels hold no spin waits on other workgroups, so running them side
    by side is safe; each sequence is its oracle's and its synchronised twin's: the contexts share no state."""
    cases = [_case(grids, "generic", "200x96", np.float64, setup=_switches(hint=6)),
             _case(grids, "generic", "256x192", np.float32, setup=_switches(hint=30))]
    refs = [_oracle(oracles, c) for c in cases]
    fillers = [filler, eh.Filler()]
    order = [(i, k) for k in range(NSTEPS) for i in (0, 1)]
    ctxs = [hip.Context(0), hip.Context(0)]
    try:
        seqs = [eh.Sequence(ctxs[i], cases[i], streams[i], filler=fillers[i]) for i in (0, 1)]
        got = eh.run_interleaved(seqs, order)
    finally:
        for c in ctxs:
            c.close()
    twins = []
    for c in cases:
        ctx = hip.Context(0)
        try:
            twins.append(eh.run_synchronised(ctx, c, streams[0]))
        finally:
            ctx.close()
    for i, nm in enumerate(("A", "B")):
        seqs[i].report(f"two contexts, {nm}")
        _hold_oracle(cases[i], got[i], refs[i], nm)
        _hold_twin(got[i], twins[i], nm)
    for i, nm in enumerate(("A", "B")):
        seqs[i].check_busy(f"two contexts, {nm}")


# ---- 8: stream = NULL -----------------------------------------------------------------------------------------------------------------

def test_null_stream_is_the_contexts_own(oracles, grids):
    """The rule (include/seabreeze_hip.h): stream = NULL means the CONTEXT'S OWN stream -- a non-blocking one, which neither
    waits for nor is waited for by the legacy default stream --, not stream 0.  So a caller that passes NULL orders its own
    work against the calls through the context: inputs go in with sb_device_upload and results come out with
    sb_device_download, both of which run on that stream (and wait for it), and the sequence ends with sb_synchronize.
    Nothing here synchronises the device or touches the default stream between the first call and the end; were NULL the
    legacy stream, the downloads would not be ordered behind the kernels."""
    case = _case(grids, "generic", "200x96", np.float64)
    ref = _oracle(oracles, case)
    tdev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p, mask, z, sigma = (tdev(a) for a in (case.p, case.mask, case.z, case.sigma))
    theta, u, v = (torch.zeros_like(tdev(a)) for a in (case.theta[0], case.u[0], case.v[0]))
    state = [torch.zeros((case.ny, case.nx), dtype=torch.float64, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()                             # torch's uploads have landed: from here on the context's stream alone
    ctx = hip.Context(0)
    try:
        ctx.set_search_radius_hint(6)
        got = []
        for k, tn in enumerate(case.tns):
            for dst, src in ((theta, case.theta[k]), (u, case.u[k]), (v, case.v[k])):
                ctx.device_upload(dst.data_ptr(), src)
            ctx.seabreeze_diag_dev(case.dt, DT_S, tn, case.nx, case.ny, case.nz, 0, hip.SB_BND_GLOBAL, p.data_ptr(), u.data_ptr(),
                                   v.data_ptr(), theta.data_ptr(), mask.data_ptr(), z.data_ptr(), sigma.data_ptr(),
                                   *[s.data_ptr() for s in state], stream=None)
            got.append([ctx.device_download(np.empty((case.ny, case.nx)), s.data_ptr()) for s in state])
        ctx.synchronize()
    finally:
        ctx.close()
    _hold_oracle(case, got, ref, "stream=None")
