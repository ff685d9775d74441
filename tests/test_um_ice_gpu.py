"""A UM-layout coast that moves with the sea ice (sb_um_coast_open_*, sb_um_ice_*[_dev], sb_um_ice_report, sb_um_coast_close;
include/seabreeze_hip.h).  The twelve ice planes of tests/um_ice_cases.py -- tests/test_um_ice_cases.py shows on the CPU what
each of them does -- go in order through one open coast; cdist's frame carries a sentinel that only the interior may lose.

After every plane the interior must equal

* sb_get_edges_um_*_dev + sb_get_dist_um_win_*_dev of that plane on a second context, BIT FOR BIT;
* the numpy restatement (tests/um_setup_ref.py, tests/um_win_ref.py) within the project's bounds for it: 12000-cells and
  signs identical, distances to 1e-12 (fp64) / 2e-6 (fp32) relative with denominator max(|o|, 1);

and the report must lie between the brute-force count and the cap of tests/um_ice_ref.py.  Then: only marked workgroups are
written, other coast calls on the context in between, seabreeze_diag_um steps with ice calls between them against a twin
whose mask is made afresh, an enqueue-only run behind device work on a caller's stream, the host form, the refusals.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import enqueue_harness as eh
import um_ice_cases as uic
import um_ice_ref as uir
import um_setup_ref as ur
import um_win_ref as uw
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

SENTINEL = uw.SENTINEL
REL = {8: 1e-12, 4: 2e-6}
SET = {s[0]: s for s in uic.SETS}


def _dt(prec):
    return np.float64 if prec == 8 else np.float32


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # (a copy: the cached inputs are read-only)


def _inner(f, halo, nx, ny):
    return f[halo[1]:halo[1] + ny, halo[0]:halo[0] + nx]


def _ghosts_keep(frame, halo, nx, ny, value=SENTINEL):
    g = np.ones(frame.shape, bool)
    _inner(g, halo, nx, ny)[...] = False
    return bool((frame[g] == value).all())


@functools.lru_cache(maxsize=None)
def _inputs(name, prec):
    """land, lf_l, planes, the reference coast of every plane (interior) -- once per set and precision"""
    _, nx, ny, win, halo, maxdist, kern = SET[name]
    land, lf_l, planes = uic.make(nx, ny, halo, _dt(prec))
    co = [np.ascontiguousarray(_inner(ur.edges_um(lf_l, ci, *halo), halo, nx, ny)) for ci in planes]
    for a in [land, lf_l] + planes + co:
        a.setflags(write=False)
    return land, lf_l, planes, co


class _Coast:
    """one open coast on one context: resident frames of landfrac, icefrac and cdist on the device"""

    def __init__(self, ctx, cset, lat, lon, lf_l, incremental=True):
        _, self.nx, self.ny, self.win, self.halo, self.maxdist, _ = cset
        self.ctx, self.dt = ctx, lf_l.dtype
        self.lf = _dev(lf_l)
        self.ci = torch.zeros_like(self.lf)
        self.cd = torch.full_like(self.lf, SENTINEL)
        ctx.um_coast_open(self.dt, self.nx, self.ny, *self.halo, *self.win, lat, lon, maxdist=self.maxdist, incremental=incremental)
        torch.cuda.synchronize()

    def ice(self, ci_l, stream=None):
        """-> cdist's frame, the report"""
        self.ci.copy_(_dev(ci_l))
        torch.cuda.synchronize()
        self.ctx.um_ice_dev(self.dt, self.lf.data_ptr(), self.ci.data_ptr(), self.cd.data_ptr(), stream=stream)
        rep = self.ctx.um_ice_report()                            # (synchronises)
        return self.cd.cpu().numpy(), rep

    def close(self):
        self.ctx.um_coast_close()


def _twin(ctx, cset, lat, lon, land, lf_l, ci_l):
    """get_edges_um_dev + get_dist_um_win_dev of one plane -> the interior"""
    _, nx, ny, win, halo, maxdist, _ = cset
    dt = lf_l.dtype
    dl, dc, dlf, dla, dlo = (_dev(a) for a in (lf_l, ci_l, land, lat, lon))
    co, cd = torch.zeros_like(dl), torch.zeros_like(dl)
    torch.cuda.synchronize()
    ctx.get_edges_um_dev(dt, nx, ny, *halo, dl.data_ptr(), dc.data_ptr(), co.data_ptr())
    ctx.get_dist_um_win_dev(dt, nx, ny, *halo, *win, co.data_ptr(), dlf.data_ptr(), dla.data_ptr(), dlo.data_ptr(), cd.data_ptr(),
                            maxdist=maxdist)
    ctx.synchronize()
    return np.ascontiguousarray(_inner(cd.cpu().numpy(), halo, nx, ny))


@pytest.fixture(scope="module")
def twinctx():
    c = hip.Context()
    yield c
    c.close()


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("grid", uic.GRIDS)
@pytest.mark.parametrize("name", [s[0] for s in uic.SETS])
def test_um_cdist_follows_every_plane(hipctx, twinctx, name, grid, prec):
    cset = SET[name]
    _, nx, ny, win, halo, maxdist, kern = cset
    assert uic.kernel_of(win, halo) == kern
    dt = _dt(prec)
    lat, lon = ur.grid_named(grid, nx, ny, dt)
    land, lf_l, planes, co = _inputs(name, prec)
    tiles = uir.groups(ny) * uir.tiles(nx)

    # ---- the numpy restatement, once per distinct coast
    ref, refs = [], {}
    for n in range(12):
        key = co[n].tobytes()
        if key not in refs:
            coast_l = np.ascontiguousarray(np.pad(co[n], ((halo[1], halo[1]), (halo[0], halo[0]))))
            refs[key] = _inner(uw.dist_win_literal(coast_l, land, lat, lon, *halo, *win, maxdist), halo, nx, ny)
        ref.append(refs[key])
    if name == "f":                                               # the reset fires: reached by the plain minimum, 12000 in the field
        coast_l = np.ascontiguousarray(np.pad(co[7], ((halo[1], halo[1]), (halo[0], halo[0]))))
        plain = _inner(uw.dist_win(ur.dist_um_vectorised, coast_l, land, lat, lon, *halo, *win, 1.0e30), halo, nx, ny)
        assert ((np.abs(plain) < 12000.0) & (ref[7] >= 12000.0)).any(), "no reset cell"

    want = []
    for inc in (True, False):
        b = _Coast(hipctx, cset, lat, lon, lf_l, incremental=inc)
        try:
            changed_calls = 0
            for n, ci in enumerate(planes):
                if inc:
                    want.append(_twin(twinctx, cset, lat, lon, land, lf_l, ci))
                frame, rep = b.ice(ci)
                what = f"{name} {grid} fp{8 * prec} plane {uic.PLANES[n]} inc {int(inc)}"
                print(what, rep)
                assert _ghosts_keep(frame, halo, nx, ny), f"{what}: ghost cells of cdist were written"
                got = np.ascontiguousarray(_inner(frame, halo, nx, ny))
                assert eh.same_bits(got, want[n]), (what, f"{int((got != want[n]).sum())} cells differ from get_edges_um + get_dist_um_win")
                if inc:
                    uw.check_dist(got, ref[n], what, REL[prec])
                assert rep["calls"] == n + 1 and rep["tiles"] == tiles
                if not inc:
                    assert rep["changed_calls"] == -1 and rep["tiles_marked"] == tiles
                    continue
                if n == 0:
                    assert rep["tiles_marked"] == tiles and rep["changed_calls"] == 0      # the first call computes everything
                    continue
                changed = uir.changed_cells(co[n], co[n - 1])
                changed_calls += 1 if changed else 0
                assert rep["changed_calls"] == changed_calls, what
                lo = int(uir.brute_marks(nx, ny, *win, changed).sum())
                cap = int(uir.cap_marks(nx, ny, *win, changed).sum())
                assert lo <= rep["tiles_marked"] <= cap, (what, lo, rep["tiles_marked"], cap)
                assert rep["tiles_marked"] == int(uir.word_marks(nx, ny, *win, changed).sum()), what
                if n in uic.UNCHANGED:
                    assert rep["tiles_marked"] == 0 and not changed
                else:
                    assert rep["tiles_marked"] > 0
        finally:
            b.close()


def test_only_marked_workgroups_are_written(hipctx, twinctx):
    """Set c.  After the first call the test overwrites the interior of cdist with a sentinel -- the one deliberate breach of
    the contract -- and runs case 4: the sentinel must stand exactly outside the workgroups the model says case 4 marks, and
    every marked workgroup must hold the field of get_edges_um + get_dist_um_win."""
    cset, prec, grid = SET["c"], 8, "dateline"
    _, nx, ny, win, halo, maxdist, _ = cset
    lat, lon = ur.grid_named(grid, nx, ny, _dt(prec))
    land, lf_l, planes, co = _inputs("c", prec)
    marked = uir.cells_of_marks(uir.word_marks(nx, ny, *win, uir.changed_cells(co[3], co[2])), nx, ny)
    assert marked.any() and not marked.all()
    want = _twin(twinctx, cset, lat, lon, land, lf_l, planes[3])
    b = _Coast(hipctx, cset, lat, lon, lf_l)
    try:
        b.ice(planes[2])
        _inner(b.cd, halo, nx, ny).fill_(-3.25)
        torch.cuda.synchronize()
        frame, rep = b.ice(planes[3])
        got = _inner(frame, halo, nx, ny)
        assert rep["tiles_marked"] * uir.ROWS * uir.COLS >= marked.sum() > 0
        assert (got[~marked] == -3.25).all(), f"{int((got[~marked] != -3.25).sum())} cells outside the marked workgroups were written"
        assert eh.same_bits(np.ascontiguousarray(got[marked]), np.ascontiguousarray(want[marked])), "a marked workgroup does not hold the field"
        assert _ghosts_keep(frame, halo, nx, ny)
    finally:
        b.close()


def test_other_coast_calls_in_between(hipctx, twinctx):
    """Between two ice calls the same context runs get_dist_um_win on another mask (it overwrites the scratch UM bit plane)
    and a regular-grid get_edges + get_dist (the scratch bit plane and the coordinate tables): the next ice call is exact."""
    for name in ("a", "c"):
        cset, prec = SET[name], 8
        _, nx, ny, win, halo, maxdist, _ = cset
        dt = _dt(prec)
        lat, lon = ur.grid_named("polar", nx, ny, dt)
        land, lf_l, planes, co = _inputs(name, prec)
        b = _Coast(hipctx, cset, lat, lon, lf_l)
        try:
            frame, _ = b.ice(planes[3])
            assert eh.same_bits(np.ascontiguousarray(_inner(frame, halo, nx, ny)), _twin(twinctx, cset, lat, lon, land, lf_l, planes[3]))
            oland, oice = ur.noise_mask(nx, ny, 11, dt)
            _, _, ocoast = ur.coast_of(oland, oice, *halo)
            other = hipctx.get_dist_um_win(ocoast, oland, lat, lon, *halo, *win, maxdist=maxdist)
            assert (np.abs(_inner(other, halo, nx, ny)) < 12000.0).any()
            st = synth.static_fields(nx, ny, dt)
            hipctx.get_dist(hipctx.get_edges(st.landfrac, st.icefrac), st.landfrac, st.lon, st.lat)
            for n in (8, 9, 10):
                frame, rep = b.ice(planes[n])
                assert eh.same_bits(np.ascontiguousarray(_inner(frame, halo, nx, ny)), _twin(twinctx, cset, lat, lon, land, lf_l, planes[n])), \
                    (name, uic.PLANES[n])
                assert 0 < rep["tiles_marked"]
        finally:
            b.close()


# ---- seabreeze_diag_um steps with ice calls between them ---------------------------------------------------------------

@pytest.mark.parametrize("mode", ["plan", "tables"])
def test_um_steps_follow_the_ice(mode):
    """200 x 70 x 4, halo_l = 15 (set a), four steps, an ice call ahead of steps 1, 2 and 4; cdist's ghost cells are
    edge-replicated after every ice call.  The twin steps on a mask made by get_edges_um + get_dist_um_win on a fresh
    context at every step.  Masks, outputs and state: bit for bit."""
    cset, dt, nz = SET["a"], np.float64, 4
    _, nx, ny, win, halo, maxdist, _ = cset
    h = halo[0]
    assert halo == (15, 15)
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    land, lf_l, planes, co = _inputs("a", 8)
    ice_of_step = {1: planes[0], 2: planes[7], 3: planes[7], 4: planes[10]}
    core = (slice(h, h + ny), slice(h, h + nx))
    st = synth.static_fields(nx + 2 * h, ny + 2 * h, dt)                   # a bigger field whose rim serves as ghosts
    p = synth.pressure_3d(st, nz, dt)[:, core[0], core[1]].copy()
    flags = hip.SB_UM_THETA_TO_T0 | hip.SB_UM_LEVEL_WALK

    def fresh_mask(ci):
        c = hip.Context()
        try:
            return c.get_dist_um_win(c.get_edges_um(lf_l, ci, *halo), land, lat, lon, *halo, *win, maxdist=maxdist)
        finally:
            c.close()

    def run(ice_path):
        ctx = hip.Context()
        try:
            if mode == "tables":
                ctx.set_table_contrast(True); ctx.set_table_window_cache(True)
            else:
                ctx.set_plan_cache(True)
            if ice_path:
                ctx.um_coast_open(dt, nx, ny, *halo, *win, lat, lon, maxdist=maxdist)
            cd = np.zeros_like(lf_l)
            state = [np.zeros((ny, nx), dt) for _ in range(4)]
            out, masks, counters, last = [], [], [], None
            for tn in (1, 2, 3, 4):
                ci = ice_of_step[tn]
                if ci is not last:
                    cd = ctx.um_ice(lf_l, ci, cd) if ice_path else fresh_mask(ci)
                    last = ci
                mask = ur.pad_edge(cd[core], h, h)
                th = synth.theta_step(st, tn, dt)
                u, v = (a[:, core[0], core[1]].copy() for a in synth.wind_step(st, nz, tn, dt))
                assert ctx.seabreeze_diag_um(7200.0, tn, p, u, v, th.copy(), st.z, st.sigma, mask, *state, halo_s=h, halo_l=h,
                                             flags=flags) == 0
                counters.append(ctx.last_counters())
                out.append([s.copy() for s in state])
                masks.append(mask)
            if ice_path:
                assert ctx.um_ice_report()["changed_calls"] == 2
                ctx.um_coast_close()
            return out, masks, counters
        finally:
            ctx.close()

    got, gm, gc = run(True)
    want, wm, wc = run(False)
    assert not np.array_equal(gm[0], gm[1]) and not np.array_equal(gm[2], gm[3]), "the ice calls left the mask alone"
    for tn in range(4):
        assert eh.same_bits(gm[tn], wm[tn]), f"step {tn + 1}: mask frames differ"
        for nm, a, w in zip(("ws", "wd", "thc", "sb_con"), got[tn], want[tn]):
            assert eh.same_bits(a, w), (mode, f"step {tn + 1}", nm, int((a != w).sum()))
    assert gc == wc and all(c["band_cells"] > 0 for c in gc), "no band cell: the steps show nothing"


# ---- enqueue only ------------------------------------------------------------------------------------------------------

def test_ice_calls_only_enqueue():
    """The ice calls go behind device work on a caller's stream (tests/enqueue_harness.py's layout: the filler, the ice frame
    copied in place, the call, a snapshot) and return while the filler is still running; one synchronisation at the end.
    The twin: the same sequence, synchronised after every call, on a fresh context."""
    cset, dt = SET["a"], np.float64
    _, nx, ny, win, halo, maxdist, _ = cset
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    land, lf_l, planes, co = _inputs("a", 8)
    seq = [planes[0], planes[3], planes[8], planes[10], planes[11]]
    filler = eh.Filler()
    s = torch.cuda.Stream()

    def run(busy):
        ctx = hip.Context()
        try:
            ctx.um_coast_open(dt, nx, ny, *halo, *win, lat, lon, maxdist=maxdist)
            lf, ci_all = _dev(lf_l), torch.stack([_dev(c) for c in seq])
            ci = _dev(planes[5])                                  # a valid frame that is not in the sequence
            cd = torch.full_like(lf, SENTINEL)
            hist = [torch.zeros_like(cd) for _ in seq]
            ev = [torch.cuda.Event() for _ in seq]
            before, after, t_enq = [None] * len(seq), [None] * len(seq), []
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                for n in range(len(seq)):
                    if busy:
                        filler.enqueue()
                        ev[n].record(s)
                    ci.copy_(ci_all[n])
                    if busy:
                        before[n] = not ev[n].query()
                    t0 = time.perf_counter()
                    ctx.um_ice_dev(dt, lf.data_ptr(), ci.data_ptr(), cd.data_ptr(), stream=s.cuda_stream)
                    t_enq.append(time.perf_counter() - t0)
                    if busy:
                        after[n] = not ev[n].query()
                    hist[n].copy_(cd)
                    if not busy:
                        s.synchronize(); ctx.synchronize()
            s.synchronize()
            rep = ctx.um_ice_report()
            ctx.um_coast_close()
            return [a.cpu().numpy() for a in hist], before, after, rep, t_enq
        finally:
            ctx.close()

    got, before, after, rep, t_enq = run(True)
    want, _, _, rep_w, _ = run(False)
    print(f"[enqueue-only] um ice: filler {filler.ms:.2f} ms, host enqueue per call (ms) {[round(1e3 * t, 3) for t in t_enq]}")
    # steady state: the calls behind the first
    if not all(before[1:]):
        raise eh.VacuousRun(f"the filler had finished before the calls were made: {before}")
    assert all(after[1:]), f"a call returned only after the filler ahead of it had finished -- a hidden synchronisation: {after}"
    eh.check_ratio(filler, float(np.median(t_enq[1:])), "um ice")
    for n in range(len(seq)):
        assert eh.same_bits(got[n], want[n]), f"call {n + 1}"
    assert rep == rep_w and rep["calls"] == len(seq) and rep["changed_calls"] == len(seq) - 1
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[2], got[3])


# ---- the host form -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
def test_host_form(hipctx, prec):
    """um_ice on numpy frames equals the _dev form's interior; the ghost cells of cdist_l are untouched"""
    cset = SET["b"]
    _, nx, ny, win, halo, maxdist, _ = cset
    dt = _dt(prec)
    lat, lon = ur.grid_named("polar", nx, ny, dt)
    land, lf_l, planes, co = _inputs("b", prec)
    b = _Coast(hipctx, cset, lat, lon, lf_l)
    try:
        dev = [b.ice(planes[n])[0] for n in (0, 3, 7, 8)]
    finally:
        b.close()
    hipctx.um_coast_open(dt, nx, ny, *halo, *win, lat, lon, maxdist=maxdist)
    try:
        cd = np.full(lf_l.shape, SENTINEL, dt)
        for k, n in enumerate((0, 3, 7, 8)):
            assert hipctx.um_ice(lf_l, planes[n], cd) is cd
            assert _ghosts_keep(cd, halo, nx, ny), "ghost cells of cdist_l were written"
            assert eh.same_bits(np.ascontiguousarray(_inner(cd, halo, nx, ny)), np.ascontiguousarray(_inner(dev[k], halo, nx, ny))), uic.PLANES[n]
        assert hipctx.um_ice_report()["calls"] == 4
        with pytest.raises(ValueError):
            hipctx.um_ice(lf_l[1:], planes[0], cd)
    finally:
        hipctx.um_coast_close()
    with pytest.raises(hip.SeabreezeHipError, match="without um_coast_open"):
        hipctx.um_ice(lf_l, planes[0], cd)


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refused_calls():
    dt, nx, ny, hi, hj, wi, wj = np.float64, 70, 12, 2, 3, 9, 4
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    ctx = hip.Context()
    lib, I = ctx.lib, C.c_int
    SB_ERR_ARG = 1
    f = torch.zeros((ny + 2 * hj, nx + 2 * hi), dtype=torch.float64, device="cuda")
    f32 = torch.zeros((ny + 2 * hj, nx + 2 * hi), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def open_(nx_=nx, ny_=ny, hi_=hi, hj_=hj, wi_=wi, wj_=wj, lat_=lat, lon_=lon, h=ctx.h):
        return lib.sb_um_coast_open_f64(h, I(nx_), I(ny_), I(hi_), I(hj_), I(wi_), I(wj_), hip._p(lat_), hip._p(lon_), C.c_double(180.0), I(1))

    def ice(fn, a, b, c):
        return fn(ctx.h, hip._p(a), hip._p(b), hip._p(c), None)

    def refused(rc):
        return rc == SB_ERR_ARG and len(lib.sb_last_error(ctx.h)) > 0

    # what a served call must give: no ice over an empty land -- no coast anywhere --, or one iced cell -- an island
    g = f.clone()
    g[hj + 5, hi + 30] = 0.6
    other = hip.Context()
    island = other.get_dist_um_win(other.get_edges_um(np.zeros(f.shape, dt), g.cpu().numpy(), hi, hj), np.zeros((ny, nx), dt), lat, lon,
                                   hi, hj, wi, wj)
    other.close()
    assert (np.abs(_inner(island, (hi, hj), nx, ny)) < 12000.0).any()
    cd = torch.full_like(f, SENTINEL)
    turn = [0]

    def serves():
        """the open coast serves a correct ice call: the island and the empty sea take turns, so every call changes the coast"""
        turn[0] += 1
        ctx.um_ice_dev(dt, f.data_ptr(), (g if turn[0] & 1 else f).data_ptr(), cd.data_ptr())
        ctx.synchronize()
        out = cd.cpu().numpy()
        want = _inner(island, (hi, hj), nx, ny) if turn[0] & 1 else np.full((ny, nx), 12000.0)
        return _ghosts_keep(out, (hi, hj), nx, ny) and bool(np.array_equal(_inner(out, (hi, hj), nx, ny), want))

    try:
        rep = (C.c_longlong * 4)()
        assert refused(ice(lib.sb_um_ice_f64_dev, f.data_ptr(), f.data_ptr(), f.data_ptr()))               # not open
        assert b"without sb_um_coast_open" in lib.sb_last_error(ctx.h)
        assert refused(lib.sb_um_ice_report(ctx.h, rep)) and refused(lib.sb_um_coast_close(ctx.h))
        host = np.zeros((ny + 2 * hj, nx + 2 * hi), dt)
        assert refused(lib.sb_um_ice_f64(ctx.h, hip._p(host), hip._p(host), hip._p(host)))
        bad = (dict(nx_=0), dict(ny_=0), dict(nx_=-3), dict(hi_=0), dict(hj_=0), dict(hi_=-1), dict(wi_=-1), dict(wj_=-1),
               dict(wi_=hip.SB_DIST_UM_MAX_WINDOW + 1), dict(wj_=hip.SB_DIST_UM_MAX_WINDOW + 1), dict(lat_=None), dict(lon_=None))
        for kw in bad:
            assert refused(open_(**kw)), kw
            assert open_() == 0 and serves(), ("after", kw)       # ... and the context still serves a correct ice call
            assert lib.sb_um_coast_close(ctx.h) == 0
        assert open_(h=None) == SB_ERR_ARG and len(lib.sb_last_error(None)) > 0
        assert open_() == 0
        assert refused(open_())                                   # open twice
        assert b"already open" in lib.sb_last_error(ctx.h)
        assert serves()
        assert refused(ice(lib.sb_um_ice_f32_dev, f32.data_ptr(), f32.data_ptr(), f32.data_ptr()))          # the other precision
        assert b"other precision" in lib.sb_last_error(ctx.h)
        assert refused(lib.sb_um_ice_f32(ctx.h, hip._p(host), hip._p(host), hip._p(host)))
        assert serves()
        for args in ((None, f.data_ptr(), f.data_ptr()), (f.data_ptr(), None, f.data_ptr()), (f.data_ptr(), f.data_ptr(), None)):
            assert refused(ice(lib.sb_um_ice_f64_dev, *args)), args
            assert serves()
        assert refused(lib.sb_um_ice_report(ctx.h, None))
        assert lib.sb_um_ice_report(ctx.h, rep) == 0 and rep[0] >= 1 and rep[3] == uir.groups(ny) * uir.tiles(nx)
        # the band's and the stream's moving coasts are states of their own: a band coast opens beside the UM one
        blon, blat = np.linspace(0, 359, nx), np.linspace(-80, 80, ny + 2 * hj)
        ctx.band_coast_open(dt, nx, ny, hj, True, True, blon, blat, 2)
        assert serves()
        ctx.band_coast_close()
        ctx.um_coast_close()
        with pytest.raises(hip.SeabreezeHipError, match=r"\(1\).*without sb_um_coast_open"):
            ctx.um_ice_dev(dt, f.data_ptr(), f.data_ptr(), f.data_ptr())
    finally:
        ctx.close()
