"""A latitude band whose coast moves with the sea ice (sb_band_coast_open_*, sb_band_ice_*_dev, sb_band_ice_report,
sb_band_coast_close; include/seabreeze_hip.h) in one process, without a communicator: a whole grid is cut into three bands
with numpy slices (tests/band_frames.py), one hip.Context per band.  Every band gets ghost-celled frames of lsm and ci whose
cut-side ghost rows are the neighbour's rows (what swap_bounds would deliver) and whose pole-side ghost rows, their
latitudes and the east-west ghost columns are NaN (never read); cdist's frame carries a sentinel that only the interior
may lose.  NO coast is exchanged: a band forms the coast of its ghost source rows itself.

After every one of the twelve planes of tests/band_ice_cases.py the stacked interiors must equal

* the whole-grid get_edges(rule, SB_BND_GLOBAL) + get_dist(kwin) of the library on the same device BIT FOR BIT -- run on
  the middle band's own context, between its ice calls: they overwrite that context's scratch bit plane and key its
  coordinate tables, which the band coast must not mind;
* the CPU oracle under the tolerances of tests/test_band_setup_gpu.py;

and every band's report must lie between the brute-force count and the cap of tests/band_ice_ref.py.  Shapes: one per
kernel of sb_dist_kernel(nx, k) -- the mirror of that decision is asserted -- in fp32 and fp64, both land rules, both
coordinate sets.  What each plane is meant to do is asserted from the oracle on the case's own inputs.  Then band steps
with ice calls between them against a twin whose cdist is made afresh, an enqueue-only run behind device work on a caller's
stream, and the calls that must be refused.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import band_ice_cases as bic
import band_ice_ref
import enqueue_harness as eh
from band_frames import SENTINEL, cuts_of, frame, frame_lat, interior, only_interior_written
from seabreeze_param_amd import hip, synth
from test_band_setup_gpu import TOL, check_dist, coords, dist_kernel

pytestmark = pytest.mark.gpu

IDS = [c[0] for c in bic.CASES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _level(k):
    return 2.3 if k < 32 else 2.62                                # (fewer blobs under the wide window: the oracle's cost)


@pytest.fixture(scope="module")
def bandctx():
    ctxs = [hip.Context() for _ in range(3)]
    yield ctxs
    for c in ctxs:
        c.close()


class _Bands:
    """three bands of one grid, a context each: resident frames of lsm, ci and cdist on the device"""

    def __init__(self, ctxs, land, lon, lat, bands, h, k, rule, incremental=True):
        self.ctxs, self.bands, self.h, self.dt = ctxs, bands, h, land.dtype
        self.ny, self.nx = land.shape
        self.lsm, self.ci, self.cd = [], [], []
        for ctx, (r0, r1) in zip(ctxs, bands):
            self.lsm.append(_dev(frame(land, r0, r1, h)))
            self.ci.append(torch.zeros_like(self.lsm[-1]))
            self.cd.append(torch.full_like(self.lsm[-1], SENTINEL))
            ctx.band_coast_open(self.dt, self.nx, r1 - r0, h, r0 == 0, r1 == self.ny, lon, frame_lat(lat, r0, r1, h), k, rule=rule,
                                incremental=incremental)
        torch.cuda.synchronize()

    def ice(self, ci, stream=None, sentinel=True):
        """one ice call per band -> the stacked interiors, per band the report.  sentinel=False: the test has filled the
        ghost cells of cdist itself"""
        rows, reps = [], []
        for i, (ctx, (r0, r1)) in enumerate(zip(self.ctxs, self.bands)):
            self.ci[i].copy_(_dev(frame(ci, r0, r1, self.h)))
            torch.cuda.synchronize()
            ctx.band_ice_dev(self.dt, self.lsm[i].data_ptr(), self.ci[i].data_ptr(), self.cd[i].data_ptr(), stream=stream)
            reps.append(ctx.band_ice_report())                    # (synchronises)
            out = self.cd[i].cpu().numpy()
            assert not sentinel or only_interior_written(out, self.h), f"band {r0}:{r1}: ghost cells of cdist were written"
            rows.append(interior(out, self.h).copy())
        return np.concatenate(rows), reps

    def close(self):
        for ctx in self.ctxs:
            ctx.band_coast_close()


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("cset", [1, 2])
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("case", bic.CASES, ids=IDS)
def test_band_cdist_follows_every_plane(bandctx, oracles, case, rule, cset, prec):
    name, nx, k, h, heights, kern = case
    assert dist_kernel(nx, k) == kern
    dt, orc = (np.float64, oracles[8]) if prec == 8 else (np.float32, oracles[4])
    bands, ny = cuts_of(heights), sum(heights)
    r0m, r1m = bands[1]
    lon, lat = coords(nx, ny, cset, dt)
    land, planes = bic.make(nx, k, bands, dt, _level(k))
    nt = band_ice_ref.tiles(nx)

    # ---- the oracle, once: the coast of every plane, a distance field per distinct coast ----
    coast_o, dist_o = [], []
    for ci in planes:
        c = orc.get_edges(land, ci, rule=rule, bnd=1)
        same = [j for j in range(len(coast_o)) if np.array_equal(coast_o[j], c)]
        coast_o.append(c)
        dist_o.append(dist_o[same[0]] if same else orc.get_dist(c, land, lon, lat, maxdist=180.0, kwin=k))
    src = [band_ice_ref.source_rows(g0, g1, ny, k) for g0, g1 in bands]
    # ---- the inputs do what the planes are meant to do ----
    assert not np.array_equal(planes[2], planes[0]) and np.array_equal(coast_o[1], coast_o[0]) and np.array_equal(coast_o[2], coast_o[0])
    assert not np.array_equal(orc.get_edges(land, planes[0], rule=1 - rule, bnd=1), coast_o[0]), "the two land rules agree"
    for n in range(3, 10):
        assert not np.array_equal(coast_o[n], coast_o[n - 1]), f"plane {bic.PLANES[n]} leaves the coast alone"
    lo, hi = src[1]
    assert not np.array_equal(coast_o[4][lo], coast_o[3][lo]) and not np.array_equal(coast_o[4][hi - 1], coast_o[3][hi - 1]), \
        "plane 5 does not reach the middle band's outermost source rows"
    assert not np.array_equal(dist_o[4][r0m:r1m], dist_o[3][r0m:r1m]), "plane 5 moves no distance of the middle band"
    assert np.array_equal(coast_o[5][lo:hi], coast_o[4][lo:hi]) and not np.array_equal(coast_o[5][src[0][0]:src[0][1]], coast_o[4][src[0][0]:src[0][1]])
    own = orc.get_dist(coast_o[4][r0m:r1m], land[r0m:r1m], lon, lat[r0m:r1m], maxdist=180.0, kwin=k)
    assert not np.array_equal(own, dist_o[4][r0m:r1m]), "a band that ignored its ghost source rows would be right"
    assert np.array_equal(coast_o[10], coast_o[0]) and not np.array_equal(coast_o[11], coast_o[10])

    whole_path = kern == "BYTES"
    want = []
    for inc in (True, False):
        b = _Bands(bandctx, land, lon, lat, bands, h, k, rule, incremental=inc)
        try:
            changed_calls = [0, 0, 0]
            for n, ci in enumerate(planes):
                if inc:
                    ctx = bandctx[1]
                    want.append(ctx.get_dist(ctx.get_edges(land, ci, rule=rule, bnd=hip.SB_BND_GLOBAL), land, lon, lat, maxdist=180.0, kwin=k))
                got, reps = b.ice(ci)
                diff = got.view(np.uint8).reshape(ny, -1) != want[n].view(np.uint8).reshape(ny, -1)
                assert not diff.any(), (name, bic.PLANES[n], inc, f"rows {np.flatnonzero(diff.any(1))[:8]} differ from the whole-grid call")
                if inc:
                    check_dist(got, dist_o[n], f"{name} rule {rule} set {cset} fp{8 * prec} plane {n + 1}", TOL[prec])
                for i, ((g0, g1), (s0, s1), rep) in enumerate(zip(bands, src, reps)):
                    print(f"{name} plane {n + 1} band {g0}:{g1} inc {int(inc)}: {rep}")
                    assert rep["calls"] == n + 1 and rep["tiles"] == (g1 - g0) * nt
                    if not inc or whole_path:
                        assert rep["changed_calls"] == -1 and rep["tiles_marked"] == rep["tiles"]
                        continue
                    if n == 0:
                        assert rep["tiles_marked"] == rep["tiles"] and rep["changed_calls"] == 0      # the first call computes everything
                        continue
                    changed = band_ice_ref.changed_cells(coast_o[n][s0:s1], coast_o[n - 1][s0:s1])
                    changed = [(x, y + s0) for x, y in changed]
                    changed_calls[i] += 1 if changed else 0
                    assert rep["changed_calls"] == changed_calls[i], (bic.PLANES[n], i)
                    lo_n = int(band_ice_ref.brute_marks(nx, g0, g1, k, changed).sum())
                    hi_n = int(band_ice_ref.cap_marks(nx, g0, g1, k, changed).sum())
                    assert lo_n <= rep["tiles_marked"] <= hi_n, (bic.PLANES[n], i, lo_n, rep["tiles_marked"], hi_n)
                    if n in (1, 2):
                        assert rep["tiles_marked"] == 0 and not changed
                    if n == 5:                                    # row r0-(k+2): beyond what the middle band's Sobel reads
                        assert (rep["tiles_marked"] == 0 and not changed) if i == 1 else (i != 0 or rep["tiles_marked"] > 0)
                    if n == 4 and i == 1:
                        assert rep["tiles_marked"] > 0
        finally:
            b.close()


# ---- band steps with ice calls between them ---------------------------------------------------------------------------

def _ghosts_of(full, r0, r1, h):
    """rows r0-h .. r1+h-1 of a whole field with the longitude wrapped into the ghost columns (every row is inside the grid)"""
    ny, nx = full.shape
    return np.ascontiguousarray(full[np.ix_(np.arange(r0 - h, r1 + h), np.arange(-h, nx + h) % nx)])


def _set_ghosts(dst, src, h):
    """the ghost cells of a device frame from another one; the interior stays"""
    dst[:h] = src[:h]
    dst[-h:] = src[-h:]
    dst[h:-h, :h] = src[h:-h, :h]
    dst[h:-h, -h:] = src[h:-h, -h:]


def _step_inputs(nx, nyl, nz, dt, tns):
    st = synth.static_fields(nx, nyl, dt)
    return st, synth.pressure_3d(st, nz, dt), {tn: (synth.theta_step(st, tn, dt),) + synth.wind_step(st, nz, tn, dt) for tn in tns}


def _switches(ctx, mode, on):
    if mode == "tables":
        ctx.set_table_contrast(on); ctx.set_table_contrast_bands(on); ctx.set_table_window_cache(on)
    else:
        ctx.set_plan_cache(True)


@pytest.mark.parametrize("mode", ["plan", "tables"])
def test_band_steps_follow_the_ice(bandctx, mode):
    """BITS32, the middle band, nz = 3, four steps, an ice call before steps 2 and 4; the ghost cells of cdist come from the
    neighbour bands' results.  The twin steps on a mask made by band_get_edges + band_get_dist on a fresh context at every
    step.  Outputs and state: bit for bit."""
    name, nx, k, h, heights, kern = bic.CASES[0]
    dt, rule, nz = np.float64, 1, 3
    bands, ny = cuts_of(heights), sum(heights)
    r0, r1 = bands[1]
    nyl = r1 - r0
    lon, lat = coords(nx, ny, 2, dt)
    land, planes = bic.make(nx, k, bands, dt, _level(k))
    ice_of_step = {1: planes[0], 2: planes[4], 3: planes[4], 4: planes[11]}
    st, p, per = _step_inputs(nx, nyl, nz, dt, (1, 2, 3, 4))

    def fresh_mask(ci):
        """the whole field from three bands of a fresh context: edges, the exchange of coast (numpy), distance"""
        c = hip.Context()
        try:
            coast = np.concatenate([interior(c.band_get_edges(frame(land, a, b, h), frame(ci, a, b, h), h, a == 0, b == ny, rule=rule), h)
                                    for a, b in bands])
            return np.concatenate([interior(c.band_get_dist(frame(coast, a, b, h), frame(land, a, b, h), lon, frame_lat(lat, a, b, h), h,
                                                            a == 0, b == ny, k), h) for a, b in bands])
        finally:
            c.close()

    def run(ice_path):
        ctx = hip.Context()
        b = None
        try:
            _switches(ctx, mode, True)
            ctx.set_search_radius_hint(k + 1)
            stream = torch.cuda.current_stream().cuda_stream
            fr = lambda a: _dev(eh.frame(a, h, dt))
            z, sg = fr(st.z), fr(st.sigma)
            torch.cuda.synchronize()
            for f in (z, sg):
                ctx.swap_bounds_dev(dt, f.data_ptr(), nx, nyl, h, stream)
            ctx.synchronize()
            pd = _dev(p)
            state = [torch.zeros((nyl, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
            mask = torch.zeros((nyl + 2 * h, nx + 2 * h), dtype=torch.float64, device="cuda")
            if ice_path:
                b = _Bands([bandctx[0], ctx, bandctx[2]], land, lon, lat, bands, h, k, rule)
                b.cd[1] = mask
            out, masks, last = [], [], None
            for tn in (1, 2, 3, 4):
                ci = ice_of_step[tn]
                if ci is not last:
                    if ice_path:
                        full, _ = b.ice(ci, sentinel=False)
                        _set_ghosts(mask, _dev(_ghosts_of(full, r0, r1, h)), h)
                    else:
                        mask.copy_(_dev(_ghosts_of(fresh_mask(ci), r0, r1, h)))
                    last = ci
                th, u, v = per[tn]
                thf, ud, vd = fr(th), _dev(u), _dev(v)
                torch.cuda.synchronize()
                ctx.band_seabreeze_diag_dev(dt, 5400.0, tn, nx, nyl, nz, h, pd.data_ptr(), ud.data_ptr(), vd.data_ptr(), thf.data_ptr(),
                                            mask.data_ptr(), z.data_ptr(), sg.data_ptr(), *[s.data_ptr() for s in state], stream)
                ctx.synchronize()
                out.append([s.cpu().numpy().copy() for s in state])
                masks.append(mask.cpu().numpy().copy())
            return out, masks
        finally:
            if b is not None:
                b.close()
            _switches(ctx, mode, False)
            ctx.close()

    got, gm = run(True)
    want, wm = run(False)
    assert not np.array_equal(gm[0], gm[1]) and not np.array_equal(gm[2], gm[3]), "the ice calls left the mask alone"
    for tn in range(4):
        assert eh.same_bits(gm[tn], wm[tn]), f"step {tn + 1}: mask frames differ"
        for nm, a, w in zip(("ws", "wd", "thc", "sb_con"), got[tn], want[tn]):
            assert eh.same_bits(a, w), (mode, f"step {tn + 1}", nm, int((a != w).sum()))
    assert np.any(got[3][3] < 1e19), "no band cell: the steps show nothing"


# ---- enqueue only ------------------------------------------------------------------------------------------------------

def test_ice_calls_and_steps_only_enqueue():
    """Ice calls and band steps go behind device work on a caller's stream (tests/enqueue_harness.py's layout: the filler,
    the step's inputs copied in place, the calls, snapshots) and return while the filler is still running; one
    synchronisation at the end.  The twin: the same sequence, synchronised after every call, on a fresh context."""
    name, nx, k, h, heights, kern = bic.CASES[0]
    dt, rule, nz = np.float64, 1, 3
    bands, ny = cuts_of(heights), sum(heights)
    r0, r1 = bands[1]
    nyl = r1 - r0
    lon, lat = coords(nx, ny, 2, dt)
    land, planes = bic.make(nx, k, bands, dt, _level(k))
    seq = [planes[0], planes[4], planes[9], planes[11]]           # the ice plane ahead of steps 1 .. 4
    st, p, per = _step_inputs(nx, nyl, nz, dt, (1, 2, 3, 4, 5))
    filler = eh.Filler()
    s = torch.cuda.Stream()

    def run(busy):
        ctx = hip.Context()
        try:
            ctx.set_search_radius_hint(k + 1)
            ctx.band_coast_open(dt, nx, nyl, h, False, False, lon, frame_lat(lat, r0, r1, h), k, rule=rule)
            fr = lambda a: _dev(eh.frame(a, h, dt))
            lsm, ci_all = _dev(frame(land, r0, r1, h)), torch.stack([_dev(frame(c, r0, r1, h)) for c in seq])
            th_all, u_all, v_all = (torch.stack([_dev(eh.frame(per[tn][j], h, dt) if j == 0 else per[tn][j]) for tn in (1, 2, 3, 4)])
                                    for j in range(3))
            # the buffers the library is given hold valid inputs of a step beyond the sequence until a step rewrites them
            ci, th, u, v = _dev(frame(planes[6], r0, r1, h)), fr(per[5][0]), _dev(per[5][1]), _dev(per[5][2])
            z, sg, pd = fr(st.z), fr(st.sigma), _dev(p)
            mask = torch.zeros((nyl + 2 * h, nx + 2 * h), dtype=torch.float64, device="cuda")
            state = [torch.zeros((nyl, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
            hist = [[torch.zeros_like(a) for a in state + [mask]] for _ in range(4)]
            ev = [torch.cuda.Event() for _ in range(4)]
            before, after = [None] * 4, [None] * 4
            torch.cuda.synchronize()
            h_s = s.cuda_stream
            with torch.cuda.stream(s):
                for f in (z, sg):
                    ctx.swap_bounds_dev(dt, f.data_ptr(), nx, nyl, h, stream=h_s)
                for n in range(4):
                    if busy:
                        filler.enqueue()
                        ev[n].record(s)
                    ci.copy_(ci_all[n]); th.copy_(th_all[n]); u.copy_(u_all[n]); v.copy_(v_all[n])
                    if busy:
                        before[n] = not ev[n].query()
                    ctx.band_ice_dev(dt, lsm.data_ptr(), ci.data_ptr(), mask.data_ptr(), stream=h_s)
                    ctx.band_seabreeze_diag_dev(dt, 5400.0, n + 1, nx, nyl, nz, h, pd.data_ptr(), u.data_ptr(), v.data_ptr(), th.data_ptr(),
                                                mask.data_ptr(), z.data_ptr(), sg.data_ptr(), *[a.data_ptr() for a in state], h_s)
                    if busy:
                        after[n] = not ev[n].query()
                    for d, a in zip(hist[n], state + [mask]):
                        d.copy_(a)
                    if not busy:
                        s.synchronize(); ctx.synchronize()
            s.synchronize()
            ctx.band_coast_close()
            return [[a.cpu().numpy() for a in step] for step in hist], before, after
        finally:
            ctx.close()

    got, before, after = run(True)
    want, _, _ = run(False)
    # steady state: the calls behind the first (the first of a context allocates)
    if not all(before[1:]):
        raise eh.VacuousRun(f"the filler had finished before the calls were made: {before}")
    assert all(after[1:]), f"a call returned only after the filler ahead of it had finished -- a hidden synchronisation: {after}"
    for n in range(4):
        for nm, a, w in zip(("ws", "wd", "thc", "sb_con", "mask"), got[n], want[n]):
            assert eh.same_bits(a, w), (f"step {n + 1}", nm)
    assert not np.array_equal(got[0][4], got[1][4]) and not np.array_equal(got[2][4], got[3][4])


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refused_calls():
    dt, nx, ny, h, k = np.float64, 64, 12, 5, 4
    lon, latf = coords(nx, ny + 2 * h, 1, dt)
    ctx = hip.Context()
    lib, I = ctx.lib, C.c_int
    SB_ERR_ARG = 1
    f = torch.zeros((ny + 2 * h, nx + 2 * h), dtype=torch.float64, device="cuda")
    f32 = torch.zeros((ny + 2 * h, nx + 2 * h), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def open_(south, north, kwin, rule=1, halo=h, lon_=lon, lat_=latf):
        return lib.sb_band_coast_open_f64(ctx.h, I(nx), I(ny), I(halo), I(south), I(north), hip._p(lon_), hip._p(lat_), C.c_double(180.0),
                                          I(kwin), I(rule), I(1))

    def ice(fn, a, b, c):
        return fn(ctx.h, hip._p(a), hip._p(b), hip._p(c), None)

    try:
        rep = (C.c_longlong * 4)()
        assert ice(lib.sb_band_ice_f64_dev, f.data_ptr(), f.data_ptr(), f.data_ptr()) == SB_ERR_ARG          # not open
        assert lib.sb_band_ice_report(ctx.h, rep) == SB_ERR_ARG and lib.sb_band_coast_close(ctx.h) == SB_ERR_ARG
        assert open_(0, 0, h) == SB_ERR_ARG and open_(0, 1, h) == SB_ERR_ARG and open_(1, 0, h) == SB_ERR_ARG   # kwin + 1 > halo, a cut side
        assert open_(0, 0, -1) == SB_ERR_ARG
        assert open_(1, 1, hip.SB_DIST_MAX_WINDOW + 1) == SB_ERR_ARG
        assert open_(0, 0, k, rule=2) == SB_ERR_ARG and open_(0, 0, k, rule=-1) == SB_ERR_ARG
        assert open_(0, 0, k, lon_=None) == SB_ERR_ARG and open_(0, 0, k, lat_=None) == SB_ERR_ARG
        assert lib.sb_band_coast_open_f64(None, I(nx), I(ny), I(h), I(0), I(0), hip._p(lon), hip._p(latf), C.c_double(180.0), I(k), I(1),
                                          I(1)) == SB_ERR_ARG
        assert open_(1, 1, h) == 0                                # both poles: no ghost row is needed
        assert lib.sb_band_coast_close(ctx.h) == 0
        assert open_(0, 0, k) == 0
        assert open_(0, 0, k) == SB_ERR_ARG                       # open twice
        assert b"already open" in lib.sb_last_error(ctx.h)
        assert ice(lib.sb_band_ice_f32_dev, f32.data_ptr(), f32.data_ptr(), f32.data_ptr()) == SB_ERR_ARG      # the other precision
        for args in ((None, f.data_ptr(), f.data_ptr()), (f.data_ptr(), None, f.data_ptr()), (f.data_ptr(), f.data_ptr(), None)):
            assert ice(lib.sb_band_ice_f64_dev, *args) == SB_ERR_ARG
        assert lib.sb_band_ice_report(ctx.h, None) == SB_ERR_ARG
        assert lib.sb_band_ice_report(ctx.h, rep) == 0 and list(rep)[:3] == [0, 0, 0]
        # ... and the coast is still usable: an empty land has no coast anywhere
        cd = torch.full_like(f, SENTINEL)
        torch.cuda.synchronize()
        ctx.band_ice_dev(dt, f.data_ptr(), f.data_ptr(), cd.data_ptr())
        assert ctx.band_ice_report()["calls"] == 1
        out = cd.cpu().numpy()
        assert only_interior_written(out, h) and np.all(interior(out, h) == 12000.0)
        ctx.band_coast_close()
        with pytest.raises(hip.SeabreezeHipError, match=r"\(1\).*without sb_band_coast_open"):
            ctx.band_ice_dev(dt, f.data_ptr(), f.data_ptr(), cd.data_ptr())
    finally:
        ctx.close()
