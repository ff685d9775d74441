"""A stream whose coast moves with the sea ice (sb_diag_stream_coast_*, sb_diag_stream_ice_*; include/seabreeze_hip.h)
through the C ABI, fp32 and fp64.

After every ice plane the stream's resident distance field must equal, bit for bit, sb_get_edges_* + sb_get_dist_*
(kwin = -1) of the library on the same inputs -- the incremental update computes only the tiles a changed coast word can
reach, and that is exact or it is wrong.  Grids are regional, 0.25 degrees round 70 N, with maxdist chosen so that the
window half-width comes out as wanted: one grid per distance kernel (sb_dist_plan.hpp), and the grid narrower than its
window, which takes the whole-grid path.  The planes: see PLANES.  Then steps with an ice call between them against
sb_diag_* called step by step with the library's own distance fields (bit for bit) and against the oracle (the rule of
tests/test_python_surface.py's streamed driver), an enqueue-only run behind device work on the context's stream, and
the calls that must be refused.
"""
import ctypes as C
import time

import numpy as np
import pytest

import ice_ref
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

#          kernel        nx   ny   k
GRIDS = {"BITS32": (700, 96, 6), "BITS64": (700, 96, 20), "BITS_SMALL": (200, 96, 6), "WIDE": (700, 130, 40),
         "BYTES": (24, 40, 15)}
PLANES = ["a initial ice", "b the same plane", "c changed below the threshold", "d one interior cell crosses 0.4",
          "e cells at column 0, nx-1, row 0, row ny-2", "f a cell in the ragged last word", "g an edge moved by one row",
          "h back to a", "i half the grid iced"]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    v = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(v) == b.view(v)).all())


def _regional(nx, ny, k, dt):
    """0.25-degree grid whose row ny // 2 lies at 70 N, and the maxdist [km] for which dist_window gives k (ref:
    sobel.f90:129-137: k = int(maxdist / dx), dx the haversine step between two diagonal neighbours at 70 N)."""
    lon = (100.0 + 0.25 * np.arange(nx)).astype(dt)
    lat = (70.0 + 0.25 * (np.arange(ny) - ny // 2)).astype(dt)
    d2r = 3.1415926 / 180.0
    p0, p1, dl = d2r * 70.0, d2r * 70.25, d2r * 0.25
    a = np.sin((p1 - p0) / 2) ** 2 + np.cos(p1) * np.cos(p0) * np.sin(dl / 2) ** 2
    dx = 2 * 6370.9989 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))
    maxdist = (k + 0.5) * dx
    assert hip.dist_window(lon, lat, maxdist) == k
    return lon, lat, float(maxdist)


def _land(nx, ny, dt):
    """Blobs of land of a few cells everywhere (coast cells across the seam and on the frame), with open sea round the
    cells the planes toggle."""
    r = synth.hash_uniform((ny, nx), 3, 77)
    s = r + np.roll(r, 1, 1) + np.roll(r, 1, 0) + np.roll(r, -1, 1)
    land = (s > 2.45).astype(dt)
    for y, x in _toggles(nx, ny).values():
        land[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = 0
        if x < 2:
            land[max(0, y - 2):y + 3, nx - 2:] = 0                   # (the wrapper's neighbours of column 0)
    return land


def _toggles(nx, ny):
    return {"d": (ny // 2 - 8, 20 if nx > 40 else 8), "e0": (ny // 2 - 13, 0), "e1": (ny // 2 - 3, nx - 1), "e2": (0, nx // 2 - 3),
            "e3": (ny - 2, nx // 2 + 5), "f": (ny // 2 + 3, nx - 5)}


def _planes(land, dt):
    """The nine ice planes, in order.  Ice lies over the sea of the northern rows; its edge is ragged."""
    ny, nx = land.shape
    tg = _toggles(nx, ny)
    edge = ny - 14 + (np.arange(nx) // 37) % 3                       # first iced row per column
    a = np.where((np.arange(ny)[:, None] >= edge[None, :]) & (land == 0), 0.6, 0.0).astype(dt)
    a[ny - 3:, nx // 2:nx // 2 + 10] = 0.0                           # open water round the toggle at row ny-2

    def toggle(p, key):
        y, x = tg[key]
        assert land[y, x] == 0
        p[y, x] = dt(0.0) if p[y, x] > 0.4 else dt(0.5)

    c = np.where(a > 0, a * dt(0.9), dt(0.1) * (land == 0)).astype(dt)     # 0.54 and 0.1: no cell crosses 0.4
    d = c.copy(); toggle(d, "d")
    e = d.copy()
    for key in ("e0", "e1", "e2", "e3"):
        toggle(e, key)
    f = e.copy(); toggle(f, "f")
    g = f.copy()
    x0, x1 = min(100, nx // 4), min(300, nx - nx // 4)
    for x in range(x0, x1):
        if land[edge[x] - 1, x] == 0:
            g[edge[x] - 1, x] = dt(0.6)
    i = a.copy()
    i[:, :nx // 2][land[:, :nx // 2] == 0] = dt(0.7)
    return [a, a.copy(), c, d, e, f, g, a.copy(), i]


def _library_cdist(ctx, land, ci, lon, lat, maxdist):
    coast = ctx.get_edges(land, ci)
    return coast, ctx.get_dist(coast, land, lon, lat, maxdist=maxdist)


def _open(ctx, land, lon, lat, maxdist, incremental=True):
    zero = np.zeros_like(land)
    ctx.stream_begin(zero, zero, zero, zero, zero, zero)
    ctx.stream_coast(land, lon, lat, maxdist=maxdist, incremental=incremental)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kernel", list(GRIDS))
def test_resident_cdist_follows_every_plane(hipctx, oracles, kernel, dt):
    nx, ny, k = GRIDS[kernel]
    lon, lat, maxdist = _regional(nx, ny, k, dt)
    land = _land(nx, ny, dt)
    planes = _planes(land, dt)
    # the library's own fields, on the SAME context: its get_dist calls between the ice calls overwrite the context's
    # scratch bit plane and key the coordinate tables, which the stream must not mind
    want, coasts = [], []
    whole = kernel == "BYTES"
    for inc in (True, False):                                        # (j): incremental = 0 throughout
        _open(hipctx, land, lon, lat, maxdist, incremental=inc)
        assert hipctx.stream_ice_report()["calls"] == 0
        for n, (name, ci) in enumerate(zip(PLANES, planes)):
            if inc:
                coast, cd = _library_cdist(hipctx, land, ci, lon, lat, maxdist)
                coasts.append(coast); want.append(cd)
            hipctx.stream_ice(ci)
            got = hipctx.stream_get_cdist()
            assert _same_bits(got, want[n]), (kernel, name, inc, int((got != want[n]).sum()))
            rep = hipctx.stream_ice_report()
            assert rep["calls"] == n + 1 and rep["tiles"] == ny * ice_ref.tiles(nx)
            if not inc or whole:
                assert rep["changed_calls"] == -1 and rep["tiles_marked"] == rep["tiles"]
                continue
            changed = [tuple(c[::-1]) for c in np.argwhere(coasts[n] != coasts[n - 1])] if n else None
            if n == 0:
                assert rep["tiles_marked"] == rep["tiles"] and rep["changed_calls"] == 0      # the first call computes everything
            elif name[0] in "bc":
                assert not changed and rep["tiles_marked"] == 0 and rep["changed_calls"] == 0
            else:
                assert changed, name                                 # (the plane is meant to move the coast)
                lo = int(ice_ref.brute_marks(nx, ny, k, changed).sum())
                hi = int(ice_ref.cap_marks(nx, ny, k, changed).sum())
                assert lo <= rep["tiles_marked"] <= hi, (name, lo, rep["tiles_marked"], hi)
                assert rep["changed_calls"] == "defghi".index(name[0]) + 1
                if name[0] == "d" and kernel == "BITS32":
                    # a change at column 20: tile column 1 (columns 256 .. 511) is beyond the cap, so it is clean
                    assert not ice_ref.cap_marks(nx, ny, k, changed)[:, 1].any() and hi < rep["tiles"] // 4
        assert _same_bits(want[7], want[0])                          # (h) is (a) again
        hipctx.stream_end()
    if kernel == "BITS64" and dt == np.float64:
        # ... and what they are all compared with is the reference's field (tests/test_setup_gpu.py's rule)
        orc = oracles[8]
        for n in (0, 4, 8):
            o = orc.get_dist(orc.get_edges(land, planes[n]), land, lon, lat, maxdist=maxdist)
            assert np.array_equal(want[n] >= 12000.0, o >= 12000.0) and np.array_equal(np.sign(want[n]), np.sign(o))
            assert (np.abs(want[n] - o) / np.maximum(np.abs(o), 1.0)).max() <= 1e-12


def _step_case(nx, ny, dt, regional):
    st = synth.static_fields(nx, ny, dt)
    if regional:
        lon, lat, maxdist = _regional(nx, ny, 6, dt)
        land = _land(nx, ny, dt)
        st.lon, st.lat, st.landfrac = lon, lat, land
        kw = dict(timestep=120.0, maxdist=180.0)
    else:
        lon, lat, maxdist, land = st.lon.astype(dt), st.lat.astype(dt), 180.0, st.landfrac.astype(dt)
        kw = dict(timestep=120.0, maxdist=700.0)
    nlev = 4
    pres = (synth.pressure_1d(nlev, dt) / 100.0).astype(dt)
    # the ice grows from the northern rows southwards, a row or two per step, and retreats once
    rows = [ny // 6, ny // 6 + 1, ny // 6 + 1, ny // 6 + 3, ny // 6 + 2, ny // 6 + 4]
    ice = [np.where((np.arange(ny)[:, None] >= ny - r) & (land == 0), 0.6, 0.0).astype(dt) for r in rows]
    th = [synth.theta_step(st, n + 1, dt) for n in range(6)]
    uv = [synth.wind_step(st, nlev, n + 1, dt) for n in range(6)]
    return st, land, lon, lat, maxdist, pres, ice, th, uv, kw


def _run_stream(ctx, case):
    st, land, lon, lat, maxdist, pres, ice, th, uv, kw = case
    zero = np.zeros_like(land)
    ctx.stream_begin(st.z, st.sigma, zero, zero, zero, zero)
    ctx.stream_coast(land, lon, lat, maxdist=maxdist)
    sb = np.zeros((6,) + land.shape)
    for n in range(6):
        ctx.stream_ice(ice[n])
        assert ctx.stream_step(n + 1, pres, th[n], uv[n][1], uv[n][0], sb[n - 1] if n else None, **kw) == (n > 0)
    # sb_con of the last step is output plane 0; the earlier ones came back one step behind, rows 0 .. ny-2, as doubles
    out, ws, wd, thc = ctx.stream_end()
    sb[5, :-1] = out[0, :-1]
    return sb, out, ws, wd


def _run_steps(ctx, case, side=None):
    """sb_diag_* (or the oracle's diag) step by step with that side's own distance fields"""
    st, land, lon, lat, maxdist, pres, ice, th, uv, kw = case
    side = side or ctx
    dt = land.dtype
    ws, wd, thc = (np.zeros_like(land) for _ in range(3))
    sb = np.zeros((6,) + land.shape)
    outs = []
    for n in range(6):
        cd = side.get_dist(side.get_edges(land, ice[n]), land, lon, lat, maxdist=maxdist)
        out = side.diag(n + 1, pres, st.z.astype(dt), st.sigma.astype(dt), th[n], uv[n][1], uv[n][0], cd, ws, wd, thc, **kw)
        sb[n, :-1] = out[0, :-1]
        outs.append(np.array(out))
    return sb, outs, ws, wd, thc


def _switches(ctx, mode, on):
    if mode == "tables":
        ctx.set_table_contrast(on); ctx.set_table_contrast_f2py(on); ctx.set_table_window_cache(on)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape,mode", [((96, 72), "plain"), ((700, 96), "plain"), ((700, 96), "tables"), ((700, 96), "plan")])
def test_steps_with_moving_ice(hipctx, oracles, shape, mode, dt):
    """Six steps, an ice call ahead of each.  mode "tables": the table contrast with its stored windows, which must follow
    the rewritten cdist; "plan": the strip kernel's stored plan on the stream against a twin that plans every call."""
    nx, ny = shape
    case = _step_case(nx, ny, dt, regional=nx == 700)
    twin = hip.Context()
    try:
        _switches(hipctx, mode, True); _switches(twin, mode, True)
        if mode == "plan":
            hipctx.set_plan_cache(True); twin.set_plan_cache(False)
        sb, out, ws, wd = _run_stream(hipctx, case)
        sb_t, outs_t, ws_t, wd_t, _ = _run_steps(twin, case)
    finally:
        _switches(hipctx, mode, False)
        twin.close()
    assert _same_bits(sb[:, :-1], sb_t[:, :-1])
    for k, name in ((0, "sb_con"), (1, "t0"), (2, "ws"), (3, "wd")):
        assert _same_bits(out[k][:-1], outs_t[5][k][:-1]), name
    assert _same_bits(ws[:-1], ws_t[:-1]) and _same_bits(wd[:-1], wd_t[:-1])
    if mode != "plain":
        return
    # the oracle, stepping the same inputs with its own get_edges + get_dist: away from the 0.75 K knife edge
    orc = oracles[4 if dt == np.float32 else 8]
    st, land, lon, lat, maxdist, pres, ice, th, uv, kw = case
    so = [np.zeros_like(land) for _ in range(3)]
    bad = 0
    for n in range(6):
        cd = orc.get_dist(orc.get_edges(land, ice[n]), land, lon, lat, maxdist=maxdist)
        oo = orc.diag(n + 1, pres, st.z.astype(dt), st.sigma.astype(dt), th[n], uv[n][1], uv[n][0], cd, *so, **kw)
        near = np.abs(np.abs(so[2][:-1]) - 0.75) < 5e-3
        band = oo[0, :-1] < 1e19
        ok = band & ~near
        bad += int((np.abs(sb[n, :-1][ok] - oo[0, :-1][ok]) > 5e-3).sum())
        assert np.array_equal(sb[n, :-1][~band] > 1e19, np.ones((~band).sum(), bool))
    assert bad == 0
    assert np.max(np.abs(ws[:-1] - oo[2, :-1])) < 1e-4 and np.max(np.abs(out[1][:-1] - oo[1, :-1])) < 1e-3


def test_ice_call_and_step_only_enqueue(hipctx):
    """An ice call and a step go behind device work on the context's stream and return while it is still running; one
    synchronisation at the end (stream_end).  The device work: sb_get_dist_f64_dev calls on the stream's own grid with the
    widest window, on the context's stream, sized by measurement to outlast the two calls twenty times -- they also
    overwrite the context's scratch bit plane and its search radius hint under the stream's feet."""
    dt = np.float64
    nx, ny, k = GRIDS["WIDE"]
    lon, lat, maxdist = _regional(nx, ny, k, dt)
    land = _land(nx, ny, dt)
    planes = _planes(land, dt)
    st = synth.static_fields(nx, ny, dt)
    st.lon, st.lat, st.landfrac = lon, lat, land
    pres = (synth.pressure_1d(4, dt) / 100.0).astype(dt)
    th = [synth.theta_step(st, n + 1, dt) for n in range(2)]
    uv = [synth.wind_step(st, 4, n + 1, dt) for n in range(2)]
    kw = dict(timestep=120.0, maxdist=180.0)
    lib = hipctx.lib
    nbytes = nx * ny * 8
    dev = [C.c_void_p() for _ in range(3)]
    for p in dev:
        assert lib.sb_device_malloc(hipctx.h, C.c_size_t(nbytes), C.byref(p)) == 0
    try:
        coast = hipctx.get_edges(land, planes[8])
        hipctx.device_upload(dev[0].value, coast); hipctx.device_upload(dev[1].value, land)

        def filler(reps):
            for _ in range(reps):
                hipctx.get_dist_dev(dt, nx, ny, dev[0].value, dev[1].value, lon, lat, dev[2].value, maxdist=maxdist,
                                    kwin=hip.SB_DIST_MAX_WINDOW)

        def filler_ms(reps):
            hipctx.synchronize()
            t0 = time.perf_counter()
            filler(reps)
            hipctx.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        filler_ms(2)
        reps = int(min(2000, max(1, np.ceil(40.0 / max(filler_ms(20) / 20, 1e-3)))))
        busy = filler_ms(reps)

        def run(behind):
            zero = np.zeros_like(land)
            hipctx.stream_begin(st.z, st.sigma, zero, zero, zero, zero)
            hipctx.stream_coast(land, lon, lat, maxdist=maxdist)
            hipctx.stream_ice(planes[0])
            hipctx.stream_step(1, pres, th[0], uv[0][1], uv[0][0], None, **kw)
            hipctx.synchronize()
            if behind:
                filler(reps)
            t0 = time.perf_counter()
            hipctx.stream_ice(planes[6])
            hipctx.stream_step(2, pres, th[1], uv[1][1], uv[1][0], np.zeros(land.shape), **kw)
            t = 1e3 * (time.perf_counter() - t0)
            return t, hipctx.stream_end()

        t_enq, got = run(True)
        _, want = run(False)
        print(f"[enqueue-only] filler {busy:.2f} ms ({reps} x get_dist_dev), ice call + step enqueued in {t_enq:.3f} ms")
        assert busy >= 20.0 * t_enq, f"the two calls took {t_enq:.3f} ms behind {busy:.2f} ms of device work: they waited, or the run shows nothing"
        for a, b in zip(got, want):
            assert _same_bits(a, b)
    finally:
        hipctx.synchronize()
        for p in dev:
            lib.sb_device_free(hipctx.h, p)


def test_refused_calls_leave_the_stream_usable(hipctx):
    dt = np.float32
    nx, ny, k = GRIDS["BITS_SMALL"]
    lon, lat, maxdist = _regional(nx, ny, k, dt)
    land = _land(nx, ny, dt)
    planes = _planes(land, dt)
    zero = np.zeros_like(land)
    hipctx.stream_begin(zero, zero, zero, zero, zero, zero)
    with pytest.raises(hip.SeabreezeHipError, match=r"\(1\).*without sb_diag_stream_coast"):          # SB_ERR_ARG
        hipctx.stream_ice(planes[0])
    with pytest.raises(hip.SeabreezeHipError, match=r"\(1\)"):                                        # another precision
        hipctx.stream_coast(land, lon, lat, maxdist=maxdist, dtype=np.float64)
    with pytest.raises(hip.SeabreezeHipError, match=r"\(1\).*SB_DIST_MAX_WINDOW"):
        hipctx.stream_coast(land, lon, lat, maxdist=29.4 * (hip.SB_DIST_MAX_WINDOW + 2))
    hipctx.stream_coast(land, lon, lat, maxdist=maxdist)
    with pytest.raises(hip.SeabreezeHipError, match=r"\(1\)"):
        hipctx.stream_ice(planes[0], dtype=np.float64)
    hipctx.stream_ice(planes[3])
    _, want = _library_cdist(hipctx, land, planes[3], lon, lat, maxdist)
    assert _same_bits(hipctx.stream_get_cdist(), want)
    hipctx.stream_end()
    with pytest.raises(hip.SeabreezeHipError, match=r"\(1\)"):                                        # no stream any more
        hipctx.stream_ice(planes[0])
