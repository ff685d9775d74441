"""One tile of the UM's 2-D decomposition whose coast moves with the sea ice (sb_um_tile_coast_open_*, sb_um_tile_ice_*[_dev],
sb_um_tile_ice_report, sb_um_tile_coast_close; include/seabreeze_hip.h).

A whole domain is cut into tiles (tests/um_tile_ice_ref.py: CASES).  Whole-domain FRAMES of landfrac and of the twelve ice
planes of tests/um_ice_cases.py are built with a ghost width of at least the tiles'; every tile's frames are cut out of those
frames, so in-domain ghost cells are the neighbours' cells and out-of-domain ones the whole-domain ring.  Every tile has a
coast of its own on a context of its own; the planes go through them in order.  After every plane the interior of every
tile's cdist must equal -- `==`, cell for cell -- the tile's cells of sb_get_edges_um_*_dev + sb_get_dist_um_win_*_dev on the
whole domain on the same device (its layout halo differs from the window: the wide kernel), and the report must lie between
the brute-force count and the cap of tests/um_tile_ice_ref.py (both bounds are shown on the CPU in
tests/test_um_tile_ice_plan.py).  Coordinates beyond the domain are NaN: a source read there would show.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import enqueue_harness as eh
import um_ice_cases as uic
import um_ice_ref as uir
import um_setup_ref as ur
import um_tile_ice_ref as uti
import um_tile_ref as ut
import um_win_ref as uw
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

SENT = uw.SENTINEL
NCTX = 9


def _dt(prec):
    return np.float64 if prec == 8 else np.float32


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # (a copy: the cached inputs are read-only)


def _inner(f, h, nx, ny):
    return f[h[1]:h[1] + ny, h[0]:h[0] + nx]


def _ghosts_keep(frame, h, nx, ny, value=SENT):
    g = np.ones(frame.shape, bool)
    _inner(g, h, nx, ny)[...] = False
    return bool((frame[g] == value).all())


def _nan_pad(a, H):
    return np.ascontiguousarray(np.pad(a, ((H[1], H[1]), (H[0], H[0])), constant_values=np.nan))


@pytest.fixture(scope="module")
def tilectxs():
    cs = [hip.Context() for _ in range(NCTX)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def twinctx():
    c = hip.Context()
    yield c
    c.close()


class _Tile:
    """one tile's open coast on one context: resident frames of landfrac, icefrac and cdist on the device, cut out of the
    whole-domain frames (ghost width H) with the tile's ghost width h"""

    def __init__(self, ctx, tile, dom, win, H, h, lat_L, lon_L, lf_L, maxdist=180.0, incremental=True):
        self.ctx, self.tile, self.H, self.h, self.win, self.dt = ctx, tile, H, h, win, lf_L.dtype
        self.nx, self.ny = tile[1] - tile[0], tile[3] - tile[2]
        self.beyond = uti.beyond_of(tile, *dom)
        self.e = uti.sources(win, self.beyond)
        self.lf = _dev(uti.cut_frame(lf_L, tile, H, h))
        self.ci = torch.zeros_like(self.lf)
        self.cd = torch.full_like(self.lf, SENT)
        ctx.um_tile_coast_open(self.dt, self.nx, self.ny, *h, *win, self.beyond, uti.cut_frame(lat_L, tile, H, h),
                               uti.cut_frame(lon_L, tile, H, h), maxdist=maxdist, incremental=incremental)
        torch.cuda.synchronize()

    def ice(self, ci_L, stream=None):
        """-> cdist's frame, the report"""
        self.ci.copy_(_dev(uti.cut_frame(ci_L, self.tile, self.H, self.h)))
        torch.cuda.synchronize()
        self.ctx.um_tile_ice_dev(self.dt, self.lf.data_ptr(), self.ci.data_ptr(), self.cd.data_ptr(), stream=stream)
        rep = self.ctx.um_tile_ice_report()                       # (synchronises)
        return self.cd.cpu().numpy(), rep

    def interior(self, frame):
        return np.ascontiguousarray(_inner(frame, self.h, self.nx, self.ny))

    def of_whole(self, whole):
        x0, x1, y0, y1 = self.tile
        return np.ascontiguousarray(whole[y0:y1, x0:x1])

    def close(self):
        self.ctx.um_tile_coast_close()


def _whole(ctx, nx, ny, H, win, maxdist, land, lat, lon, lf_L, ci_L):
    """sb_get_edges_um_*_dev + sb_get_dist_um_win_*_dev on the whole domain's frames -> the interior.  The layout halo H
    differs from the window, so the distance kernel is the wide one."""
    assert not (win == H and max(win) <= 31)
    dt = lf_L.dtype
    dl, dc, dlf, dla, dlo = (_dev(a) for a in (lf_L, ci_L, land, lat, lon))
    co, cd = torch.zeros_like(dl), torch.zeros_like(dl)
    torch.cuda.synchronize()
    ctx.get_edges_um_dev(dt, nx, ny, *H, dl.data_ptr(), dc.data_ptr(), co.data_ptr())
    ctx.get_dist_um_win_dev(dt, nx, ny, *H, *win, co.data_ptr(), dlf.data_ptr(), dla.data_ptr(), dlo.data_ptr(), cd.data_ptr(),
                            maxdist=maxdist)
    ctx.synchronize()
    return np.ascontiguousarray(_inner(cd.cpu().numpy(), H, nx, ny)), np.ascontiguousarray(_inner(co.cpu().numpy(), H, nx, ny))


# ---- 1: twelve planes, every tile, both grids and precisions -----------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("grid", uic.GRIDS)
@pytest.mark.parametrize("case", sorted(uti.CASES))
def test_every_tile_follows_every_plane(tilectxs, twinctx, case, grid, prec):
    c, dt = uti.CASES[case], _dt(prec)
    nx, ny, win, maxdist = c["nx"], c["ny"], c["win"], c["maxdist"]
    H, land, lf_L, planes, co = uti.whole_inputs(case, prec)
    lat, lon = ur.grid_named(grid, nx, ny, dt)
    lat_L, lon_L = _nan_pad(lat, H), _nan_pad(lon, H)
    tiles = ut.tiles(c["cuts"])
    assert len(tiles) <= NCTX
    if case in "ab":
        assert any(0 < b < w for t in tiles for b, w in zip(uti.beyond_of(t, nx, ny), (win[0], win[0], win[1], win[1])))
    want = []
    for n, ci in enumerate(planes):
        w, coast = _whole(twinctx, nx, ny, H, win, maxdist, land, lat, lon, lf_L, ci)
        assert np.array_equal(coast, co[n]), "the whole-domain coast is not the numpy restatement's"
        want.append(w)
    assert (np.abs(want[3]) < 12000.0).any() and not np.array_equal(want[0], want[7])
    for inc in (True, False):
        # every tile's ghost width: the smallest that serves it, e* + 1, on one tile in three a cell more
        coasts = []
        for i, t in enumerate(tiles):
            e = uti.sources(win, uti.beyond_of(t, nx, ny))
            h = (min(max(e[0], e[1]) + 1 + (i % 3 == 0), H[0]), min(max(e[2], e[3]) + 1 + (i % 3 == 0), H[1]))
            coasts.append(_Tile(tilectxs[i], t, (nx, ny), win, H, h, lat_L, lon_L, lf_L, maxdist, incremental=inc))
        try:
            changed_calls = [0] * len(tiles)
            for n, ci in enumerate(planes):
                for i, b in enumerate(coasts):
                    frame, rep = b.ice(ci)
                    what = f"{case} {grid} fp{8 * prec} tile {b.tile} plane {uic.PLANES[n]} inc {int(inc)}"
                    assert _ghosts_keep(frame, b.h, b.nx, b.ny), f"{what}: ghost cells of cdist_l were written"
                    got, w = b.interior(frame), b.of_whole(want[n])
                    bad = int((got != w).sum())
                    assert bad == 0 and eh.same_bits(got, w), f"{what}: {bad} cells differ from the whole-domain field"
                    ntiles = uir.groups(b.ny) * uir.tiles(b.nx)
                    assert rep["calls"] == n + 1 and rep["tiles"] == ntiles
                    if not inc:
                        assert rep["changed_calls"] == -1 and rep["tiles_marked"] == ntiles
                        continue
                    if n == 0:
                        assert rep["tiles_marked"] == ntiles and rep["changed_calls"] == 0     # the first call computes everything
                        continue
                    changed = uti.changed_cells(co[n], co[n - 1], b.tile, b.e)
                    changed_calls[i] += 1 if changed else 0
                    assert rep["changed_calls"] == changed_calls[i], what     # (planes that leave every word alone are not counted)
                    lo = int(uti.brute_marks(b.nx, b.ny, win, changed).sum())
                    cap = int(uti.cap_marks(b.nx, b.ny, win, b.e, changed).sum())
                    assert lo <= rep["tiles_marked"] <= cap, (what, lo, rep["tiles_marked"], cap)
                    assert rep["tiles_marked"] == int(uti.word_marks(b.nx, b.ny, win, b.e, changed).sum()), what
                    assert (rep["tiles_marked"] > 0) == bool(changed)
            if inc:
                assert max(changed_calls) >= 4 and all(k <= 11 - len(uic.UNCHANGED) for k in changed_calls)
        finally:
            for b in coasts:
                b.close()


# ---- 2: km scale -------------------------------------------------------------------------------------------------------

def test_km_scale(tilectxs, twinctx):
    """um_tile_ref.ISLANDS: 300 x 250 at 0.0135 degrees, window 113, 2 x 2 cut.  Three planes: no ice, one iced cell of open
    sea -- an eighth islet, in one tile's interior and within the window of the other three --, no ice again."""
    c, dt = ut.ISLANDS, np.float64
    g = ut.islands_case()
    ny, nx = g["land"].shape
    win, maxdist = c["win"], c["maxdist"]
    H = (win[0] + 2, win[1] + 2)
    lf_L = ur.pad_edge(g["land"], *H)
    ice = np.zeros_like(lf_L)
    ice[H[1] + 130, H[0] + 160] = 0.6
    lat_L, lon_L = _nan_pad(g["lat"], H), _nan_pad(g["lon"], H)
    seq = [np.zeros_like(lf_L), ice, np.zeros_like(lf_L)]
    want = [_whole(twinctx, nx, ny, H, win, maxdist, g["land"], g["lat"], g["lon"], lf_L, ci)[0] for ci in seq[:2]]
    want.append(want[0])
    tiles = ut.tiles(c["cuts"])
    coasts = [_Tile(tilectxs[i], t, (nx, ny), win, H, (win[0] + 1, win[1] + 1), lat_L, lon_L, lf_L, maxdist) for i, t in enumerate(tiles)]
    moved = []
    try:
        for n, ci in enumerate(seq):
            for b in coasts:
                frame, rep = b.ice(ci)
                got, w = b.interior(frame), b.of_whole(want[n])
                assert eh.same_bits(got, w), (b.tile, n, int((got != w).sum()))
                if n:
                    assert 0 < rep["tiles_marked"] and rep["changed_calls"] == n
                if n == 1:
                    moved.append(not np.array_equal(got, b.of_whole(want[0])))
        # the tile that holds the islet, and at least one that sees it across a seam only
        assert moved[tiles.index((150, 300, 125, 250))] and sum(moved) >= 2, moved
    finally:
        for b in coasts:
            b.close()


# ---- 3: only marked workgroups are written -----------------------------------------------------------------------------

def test_only_marked_workgroups_are_written(tilectxs, twinctx):
    """um_tile_ice_ref.WRITTEN.  After the first call the test puts a sentinel into every interior cell outside the word
    model's cap -- the one deliberate breach of the contract -- and runs the next plane: the sentinel stands, every other
    cell holds the whole-domain field, the report lies between the brute-force count and the cap."""
    case, before, plane = uti.WRITTEN
    c, prec = uti.CASES[case], 8
    nx, ny, win = c["nx"], c["ny"], c["win"]
    H, land, lf_L, planes, co = uti.whole_inputs(case, prec)
    lat, lon = ur.grid_named("dateline", nx, ny, _dt(prec))
    lat_L, lon_L = _nan_pad(lat, H), _nan_pad(lon, H)
    want = _whole(twinctx, nx, ny, H, win, c["maxdist"], land, lat, lon, lf_L, planes[plane])[0]
    stood = 0
    for i, t in enumerate(ut.tiles(c["cuts"])):
        b = _Tile(tilectxs[i], t, (nx, ny), win, H, H, lat_L, lon_L, lf_L)
        try:
            b.ice(planes[before])
            changed = uti.changed_cells(co[before], co[plane], t, b.e)
            capm = uti.cap_marks(b.nx, b.ny, win, b.e, changed)
            cap = uir.cells_of_marks(capm, b.nx, b.ny)
            lo = int(uti.brute_marks(b.nx, b.ny, win, changed).sum())
            inner = _inner(b.cd, b.h, b.nx, b.ny)
            inner[torch.from_numpy(~cap).cuda()] = -3.25
            torch.cuda.synchronize()
            frame, rep = b.ice(planes[plane])
            got = b.interior(frame)
            assert (got[~cap] == -3.25).all(), f"{t}: {int((got[~cap] != -3.25).sum())} cells outside the cap were written"
            assert eh.same_bits(np.ascontiguousarray(got[cap]), np.ascontiguousarray(b.of_whole(want)[cap])), t
            assert lo <= rep["tiles_marked"] <= int(capm.sum()), (t, lo, rep["tiles_marked"], int(capm.sum()))
            assert (rep["tiles_marked"] > 0) == bool(changed) and _ghosts_keep(frame, b.h, b.nx, b.ny)
            stood += int((~cap).sum())
        finally:
            b.close()
    assert stood > 0


# ---- 4: the seam itself ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
def test_a_flip_beyond_the_seam(hipctx, twinctx, prec):
    """All sea, 200 x 70, window 15, the middle tile (67, 134, 23, 46) with a halo of 17.  An iced cell two cells beyond the
    source rectangle -- the halo holds it -- marks nothing; one more in the neighbour's column exactly 15 cells beyond the west
    side moves interior cells of this tile and is counted."""
    dt, nx, ny, win, H, t = _dt(prec), 200, 70, (15, 15), (17, 17), (67, 134, 23, 46)
    lat, lon = ur.grid_named("polar", nx, ny, dt)
    lat_L, lon_L = _nan_pad(lat, H), _nan_pad(lon, H)
    land, lf_L = np.zeros((ny, nx), dt), np.zeros((ny + 2 * H[1], nx + 2 * H[0]), dt)
    none, far, near = (np.zeros_like(lf_L) for _ in range(3))
    far[H[1] + 30, H[0] + 67 - 17] = 0.6                          # frame column 0 of the tile: two cells beyond the rectangle
    near[...] = far
    near[H[1] + 30, H[0] + 67 - 15] = 0.6                         # the rectangle's first column
    want = [_whole(twinctx, nx, ny, H, win, 180.0, land, lat, lon, lf_L, ci)[0] for ci in (none, far, near)]
    b = _Tile(hipctx, t, (nx, ny), win, H, H, lat_L, lon_L, lf_L)
    try:
        assert b.e == (15, 15, 15, 15)
        f0, _ = b.ice(none)
        f1, r1 = b.ice(far)
        assert r1["tiles_marked"] == 0 and r1["changed_calls"] == 0
        f2, r2 = b.ice(near)
        assert r2["tiles_marked"] > 0 and r2["changed_calls"] == 1
        for f, w in zip((f0, f1, f2), want):
            assert eh.same_bits(b.interior(f), b.of_whole(w))
        assert (b.interior(f0) >= 12000.0).all() and np.array_equal(b.interior(f0), b.interior(f1))
        moved = b.interior(f2) != b.interior(f1)
        assert moved[:, 0].any() and not moved[:, 2:].any(), "the source 15 cells beyond the side reaches interior column 0"
    finally:
        b.close()


# ---- 5: other coast calls in between -----------------------------------------------------------------------------------

def test_other_coast_calls_in_between(hipctx, twinctx):
    """Between two ice calls the same context runs tile_get_dist_um and get_dist_um_win on another mask (both overwrite the
    scratch UM bit plane): the next ice call is exact."""
    case, prec = "a", 8
    c, dt = uti.CASES[case], _dt(prec)
    nx, ny, win = c["nx"], c["ny"], c["win"]
    H, land, lf_L, planes, co = uti.whole_inputs(case, prec)
    lat, lon = ur.grid_named("polar", nx, ny, dt)
    lat_L, lon_L = _nan_pad(lat, H), _nan_pad(lon, H)
    t = ut.tiles(c["cuts"])[4]
    b = _Tile(hipctx, t, (nx, ny), win, H, H, lat_L, lon_L, lf_L)
    try:
        frame, _ = b.ice(planes[3])
        assert eh.same_bits(b.interior(frame), b.of_whole(_whole(twinctx, nx, ny, H, win, 180.0, land, lat, lon, lf_L, planes[3])[0]))
        oland, oice = ur.noise_mask(nx, ny, 11, dt)
        _, _, ocoast = ur.coast_of(oland, oice, *H)
        other = hipctx.get_dist_um_win(ocoast, oland, lat, lon, *H, *win)
        assert (np.abs(_inner(other, H, nx, ny)) < 12000.0).any()
        fr = lambda a: uti.cut_frame(a, t, H, H)
        tile_other = hipctx.tile_get_dist_um(fr(ocoast), fr(ur.pad_edge(oland, *H)), fr(ur.pad_edge(lat, *H)), fr(ur.pad_edge(lon, *H)),
                                             *H, *win, ut.sides_of(t, nx, ny))
        assert (np.abs(_inner(tile_other, H, b.nx, b.ny)) < 12000.0).any()
        for n in (8, 9, 10):
            frame, rep = b.ice(planes[n])
            w = _whole(twinctx, nx, ny, H, win, 180.0, land, lat, lon, lf_L, planes[n])[0]
            assert eh.same_bits(b.interior(frame), b.of_whole(w)), uic.PLANES[n]
            assert 0 < rep["tiles_marked"]
    finally:
        b.close()


# ---- 6: seabreeze_diag_um steps with ice calls between them ------------------------------------------------------------

def test_tile_steps_follow_the_ice():
    """The middle tile of case a's cut, 124 x 23 x 4 with halo 16 under a 15-cell window -- its west side lies 10 cells from
    the domain's edge --, four steps, an ice call ahead of steps 1, 2 and 4; cdist's ghost cells are edge-replicated after
    every ice call.  The twin steps on a mask made by tile_get_edges_um + tile_get_dist_um at every step on a fresh context,
    with the coast beyond the domain's end zeroed between the two as those calls ask of their caller (plane 8 holds a coast
    cell there).  Masks, outputs and state: bit for bit."""
    dt, nz, win, h, t, dom = np.float64, 4, (15, 15), 16, (10, 134, 23, 46), (200, 70)
    nx, ny = t[1] - t[0], t[3] - t[2]
    H = (h, h)
    land, lf_L, planes = uic.make(*dom, H, dt)
    lat, lon = ur.grid_named("dateline", *dom, dt)
    fr = lambda a: uti.cut_frame(a, t, H, H)
    lf_l, lat_l, lon_l = fr(lf_L), fr(ur.pad_edge(lat, *H)), fr(ur.pad_edge(lon, *H))
    ices = [fr(p) for p in planes]
    ice_of_step = {1: ices[0], 2: ices[7], 3: ices[7], 4: ices[10]}
    core = (slice(h, h + ny), slice(h, h + nx))
    st = synth.static_fields(nx + 2 * h, ny + 2 * h, dt)                   # a bigger field whose rim serves as ghosts
    p = synth.pressure_3d(st, nz, dt)[:, core[0], core[1]].copy()
    flags = hip.SB_UM_THETA_TO_T0 | hip.SB_UM_LEVEL_WALK
    beyond, sides = uti.beyond_of(t, *dom), ut.sides_of(t, *dom)
    assert sides == 0

    def fresh_mask(ci):
        c = hip.Context()
        try:
            coast = c.tile_get_edges_um(lf_l, ci, h, h, *win, sides, out=np.zeros_like(lf_l))
            coast[~ut.in_domain(t, *dom, h, h, *win)] = 0.0
            return c.tile_get_dist_um(coast, lf_l, lat_l, lon_l, h, h, *win, sides, out=np.zeros_like(lf_l))
        finally:
            c.close()

    def run(ice_path):
        ctx = hip.Context()
        try:
            ctx.set_plan_cache(True)
            if ice_path:
                ctx.um_tile_coast_open(dt, nx, ny, h, h, *win, beyond, lat_l, lon_l)
            cd = np.zeros_like(lf_l)
            state = [np.zeros((ny, nx), dt) for _ in range(4)]
            out, masks, counters, last = [], [], [], None
            for tn in (1, 2, 3, 4):
                ci = ice_of_step[tn]
                if ci is not last:
                    cd = ctx.um_tile_ice(lf_l, ci, cd) if ice_path else fresh_mask(ci)
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
                assert ctx.um_tile_ice_report()["changed_calls"] == 2
                ctx.um_tile_coast_close()
            return out, masks, counters
        finally:
            ctx.close()

    got, gm, gc = run(True)
    want, wm, wc = run(False)
    assert not np.array_equal(gm[0], gm[1]) and not np.array_equal(gm[2], gm[3]), "the ice calls left the mask alone"
    for tn in range(4):
        assert eh.same_bits(gm[tn], wm[tn]), f"step {tn + 1}: mask frames differ"
        for nm, a, w in zip(("ws", "wd", "thc", "sb_con"), got[tn], want[tn]):
            assert eh.same_bits(a, w), (f"step {tn + 1}", nm, int((a != w).sum()))
    assert gc == wc and all(c["band_cells"] > 0 for c in gc), "no band cell: the steps show nothing"


# ---- 7: enqueue only ---------------------------------------------------------------------------------------------------

def test_ice_calls_only_enqueue():
    """The ice calls go behind device work on a caller's stream (tests/enqueue_harness.py's layout: the filler, the ice frame
    copied in place, the call, a snapshot) and return while the filler is still running; one synchronisation at the end.
    The twin: the same sequence, synchronised after every call, on a fresh context."""
    case, dt = "a", np.float64
    c = uti.CASES[case]
    nx, ny, win = c["nx"], c["ny"], c["win"]
    H, land, lf_L, planes, co = uti.whole_inputs(case, 8)
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    t = ut.tiles(c["cuts"])[4]
    tnx, tny, beyond = t[1] - t[0], t[3] - t[2], uti.beyond_of(t, nx, ny)
    fr = lambda a: uti.cut_frame(a, t, H, H)
    lat_l, lon_l = fr(_nan_pad(lat, H)), fr(_nan_pad(lon, H))
    seq = [fr(planes[n]) for n in (0, 3, 8, 10, 11)]
    filler = eh.Filler()
    s = torch.cuda.Stream()

    def run(busy):
        ctx = hip.Context()
        try:
            ctx.um_tile_coast_open(dt, tnx, tny, *H, *win, beyond, lat_l, lon_l)
            lf, ci_all = _dev(fr(lf_L)), torch.stack([_dev(x) for x in seq])
            ci = _dev(fr(planes[5]))                              # a valid frame that is not in the sequence
            cd = torch.full_like(lf, SENT)
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
                    ctx.um_tile_ice_dev(dt, lf.data_ptr(), ci.data_ptr(), cd.data_ptr(), stream=s.cuda_stream)
                    t_enq.append(time.perf_counter() - t0)
                    if busy:
                        after[n] = not ev[n].query()
                    hist[n].copy_(cd)
                    if not busy:
                        s.synchronize(); ctx.synchronize()
            s.synchronize()
            rep = ctx.um_tile_ice_report()
            ctx.um_tile_coast_close()
            return [a.cpu().numpy() for a in hist], before, after, rep, t_enq
        finally:
            ctx.close()

    got, before, after, rep, t_enq = run(True)
    want, _, _, rep_w, _ = run(False)
    print(f"[enqueue-only] um tile ice: filler {filler.ms:.2f} ms, host enqueue per call (ms) {[round(1e3 * x, 3) for x in t_enq]}")
    if not all(before[1:]):
        raise eh.VacuousRun(f"the filler had finished before the calls were made: {before}")
    assert all(after[1:]), f"a call returned only after the filler ahead of it had finished -- a hidden synchronisation: {after}"
    eh.check_ratio(filler, float(np.median(t_enq[1:])), "um tile ice")
    for n in range(len(seq)):
        assert eh.same_bits(got[n], want[n]), f"call {n + 1}"
    assert rep == rep_w and rep["calls"] == len(seq) and rep["changed_calls"] == len(seq) - 1
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[2], got[3])


# ---- 8: the host form --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
def test_host_form(hipctx, prec):
    """um_tile_ice on numpy frames equals the _dev form's interior; the ghost cells of cdist_l are untouched"""
    case = "b"
    c, dt = uti.CASES[case], _dt(prec)
    nx, ny, win = c["nx"], c["ny"], c["win"]
    H, land, lf_L, planes, co = uti.whole_inputs(case, prec)
    lat, lon = ur.grid_named("polar", nx, ny, dt)
    lat_L, lon_L = _nan_pad(lat, H), _nan_pad(lon, H)
    t = ut.tiles(c["cuts"])[4]                                    # 13 x 9, 6 < 9 rows to the domain's edge
    b = _Tile(hipctx, t, (nx, ny), win, H, H, lat_L, lon_L, lf_L)
    try:
        assert (b.nx, b.ny) == (13, 9) and b.e[2] == 6
        dev = [b.ice(planes[n])[0] for n in (0, 3, 7, 8)]
    finally:
        b.close()
    fr = lambda a: uti.cut_frame(a, t, H, H)
    lf_l = fr(lf_L)
    hipctx.um_tile_coast_open(dt, b.nx, b.ny, *H, *win, b.beyond, fr(lat_L), fr(lon_L))
    try:
        cd = np.full(lf_l.shape, SENT, dt)
        for k, n in enumerate((0, 3, 7, 8)):
            assert hipctx.um_tile_ice(lf_l, fr(planes[n]), cd) is cd
            assert _ghosts_keep(cd, H, b.nx, b.ny), "ghost cells of cdist_l were written"
            assert eh.same_bits(b.interior(cd), b.interior(dev[k])), uic.PLANES[n]
        assert hipctx.um_tile_ice_report()["calls"] == 4
        with pytest.raises(ValueError):
            hipctx.um_tile_ice(lf_l[1:], fr(planes[0]), cd)
    finally:
        hipctx.um_tile_coast_close()
    with pytest.raises(hip.SeabreezeHipError, match="without um_tile_coast_open"):
        hipctx.um_tile_ice(lf_l, fr(planes[0]), cd)


# ---- 9: a UM coast and a UM tile coast on one context ------------------------------------------------------------------

def test_um_coast_and_tile_coast_side_by_side(hipctx, twinctx):
    """Both are open on one context at once and their calls alternate: the tile coast gives the whole-domain field, the UM
    coast the interior-only field of the same tile -- which differs from it."""
    case, prec = "a", 8
    c, dt = uti.CASES[case], _dt(prec)
    nx, ny, win = c["nx"], c["ny"], c["win"]
    H, land, lf_L, planes, co = uti.whole_inputs(case, prec)
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    lat_L, lon_L = _nan_pad(lat, H), _nan_pad(lon, H)
    t = ut.tiles(c["cuts"])[4]
    x0, x1, y0, y1 = t
    b = _Tile(hipctx, t, (nx, ny), win, H, H, lat_L, lon_L, lf_L)
    hipctx.um_coast_open(dt, b.nx, b.ny, *H, *win, lat[y0:y1, x0:x1], lon[y0:y1, x0:x1])
    try:
        cd_um = torch.full_like(b.cd, SENT)
        differs = 0
        for n in (0, 3, 7, 8, 10):
            frame, _ = b.ice(planes[n])
            hipctx.um_ice_dev(dt, b.lf.data_ptr(), b.ci.data_ptr(), cd_um.data_ptr())
            hipctx.synchronize()
            w = _whole(twinctx, nx, ny, H, win, 180.0, land, lat, lon, lf_L, planes[n])[0]
            assert eh.same_bits(b.interior(frame), b.of_whole(w)), uic.PLANES[n]
            own = ut.cut(co[n], *t, *H, 0.0)                       # the interior-only rule: the tile's own coast cells
            own[~ut.in_domain(t, nx, ny, *H, 0, 0)] = 0.0
            um_want = twinctx.get_dist_um_win(own, np.ascontiguousarray(land[y0:y1, x0:x1]), np.ascontiguousarray(lat[y0:y1, x0:x1]),
                                              np.ascontiguousarray(lon[y0:y1, x0:x1]), *H, *win)
            got_um = b.interior(cd_um.cpu().numpy())
            assert eh.same_bits(got_um, b.interior(um_want)), uic.PLANES[n]
            differs += int(not np.array_equal(got_um, b.interior(frame)))
        assert differs > 0
        assert hipctx.um_ice_report()["calls"] == 5 == hipctx.um_tile_ice_report()["calls"]
    finally:
        hipctx.um_coast_close()
        b.close()


# ---- 10: refusals ------------------------------------------------------------------------------------------------------

def test_refused_calls():
    dt, nx, ny, hi, hj, wi, wj = np.float64, 70, 12, 10, 5, 9, 4
    beyond = (30, 5, 0, 20)                                       # e* = 9, 5, 0, 4
    shape = (ny + 2 * hj, nx + 2 * hi)
    lat = np.full(shape, -35.0, dt) + 0.1 * np.arange(shape[0])[:, None]
    lon = np.full(shape, 170.0, dt) + 0.1 * np.arange(shape[1])[None, :]
    ctx = hip.Context()
    lib, I = ctx.lib, C.c_int
    SB_ERR_ARG = 1
    f = torch.zeros(shape, dtype=torch.float64, device="cuda")
    f32 = torch.zeros(shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def open_(nx_=nx, ny_=ny, hi_=hi, hj_=hj, wi_=wi, wj_=wj, b_=beyond, lat_=lat, lon_=lon, h=ctx.h):
        b = (C.c_int * 4)(*b_) if b_ is not None else None
        return lib.sb_um_tile_coast_open_f64(h, I(nx_), I(ny_), I(hi_), I(hj_), I(wi_), I(wj_), b, hip._p(lat_), hip._p(lon_),
                                             C.c_double(180.0), I(1))

    def ice(fn, a, b, c):
        return fn(ctx.h, hip._p(a), hip._p(b), hip._p(c), None)

    def refused(rc):
        return rc == SB_ERR_ARG and len(lib.sb_last_error(ctx.h)) > 0

    # what a served call must give: no ice over an empty land -- no coast anywhere --, or one iced ghost cell west of the
    # interior, inside the source rectangle -- an island across the seam
    g = f.clone()
    g[hj + 5, hi - 4] = 0.6
    other = hip.Context()
    coast = other.tile_get_edges_um(np.zeros(shape, dt), g.cpu().numpy(), hi, hj, wi, wj, 4, out=np.zeros(shape, dt))
    island = other.tile_get_dist_um(coast, np.zeros(shape, dt), lat, lon, hi, hj, wi, wj, 4, out=np.zeros(shape, dt))
    other.close()
    assert (np.abs(_inner(island, (hi, hj), nx, ny)) < 12000.0).any()
    cd = torch.full_like(f, SENT)
    turn = [0]

    def serves():
        """the open coast serves a correct ice call: the island and the empty sea take turns, so every call changes the coast"""
        turn[0] += 1
        ctx.um_tile_ice_dev(dt, f.data_ptr(), (g if turn[0] & 1 else f).data_ptr(), cd.data_ptr())
        ctx.synchronize()
        out = cd.cpu().numpy()
        want = _inner(island, (hi, hj), nx, ny) if turn[0] & 1 else np.full((ny, nx), 12000.0)
        return _ghosts_keep(out, (hi, hj), nx, ny) and bool(np.array_equal(_inner(out, (hi, hj), nx, ny), want))

    try:
        rep = (C.c_longlong * 4)()
        assert refused(ice(lib.sb_um_tile_ice_f64_dev, f.data_ptr(), f.data_ptr(), cd.data_ptr()))          # not open
        assert b"without sb_um_tile_coast_open" in lib.sb_last_error(ctx.h)
        ctx.synchronize()
        assert bool((cd == SENT).all().item()), "a refused call wrote cdist_l"
        assert refused(lib.sb_um_tile_ice_report(ctx.h, rep)) and refused(lib.sb_um_tile_coast_close(ctx.h))
        host = np.zeros(shape, dt)
        hcd = np.full(shape, SENT, dt)
        assert refused(lib.sb_um_tile_ice_f64(ctx.h, hip._p(host), hip._p(host), hip._p(hcd))) and (hcd == SENT).all()
        bad = (dict(nx_=0), dict(ny_=0), dict(nx_=-3), dict(wi_=-1), dict(wj_=-1), dict(wi_=hip.SB_DIST_UM_MAX_WINDOW + 1),
               dict(wj_=hip.SB_DIST_UM_MAX_WINDOW + 1), dict(b_=(-1, 5, 0, 20)), dict(b_=(30, 5, 0, -7)), dict(b_=None),
               dict(hi_=9), dict(hj_=4),                          # below e* + 1: west needs 10, north 5
               dict(hj_=0, wj_=0), dict(hi_=0, wi_=0),            # below 1: the ring of an edge side, of a side without a window
               dict(lat_=None), dict(lon_=None))
        for kw in bad:
            assert refused(open_(**kw)), kw
            assert refused(lib.sb_um_tile_ice_report(ctx.h, rep)), ("a refused open left a coast open", kw)
            assert open_() == 0 and serves(), ("after", kw)       # ... and the context still serves a correct ice call
            assert lib.sb_um_tile_coast_close(ctx.h) == 0
        assert open_(h=None) == SB_ERR_ARG and len(lib.sb_last_error(None)) > 0
        assert open_() == 0
        assert refused(open_())                                   # open twice
        assert b"already open" in lib.sb_last_error(ctx.h)
        assert serves()
        assert refused(ice(lib.sb_um_tile_ice_f32_dev, f32.data_ptr(), f32.data_ptr(), f32.data_ptr()))     # the other precision
        assert b"other precision" in lib.sb_last_error(ctx.h)
        assert refused(lib.sb_um_tile_ice_f32(ctx.h, hip._p(host), hip._p(host), hip._p(host)))
        assert serves()
        for args in ((None, f.data_ptr(), cd.data_ptr()), (f.data_ptr(), None, cd.data_ptr()), (f.data_ptr(), f.data_ptr(), None)):
            last = cd.clone()
            n_before = ctx.um_tile_ice_report()["calls"]
            assert refused(ice(lib.sb_um_tile_ice_f64_dev, *args)), args
            ctx.synchronize()
            assert torch.equal(cd, last) and ctx.um_tile_ice_report()["calls"] == n_before, "a refused call wrote cdist_l or counted"
            assert serves()
        assert refused(lib.sb_um_tile_ice_report(ctx.h, None))
        assert lib.sb_um_tile_ice_report(ctx.h, rep) == 0 and rep[0] >= 1 and rep[3] == uir.groups(ny) * uir.tiles(nx)
        ctx.um_tile_coast_close()
        with pytest.raises(hip.SeabreezeHipError, match=r"\(1\).*without sb_um_tile_coast_open"):
            ctx.um_tile_ice_dev(dt, f.data_ptr(), f.data_ptr(), f.data_ptr())
    finally:
        ctx.close()
