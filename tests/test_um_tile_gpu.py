"""sb_tile_get_edges_um_* / sb_tile_get_dist_um_*: the UM-layout coast setup on one tile of a 2-D domain decomposition.
A whole domain is cut into tiles here; every tile's frames are cut out of the whole fields (tests/um_tile_ref.py: cut, in
the role of swap_bounds), the tile calls run per tile, and the interiors must equal the tile's cells of the whole-domain
sb_get_edges_um_* + sb_get_dist_um_win_* on the same device BIT FOR BIT -- the whole-domain call is made with a layout halo
that differs from the window, so that it takes the kernel whose arithmetic the tile kernel shares.  That the inputs cannot
pass on interior sources, and hold reset cells, is shown on the CPU (tests/test_um_tile_host.py).

Out-of-domain ghost cells of the frames hold values that would show if they were read: a coast of 5 (a source, were it
one), NaN coordinates and land fractions."""
import numpy as np
import pytest
import torch

import um_setup_ref as ur
import um_tile_ref as ut
import um_win_ref as uw
from seabreeze_param_amd import hip

pytestmark = pytest.mark.gpu

SENT = uw.SENTINEL


def _dt(prec):
    return np.float64 if prec == 8 else np.float32


def _frames(case, tile, halo, coast_fill=5.0):
    """coast, land, lat, lon frames of a tile, cut from the whole domain's interior fields"""
    c = lambda a, fill: ut.cut(a, *tile, *halo, fill)
    return c(case["coast"], coast_fill), c(case["land"], np.nan), c(case["lat"], np.nan), c(case["lon"], np.nan)


def _whole(ctx, case, win, maxdist):
    """the whole-domain field (interior) from the wide kernel: layout halo 1 differs from every window used here"""
    key = (id(case), win, maxdist)
    if key not in _whole.memo:
        coast_l = np.ascontiguousarray(np.pad(case["coast"], 1))
        f = ctx.get_dist_um_win(coast_l, case["land"], case["lat"], case["lon"], 1, 1, *win, maxdist=maxdist)
        _whole.memo[key] = (case, np.ascontiguousarray(f[1:-1, 1:-1]))       # (the case is kept: its id stays its own)
    return _whole.memo[key][1]


_whole.memo = {}


def _check_tiles(ctx, case, cuts, halo, win, maxdist, dt):
    whole = _whole(ctx, case, win, maxdist)
    ny, nx = whole.shape
    hi, hj = halo
    for t in ut.tiles(cuts):
        x0, x1, y0, y1 = t
        coast_f, land_f, lat_f, lon_f = _frames(case, t, halo)
        out = uw.sentinel_field(coast_f.shape, dt, hi, hj)
        got = ctx.tile_get_dist_um(coast_f, land_f, lat_f, lon_f, hi, hj, *win, ut.sides_of(t, nx, ny), maxdist=maxdist,
                                   out=out.copy())
        ghost = out == SENT
        assert got.dtype == dt and np.array_equal(got[ghost], out[ghost]), f"{t}: ghost cells of cdist_l were written"
        inner = got[hj:hj + y1 - y0, hi:hi + x1 - x0]
        bad = np.count_nonzero(inner != whole[y0:y1, x0:x1])
        assert bad == 0, f"tile {t}: {bad} cells differ from the whole-domain field"
    return whole


# ---- 1: sparse coasts, wide window -------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("cuts", sorted(ut.SPARSE_CUTS))
def test_sparse_coasts_under_a_wide_window(hipctx, cuts, prec):
    """"west" 200 x 30, window 40 x 9, frames with halo 41 x 10: sources beyond the seam, and beyond the neighbouring tile"""
    c = ut.SPARSE
    whole = _check_tiles(hipctx, ut.sparse_case(prec), ut.SPARSE_CUTS[cuts], c["halo"], c["win"], c["maxdist"], _dt(prec))
    assert (whole >= 12000.0).any() and (np.abs(whole) < 12000.0).any()


# ---- 2: edges and distance in a chain on dense coasts ------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("halo", ut.DENSE["halos"])
@pytest.mark.parametrize("grid", sorted(ur.GRIDS))
def test_chain_on_dense_coasts(hipctx, grid, halo, prec):
    """150 x 22 with ice, window 6 x 5, 3 x 3 cut: tile_get_edges_um(ext = win) on frames cut from the edge-padded whole
    fields, then tile_get_dist_um on the coast it wrote"""
    c, dt, g = ut.DENSE, _dt(prec), ut.dense_case(grid, prec)
    nx, ny, (hi, hj), win = c["nx"], c["ny"], halo, c["win"]
    lf_w, ci_w = ur.pad_edge(g["land"], hi, hj), ur.pad_edge(g["ice"], hi, hj)
    lat_w, lon_w = ur.pad_edge(g["lat"], hi, hj), ur.pad_edge(g["lon"], hi, hj)
    coast_w = hipctx.get_edges_um(ur.pad_edge(g["land"], 1, 1), ur.pad_edge(g["ice"], 1, 1), 1, 1)
    assert np.array_equal(coast_w[1:-1, 1:-1], g["coast"])
    cd_w = hipctx.get_dist_um_win(coast_w, g["land"], g["lat"], g["lon"], 1, 1, *win, maxdist=c["maxdist"])[1:-1, 1:-1]
    for t in ut.tiles(c["cuts"]):
        x0, x1, y0, y1 = t
        fr = lambda a: np.ascontiguousarray(a[y0:y1 + 2 * hj, x0:x1 + 2 * hi])
        sides = ut.sides_of(t, nx, ny)
        coast_f = hipctx.tile_get_edges_um(fr(lf_w), fr(ci_w), hi, hj, *win, sides, out=np.full(fr(lf_w).shape, SENT, dt))
        want = ut.tile_edges(g["coast"], t, hi, hj, *win, SENT)
        assert np.array_equal(coast_f, want), f"{t}: coast differs, or a cell beyond ext / outside the domain was written"
        out = uw.sentinel_field(coast_f.shape, dt, hi, hj)
        got = hipctx.tile_get_dist_um(coast_f, fr(lf_w), fr(lat_w), fr(lon_w), hi, hj, *win, sides, maxdist=c["maxdist"],
                                      out=out.copy())
        assert np.array_equal(got[out == SENT], out[out == SENT])
        assert np.array_equal(got[hj:hj + y1 - y0, hi:hi + x1 - x0], cd_w[y0:y1, x0:x1]), t


# ---- 3: km scale -------------------------------------------------------------------------------------------------------

def test_seven_islands_at_km_scale(hipctx):
    """300 x 250 at 0.0135 degrees, window 113, halo 114, 2 x 2 cut: four passes of the row staging"""
    c = ut.ISLANDS
    whole = _check_tiles(hipctx, ut.islands_case(), c["cuts"], c["halo"], c["win"], c["maxdist"], np.float64)
    assert (whole >= 12000.0).any() and (np.abs(whole) < 12000.0).any()


# ---- 4: degenerate and in-place forms ----------------------------------------------------------------------------------

def _whole_domain_frames(prec, h):
    g = ut.dense_case("dateline", prec)
    pad = lambda a: ur.pad_edge(a, h, h)
    coast_f = np.ascontiguousarray(np.pad(g["coast"], h))
    return g, coast_f, pad(g["land"]), pad(g["ice"]), pad(g["lat"]), pad(g["lon"])


@pytest.mark.parametrize("prec", [8, 4])
def test_all_four_sides_at_the_edge_is_the_whole_domain(hipctx, prec):
    """halo 3, window 6, sides = 15: sb_get_dist_um_win's field bit for bit (its wide kernel: the window differs from the
    halo); nothing beyond the interior is a source although the window reaches past the ghost cells"""
    h, win = 3, (6, 6)
    g, coast_f, land_f, _, lat_f, lon_f = _whole_domain_frames(prec, h)
    ref = hipctx.get_dist_um_win(coast_f, g["land"], g["lat"], g["lon"], h, h, *win)
    coast_f[:h] = coast_f[-h:] = 5.0                              # (ghost cells that would be sources, were they read)
    coast_f[:, :h] = coast_f[:, -h:] = 5.0
    got = hipctx.tile_get_dist_um(coast_f, land_f, lat_f, lon_f, h, h, *win, 15)
    assert np.array_equal(got, ref)


def test_in_place(hipctx):
    """cdist_l is coast_l"""
    c, g = ut.SPARSE, ut.sparse_case(8)
    t = ut.GHOST_ONLY_TILE
    sides = ut.sides_of(t, c["nx"], c["ny"])
    coast_f, land_f, lat_f, lon_f = _frames(g, t, c["halo"])
    ref = hipctx.tile_get_dist_um(coast_f, land_f, lat_f, lon_f, *c["halo"], *c["win"], sides)
    field = coast_f.copy()
    got = hipctx.tile_get_dist_um(field, land_f, lat_f, lon_f, *c["halo"], *c["win"], sides, out=field)
    hi, hj = c["halo"]
    x0, x1, y0, y1 = t
    core = (slice(hj, hj + y1 - y0), slice(hi, hi + x1 - x0))
    assert got is field and np.array_equal(field[core], ref[core])
    ghost = np.ones(field.shape, bool)
    ghost[core] = False
    assert np.array_equal(field[ghost], coast_f[ghost])
    assert np.array_equal(ref[core], _whole(hipctx, g, c["win"], c["maxdist"])[y0:y1, x0:x1])


@pytest.mark.parametrize("prec", [8, 4])
def test_dev_forms_on_a_torch_stream(hipctx, prec):
    """tile_get_edges_um_dev -> tile_get_dist_um_dev on a non-default torch stream, behind device-side copies that fill
    their inputs on that stream, no synchronisation in between: the host forms' fields"""
    c, dt, g = ut.DENSE, _dt(prec), ut.dense_case("polar", prec)
    (hi, hj), win, t = c["halos"][0], c["win"], ut.tiles(c["cuts"])[4]
    x0, x1, y0, y1 = t
    nxt, nyt, sides = x1 - x0, y1 - y0, ut.sides_of(t, c["nx"], c["ny"])
    assert sides == 0
    fr = lambda a: np.ascontiguousarray(ur.pad_edge(a, hi, hj)[y0:y1 + 2 * hj, x0:x1 + 2 * hi])
    lf, ci, la, lo = fr(g["land"]), fr(g["ice"]), fr(g["lat"]), fr(g["lon"])
    coast_ref = hipctx.tile_get_edges_um(lf, ci, hi, hj, *win, sides, out=np.full(lf.shape, SENT, dt))
    cd_ref = hipctx.tile_get_dist_um(coast_ref, lf, la, lo, hi, hj, *win, sides, out=np.full(lf.shape, SENT, dt))
    src = [torch.from_numpy(a).to("cuda") for a in (lf, ci, la, lo)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sh = s.cuda_stream
        dl, dc, dla, dlo = (torch.empty_like(a).copy_(a) for a in src)      # device-side fills, on the stream
        co = torch.full_like(dl, SENT)
        cd = torch.full_like(dl, SENT)
        hipctx.tile_get_edges_um_dev(dt, nxt, nyt, hi, hj, *win, sides, dl.data_ptr(), dc.data_ptr(), co.data_ptr(), stream=sh)
        hipctx.tile_get_dist_um_dev(dt, nxt, nyt, hi, hj, *win, sides, co.data_ptr(), dl.data_ptr(), dla.data_ptr(),
                                    dlo.data_ptr(), cd.data_ptr(), stream=sh)
    s.synchronize()
    assert np.array_equal(co.cpu().numpy(), coast_ref)
    assert np.array_equal(cd.cpu().numpy(), cd_ref)
    assert (np.abs(cd_ref[hj:hj + nyt, hi:hi + nxt]) < 12000.0).any()


# ---- 5: refusals -------------------------------------------------------------------------------------------------------

def _refused(call, out):
    before = out.copy()
    with pytest.raises(hip.SeabreezeHipError) as err:
        call()
    assert "failed (1)" in str(err.value), str(err.value)          # SB_ERR_ARG
    assert np.array_equal(out, before, equal_nan=True), "a refused call wrote its output"


def test_refusals(hipctx):
    dt, nx, ny, h = np.float64, 20, 12, 4
    shape = (ny + 2 * h, nx + 2 * h)
    lf, ci = np.zeros(shape, dt), np.zeros(shape, dt)
    lf[:, : shape[1] // 2] = 1.0
    la, lo = np.full(shape, 10.0, dt), np.full(shape, 20.0, dt)
    out = np.full(shape, SENT, dt)
    ctx = hipctx
    edges = lambda hi, hj, ei, ej, sides, l=lf, c=ci, o=out: ctx.tile_get_edges_um(l, c, hi, hj, ei, ej, sides, out=o)
    dist = lambda hi, hj, wi, wj, sides, co=lf, o=out: ctx.tile_get_dist_um(co, lf, la, lo, hi, hj, wi, wj, sides, out=o)
    # sides outside 0 .. 15
    for sides in (-1, 16):
        _refused(lambda: edges(h, h, 1, 1, sides), out)
        _refused(lambda: dist(h, h, 1, 1, sides), out)
    # ext / win negative, win beyond 255
    for e in ((-1, 1), (1, -1)):
        _refused(lambda: edges(h, h, *e, 0), out)
        _refused(lambda: dist(h, h, *e, 0), out)
    for w in ((256, 1), (1, 256)):
        _refused(lambda: dist(h, h, *w, 15), out)
    # a halo too small: a cut side needs ext + 1 (edges) / win (distance), an edge side 1 (edges)
    _refused(lambda: edges(h, h, h, 1, ut.EAST | ut.SOUTH | ut.NORTH), out)         # west is cut: ext_i + 1 > halo_i
    _refused(lambda: edges(h, h, 1, h, ut.WEST | ut.EAST | ut.SOUTH), out)          # north is cut: ext_j + 1 > halo_j
    _refused(lambda: dist(h, h, h + 1, 1, ut.WEST | ut.SOUTH | ut.NORTH), out)      # east is cut: win_i > halo_i
    _refused(lambda: dist(h, h, 1, h + 1, ut.WEST | ut.EAST | ut.NORTH), out)       # south is cut: win_j > halo_j
    flat = np.full((ny, nx), SENT, dt)
    _refused(lambda: ctx.tile_get_edges_um(np.zeros((ny, nx), dt), np.zeros((ny, nx), dt), 0, 0, 0, 0, 15, out=flat), flat)
    # bad sizes: a frame with no interior
    thin = np.full((2 * h, nx + 2 * h), SENT, dt)
    _refused(lambda: ctx.tile_get_edges_um(np.zeros(thin.shape, dt), np.zeros(thin.shape, dt), h, h, 1, 1, 0, out=thin), thin)
    _refused(lambda: ctx.tile_get_dist_um(np.zeros(thin.shape, dt), np.zeros(thin.shape, dt), np.zeros(thin.shape, dt),
                                          np.zeros(thin.shape, dt), h, h, 1, 1, 0, out=thin), thin)
    # coast_l overlapping an input of the edges call
    _refused(lambda: edges(h, h, 1, 1, 0, o=lf), lf)
    _refused(lambda: edges(h, h, 1, 1, 0, o=ci), ci)
    # NULL pointers (the C ABI itself)
    import ctypes as C
    p = lambda a: C.c_void_p(a.ctypes.data)
    i = C.c_int
    for args in ((None, p(ci), p(out)), (p(lf), None, p(out)), (p(lf), p(ci), None)):
        assert ctx.lib.sb_tile_get_edges_um_f64(ctx.h, i(nx), i(ny), i(h), i(h), i(1), i(1), i(0), *args) == 1
    for k in range(5):
        args = [p(lf), p(lf), p(la), p(lo), p(out)]
        args.insert(4, C.c_double(180.0))
        args[k if k < 4 else 5] = None
        assert ctx.lib.sb_tile_get_dist_um_f64(ctx.h, i(nx), i(ny), i(h), i(h), i(1), i(1), i(0), *args) == 1
    assert (out == SENT).all()
    # ... and the widest halo-bound calls are served: ext = halo - 1, win = halo on cut sides
    got = edges(h, h, h - 1, h - 1, 0, o=out.copy())
    assert set(np.unique(got[1:-1, 1:-1])) <= {0.0, 1.0} and (got[0] == SENT).all() and (got[:, 0] == SENT).all()
    got = dist(h, h, h, h, 0, co=got, o=out.copy())
    assert (np.abs(got[h:-h, h:-h]) < 12000.0).any() and (got[:h] == SENT).all()
