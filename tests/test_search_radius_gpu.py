"""search_radius on the GPU (sb_radius_kernels.hip) against the numpy model of tests/radius_ref.py: the plane, the summary
and the histogram are integers and must be EQUAL -- summary and histogram recomputed from the model's plane.  Where a diag
call can say the same thing afterwards (sb_last_counters), it must."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import radius_ref as rr
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

MAXDIST = 700.0
PRECS = [np.float64, np.float32]
KEYS = ("band_cells", "with_radius", "without_window", "max_radius")


@pytest.fixture(scope="module")
def ctx2():
    """a second context: the diag calls whose counters are compared run here, search_radius in the session's"""
    c = hip.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def coast(hipctx):
    """per precision: the 200 x 72 synthetic fields and the library's own coast distance; never modified"""
    out = {}
    for dt in PRECS:
        st = synth.static_fields(200, 72, dt)
        edges = hipctx.get_edges(st.landfrac, st.icefrac)
        mask = hipctx.get_dist(edges, st.landfrac, st.lon, st.lat, maxdist=MAXDIST)
        mask.setflags(write=False)
        out[np.dtype(dt)] = (st, mask)
    return out


def _check(ctx, mask, maxdist, halo=0, bnd=hip.SB_BND_GLOBAL, band=None, nhist=0, what=""):
    """one call against the model; returns (plane, summary list, hist)"""
    ref = rr.search_radius(mask, maxdist, halo, bnd, band)
    if band is None:
        r, s, h = ctx.search_radius(mask, maxdist=maxdist, halo=halo, bnd=bnd, nhist=nhist)
    else:
        r, s, h = ctx.band_search_radius(mask, halo, band[0], band[1], maxdist=maxdist, nhist=nhist)
    assert r.dtype == np.int32 and r.shape == ref.shape
    bad = np.argwhere(r != ref)
    assert bad.size == 0, f"{what}: {len(bad)} cells differ, first (y, x) = {bad[0]}: {r[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
    s = [s[k] for k in KEYS]
    assert s == rr.summary_of(ref), what
    if nhist:
        assert np.array_equal(h, rr.hist_of(ref, nhist)), what
    else:
        assert h is None
    return ref, s, h


def _tun(maxdist):
    t = hip.Tunables()
    hip.load_library().sb_default_tunables(C.byref(t))
    t.maxdist_km = maxdist
    return t


# ---- 1: the synthetic coast, and what a diag call counts afterwards -----------------------------------------------------

@pytest.mark.parametrize("dt", PRECS)
def test_synthetic_coast_global(hipctx, ctx2, coast, dt):
    st, mask = coast[np.dtype(dt)]
    ny, nx = mask.shape
    ref, s, _ = _check(hipctx, mask, MAXDIST, nhist=40, what="global")
    assert s[3] >= 2
    nz = 2
    u, v = synth.wind_step(st, nz, 1, dt)
    state = [np.zeros((ny, nx), dt) for _ in range(4)]
    ctx2.seabreeze_diag(5400.0, 1, synth.pressure_3d(st, nz, dt), u, v, synth.theta_step(st, 1, dt), mask, st.z, st.sigma, *state,
                        halo=0, bnd=hip.SB_BND_GLOBAL, tunables=_tun(MAXDIST))
    c = ctx2.last_counters()
    assert (s[0], s[2], s[3]) == (c["band_cells"], c["one_class_cells"], c["max_radius"])


@pytest.mark.parametrize("dt", PRECS)
def test_synthetic_coast_wrapper(hipctx, ctx2, coast, dt):
    st, mask = coast[np.dtype(dt)]
    ny, nx = mask.shape
    ref, s, _ = _check(hipctx, mask, MAXDIST, bnd=hip.SB_BND_WRAPPER, nhist=40, what="wrapper")
    assert s[3] >= 2 and not ref[ny - 1].any()
    nz = 2
    u, v = synth.wind_step(st, nz, 1, dt)
    state = [np.zeros((ny, nx), dt) for _ in range(3)]
    ctx2.diag(1, synth.pressure_1d(nz, dt), st.z, st.sigma, synth.theta_step(st, 1, dt), v, u, mask, *state, maxdist=MAXDIST,
              timestep=90.0)
    c = ctx2.last_counters()
    assert (s[0], s[2], s[3]) == (c["band_cells"], c["one_class_cells"], c["max_radius"])


# ---- 2: directed masks: +-1, every cell a band cell -----------------------------------------------------------------------

def _sea(ny, nx, dt):
    return np.full((ny, nx), -1.0, dt)


@pytest.mark.parametrize("dt", PRECS)
def test_seam_and_wrapper_quirk(hipctx, dt):
    ny, nx = 40, 130
    first, last = _sea(ny, nx, dt), _sea(ny, nx, dt)
    first[20, 0] = 1.0
    last[20, nx - 1] = 1.0
    r, _, _ = _check(hipctx, first, 1e9, what="land at column 0, global")
    assert r[20, nx - 1] == 1 and r[20, nx - 2] == 2 and r[20, 64] == 64 and r[20, 65] == 65 and r[20, 66] == 64
    r, _, _ = _check(hipctx, last, 1e9, what="land at column nx-1, global")
    assert r[20, 0] == 1 and r[20, 64] == 65 and r[0, 64] == 65
    # the wrapper rule reads column 0 for offsets -1 and nx-1: the land cell at column 0 is seen twice over the seam, a
    # cell in the last column has it for its own centre, and the land cell in the last column is never seen at all
    r, s, _ = _check(hipctx, first, 1e9, bnd=hip.SB_BND_WRAPPER, what="land at column 0, wrapper")
    assert r[20, nx - 1] == 1 and r[20, nx - 2] == 1 and r[20, nx - 3] == 2
    r, s, _ = _check(hipctx, last, 1e9, bnd=hip.SB_BND_WRAPPER, what="land at column nx-1, wrapper")
    assert s[0] == (ny - 1) * nx and s[2] == s[0] and s[3] == 0 and (r[:ny - 1] == -1).all()


@pytest.mark.parametrize("dt", PRECS)
def test_one_land_cell_radii_to_150(hipctx, dt):
    ny, nx = 160, 300
    m = _sea(ny, nx, dt)
    m[0, 150] = 1.0
    r, s, h = _check(hipctx, m, 1e9, nhist=129, what="one land cell")
    assert s[3] == 159 and s[2] == 0                     # the latitude is clamped, not periodic: row 159 is 159 rows away
    assert h[128] == (r >= 128).sum() > 0 and h[127] == (r == 127).sum() > 0
    m = _sea(ny, nx, dt)
    m[80, 150] = 1.0
    r, s, h = _check(hipctx, m, 1e9, nhist=129, what="one land cell in the middle")
    assert s[3] == 150 and h[128] == (r >= 128).sum() > 0


@pytest.mark.parametrize("dt", PRECS)
def test_checkerboard_regimes(hipctx, dt):
    ny, nx = 130, 200
    y, x = np.mgrid[0:ny, 0:nx]
    m = np.where(((y // 40) + (x // 40)) % 2 == 0, 1.0, -1.0).astype(dt)
    r, s, h = _check(hipctx, m, 1e9, nhist=129, what="checkerboard")
    # 20 inside a block; the blocks at the seam (200 = 5 x 40: two of one class meet) and in the first row (no row beyond
    # the pole) are wider than 40 cells one way, and where both happen the radius reaches 40
    assert r[60, 60] == 20 and s[3] == 40 and s[2] == 0
    reg = hip.contrast_regimes(h)
    assert reg == rr.regimes_of(r) and reg["strip"] > 0 and reg["wide"] > 0 and reg["table"] > 0 and reg["none"] == 0


@pytest.mark.parametrize("dt", PRECS)
def test_band_at_both_poles(hipctx, dt):
    """a slanted coast from the first row to the last: the windows of the band cells in both pole rows run into the clamp"""
    ny, nx = 72, 200
    y, x = np.mgrid[0:ny, 0:nx]
    m = (x - 50.0 - 0.7 * y).astype(dt)
    m[m > 100] = (-(m[m > 100] - 150) - 50).astype(dt)    # and back to the sea side round the circle
    r, s, _ = _check(hipctx, m, 12.5, what="slanted coast, global")
    assert r[0].any() and r[ny - 1].any() and s[2] == 0 and s[3] >= 9
    _check(hipctx, m, 12.5, bnd=hip.SB_BND_WRAPPER, what="slanted coast, wrapper")


@pytest.mark.parametrize("dt", PRECS)
def test_all_land_is_answered_at_once(hipctx, dt):
    ny, nx = 72, 200
    m = np.ones((ny, nx), dt)
    hipctx.search_radius(m, maxdist=1e9)                  # (workspace and code are in place)
    t0 = time.perf_counter()
    r, s, h = _check(hipctx, m, 1e9, nhist=8, what="all land")
    assert time.perf_counter() - t0 < 3.0
    assert (r == -1).all() and s == [nx * ny, 0, nx * ny, 0] and h[0] == nx * ny and h[1:].sum() == 0
    r, s, _ = _check(hipctx, -m, 1e9, bnd=hip.SB_BND_WRAPPER, what="all sea, wrapper")
    assert s[2] == s[0] == (ny - 1) * nx


def test_all_land_on_a_grid_where_a_walk_would_show(hipctx):
    """4096 x 2048, single precision, all land: a walk of nx + ny = 6144 steps for each of 8.4 million band cells is 5e10
    steps of two loads each; the answer from the flags is one pass over mask.  Only the call is timed (it stages 32 MB
    each way); the expected plane needs no model."""
    ny, nx = 2048, 4096
    m = np.ones((ny, nx), np.float32)
    hipctx.search_radius(m[:8], maxdist=1e9)              # (code in place)
    t0 = time.perf_counter()
    r, s, h = hipctx.search_radius(m, maxdist=1e9, nhist=4)
    took = time.perf_counter() - t0
    assert took < 3.0, took
    assert (r == -1).all() and [s[k] for k in KEYS] == [nx * ny, 0, nx * ny, 0] and h.tolist() == [nx * ny, 0, 0, 0]


def _stripes(ny, nx, dt, land):
    """every row the same: the radius of a cell is its row distance to the other class (the clamp adds no row)"""
    m = _sea(ny, nx, dt)
    for a, b in land:
        m[:, a:b] = 1.0
    return m


@pytest.mark.parametrize("dt", PRECS)
def test_rows_of_whole_words(hipctx, dt):
    """nx = 128: two full 64-cell words, no partial last word; stripes that end on the word boundary and at the seam"""
    ny, nx = 10, 128
    for land in ([(0, 64)], [(64, 128)], [(63, 65)], [(127, 128)], [(0, 1), (100, 101)]):
        m = _stripes(ny, nx, dt, land)
        for bnd in (hip.SB_BND_GLOBAL, hip.SB_BND_WRAPPER):
            r, s, _ = _check(hipctx, m, 1e9, bnd=bnd, nhist=40, what=f"stripes {land}, rule {bnd}")
    m = _stripes(ny, nx, dt, [(0, 64)])
    r, _, _ = _check(hipctx, m, 1e9, what="half and half")
    assert r[5, 31] == 32 and r[5, 32] == 32 and r[5, 64] == 1 and r[5, 96] == 32 and r[5, 127] == 1
    rng = np.random.default_rng(3)
    m = np.where(rng.random((ny, nx)) < 0.02, 1.0, -1.0).astype(dt)
    _check(hipctx, m, 1e9, what="sparse land, 128 columns")
    _check(hipctx, m, 1e9, halo=2, bnd=hip.SB_BND_HALO, what="the same field as a frame: 124 + 2*2 = 128 frame columns")


@pytest.mark.parametrize("dt", PRECS)
def test_rows_of_more_than_64_words(hipctx, dt):
    """nx > 4096: a row's word summary is two words, and the nearest word with a cell of the other class lies in the other
    one, to the right, to the left and round the seam -- for sea cells looking for land and for the land cells of a stripe
    four words wide looking for sea.  Every row the same, so the radii are the row distances themselves."""
    land = [(100, 101), (800, 801), (1500, 1570), (2135, 2136), (2700, 2701), (3300, 3301), (3900, 4150)]
    m = _stripes(2, 4224, dt, land)                       # 66 full words
    r, s, _ = _check(hipctx, m, 1e9, what="4224 columns, global")
    assert r[1, 4223] == 74 and r[1, 4025] == 125 and r[1, 3600] == 300 and s[3] == 350 and s[2] == 0
    m = _stripes(2, 4200, dt, land)                       # 65 words and 40 cells
    r, s, _ = _check(hipctx, m, 1e9, bnd=hip.SB_BND_WRAPPER, what="4200 columns, wrapper")
    assert s[3] == 350
    f = _stripes(2 + 6, 4200 + 6, dt, [(0, 2), (2050, 2052), (4095, 4099), (4204, 4206)])
    r, s, _ = _check(hipctx, f, 1e9, halo=3, bnd=hip.SB_BND_HALO, what="4206 frame columns, no wrap")
    assert s[1] > 0 and s[2] > 0


@pytest.mark.parametrize("dt", PRECS)
def test_signed_zero_nan_and_the_band_limit(hipctx, dt):
    m = _sea(6, 10, dt)
    m[2, 3] = -0.0                                        # land side
    m[4, 7] = np.nan                                      # sea side, and a band cell whatever maxdist
    m[0, 0] = -5.0                                        # |mask| == maxdist: a band cell
    m[0, 1] = -np.nextafter(dt(5.0), dt(10.0))            # one step beyond: not a band cell
    r, s, _ = _check(hipctx, m, 5.0, what="special values")
    assert r[2, 3] == 1 and r[4, 7] == 4 and r[0, 0] == 3 and r[0, 1] == 0 and s[0] == 59
    m = np.full((6, 10), np.nan, dt)                      # all NaN: all band cells, all sea side
    r, s, _ = _check(hipctx, m, 5.0, what="all NaN")
    assert s == [60, 0, 60, 0]


# ---- 3: a ghost-celled frame ------------------------------------------------------------------------------------------------

def _frame(a, h):
    return np.ascontiguousarray(np.pad(np.pad(a, ((0, 0), (h, h)), mode="wrap"), ((h, h), (0, 0)), mode="edge"))


@pytest.mark.parametrize("dt", PRECS)
def test_halo_frame(hipctx, ctx2, coast, dt):
    """The 200 x 72 coast in a frame of 5 ghost cells, periodic and clamped copies.  Within 700 km of this coast no window
    is wider than 3 cells, so the frame would cut none: maxdist is set beyond get_dist's fill value (12000), every cell is
    a band cell, the radii reach 15 and the frame cuts the widest."""
    st, mask = coast[np.dtype(dt)]
    ny, nx = mask.shape
    h, nz, maxdist = 5, 2, 20000.0
    mf = _frame(mask, h)
    ref, s, _ = _check(hipctx, mf, maxdist, halo=h, bnd=hip.SB_BND_HALO, nhist=16, what="frame")
    assert (ref == -1).any() and (ref > 0).any(), "the frame must cut some windows and leave others whole"
    whole = rr.search_radius(mask, maxdist, 0, rr.BND_GLOBAL)
    inside = ref > 0
    assert np.array_equal(ref[inside], whole[inside]) and (whole[ref == -1] > h).all()
    u, v = synth.wind_step(st, nz, 1, dt)
    state = [np.zeros((ny, nx), dt) for _ in range(4)]
    ctx2.seabreeze_diag(5400.0, 1, synth.pressure_3d(st, nz, dt), u, v, _frame(synth.theta_step(st, 1, dt), h), mf, _frame(st.z, h),
                        _frame(st.sigma, h), *state, halo=h, bnd=hip.SB_BND_HALO, tunables=_tun(maxdist))
    c = ctx2.last_counters()
    assert (s[0], s[2]) == (c["band_cells"], c["one_class_cells"])


# ---- 4: the forms ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", PRECS)
def test_dev_form_and_null_radius(hipctx, coast, dt):
    _, mask = coast[np.dtype(dt)]
    ny, nx = mask.shape
    nh = 24
    r, s, h = hipctx.search_radius(mask, maxdist=MAXDIST, nhist=nh)
    dm = torch.from_numpy(mask.copy()).cuda()
    dr = torch.full((ny, nx), 77, dtype=torch.int32, device="cuda")
    ds = torch.full((4,), 77, dtype=torch.int64, device="cuda")      # (the call zeroes them itself)
    dh = torch.full((nh,), 77, dtype=torch.int64, device="cuda")
    ds2 = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        hipctx.search_radius_dev(dt, nx, ny, 0, hip.SB_BND_GLOBAL, dm.data_ptr(), dr.data_ptr(), ds.data_ptr(), dh.data_ptr(), nh,
                                 maxdist=MAXDIST, stream=st.cuda_stream)
        hipctx.search_radius_dev(dt, nx, ny, 0, hip.SB_BND_GLOBAL, dm.data_ptr(), None, ds2.data_ptr(), maxdist=MAXDIST,
                                 stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(dr.cpu().numpy(), r) and np.array_equal(dh.cpu().numpy(), h)
    assert ds.cpu().tolist() == [s[k] for k in KEYS] == ds2.cpu().tolist()
    # the host form without a plane
    lib, summ = hipctx.lib, (C.c_longlong * 4)()
    sfx, ct = ("f64", C.c_double) if dt == np.float64 else ("f32", C.c_float)
    fn = getattr(lib, f"sb_search_radius_{sfx}")
    args = lambda nx_, ny_, halo, bnd, m, rad, su, hi, nhi: (hipctx.h, C.c_int(nx_), C.c_int(ny_), C.c_int(halo), C.c_int(bnd),
                                                             hip._p(m), ct(MAXDIST), hip._p(rad), su, hip._p(hi), C.c_int(nhi))
    assert fn(*args(nx, ny, 0, 1, mask, None, summ, None, 0)) == 0
    assert list(summ) == [s[k] for k in KEYS]
    # argument errors
    hist = np.zeros(4, np.int64)
    assert fn(*args(nx, ny, 0, 1, None, r, summ, None, 0)) == 1          # no mask
    assert fn(*args(nx, ny, 0, 1, mask, None, None, None, 0)) == 1       # nothing asked for
    assert fn(*args(nx, ny, 0, 1, mask, None, None, hist, 0)) == 1       # ... a histogram of no bins is nothing
    assert fn(*args(0, ny, 0, 1, mask, r, summ, None, 0)) == 1           # bad sizes
    assert fn(*args(nx, -1, 0, 1, mask, r, summ, None, 0)) == 1
    assert fn(*args(nx, ny, 0, 3, mask, r, summ, None, 0)) == 1          # no such rule
    assert fn(*args(nx - 2, ny - 2, 1, 1, mask, r, summ, None, 0)) == 1  # halo with a rule that has none
    assert fn(*args(nx - 2, ny - 2, 1, 0, mask, r, summ, None, 0)) == 1
    assert fn(*args(nx, ny, 0, 1, mask, r, summ, hist, 1)) == 1          # a histogram needs two bins
    assert fn(*args(nx, ny, 0, 1, mask, None, None, hist, 4)) == 0       # a histogram alone is a result
    assert np.array_equal(hist, rr.hist_of(r, 4))
    assert fn(*args(128, 1 << 30, 0, 1, mask, r, summ, None, 0)) == 1    # more segments than the kernels number
    assert b"segments" in lib.sb_last_error(hipctx.h)
    assert fn(*args(70000, 4, 0, 1, mask, r, summ, None, 0)) == 1        # a row the 16-bit distance cannot span
    assert b"wider" in lib.sb_last_error(hipctx.h)
    fb = getattr(lib, f"sb_band_search_radius_{sfx}")
    assert fb(hipctx.h, C.c_int(nx), C.c_int(ny), C.c_int(-1), C.c_int(1), C.c_int(1), hip._p(mask), ct(MAXDIST), hip._p(r), summ,
              None, C.c_int(0)) == 1


def test_band_runner_check_halo(coast):
    """BandRunner.check_halo on one rank that owns the globe: the whole-grid numbers, from the mask it holds"""
    from seabreeze_param_amd import bands
    dt = np.float64
    st, mask = coast[np.dtype(dt)]
    ny, nx = mask.shape
    ctx = hip.Context()
    try:
        br = bands.BandRunner(ctx, torch, None, 0, 1, nx, ny, 2, 16, dtype=dt)
        br.upload_static(st.z, st.sigma, mask)
        s = rr.summary_of(rr.search_radius(mask, MAXDIST, 0, rr.BND_GLOBAL))
        assert br.check_halo(MAXDIST) == (s[3], s[2])
        s = rr.summary_of(rr.search_radius(mask, 100.0, 0, rr.BND_GLOBAL))
        assert br.check_halo(100.0) == (s[3], s[2])
    finally:
        ctx.close()


@pytest.mark.parametrize("dt", PRECS)
def test_band_dev_form_and_check_halo_of_a_cut_band(hipctx, dt):
    """sb_band_search_radius_*_dev on a frame cut on both sides, against the host band form; and BandRunner.check_halo on
    the middle rank of three, which takes that entry point, from the frame it holds -- one process, no communicator."""
    from seabreeze_param_amd import bands
    nx, ny, h, r0, r1, nh = 200, 96, 2, 30, 63, 12
    st = synth.static_fields(nx, ny, dt)
    edges = hipctx.get_edges(st.landfrac, st.icefrac, rule=1, bnd=hip.SB_BND_GLOBAL)
    mask = hipctx.get_dist(edges, st.landfrac, st.lon, st.lat, maxdist=MAXDIST)
    f = np.zeros((r1 - r0 + 2 * h, nx + 2 * h), dt)
    f[:, h:h + nx] = mask[r0 - h:r1 + h]
    want, s, hist = _check(hipctx, f, MAXDIST, halo=h, band=(False, False), nhist=nh, what="cut band, host form")
    assert s[2] > 0 and s[1] > 0                           # two ghost rows are too few for some cells, enough for others
    df = torch.from_numpy(f).cuda()
    dr = torch.full((r1 - r0, nx), 77, dtype=torch.int32, device="cuda")
    ds = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    dh = torch.full((nh,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    strm = torch.cuda.Stream()
    with torch.cuda.stream(strm):
        hipctx.band_search_radius_dev(dt, nx, r1 - r0, h, False, False, df.data_ptr(), dr.data_ptr(), ds.data_ptr(), dh.data_ptr(),
                                      nh, maxdist=MAXDIST, stream=strm.cuda_stream)
    strm.synchronize()
    assert np.array_equal(dr.cpu().numpy(), want) and ds.cpu().tolist() == s and np.array_equal(dh.cpu().numpy(), hist)
    ctx = hip.Context()
    try:
        br = bands.BandRunner(ctx, torch, None, 1, 3, nx, ny, 2, h, dtype=dt, rows=(r0, r1))
        br.mask = df
        assert br.check_halo(MAXDIST) == (s[3], s[2])
    finally:
        ctx.close()


# ---- 5: a band's plane is the whole grid's, as far as its ghost rows reach ---------------------------------------------

@pytest.mark.parametrize("dt", PRECS)
def test_band_property(hipctx, dt):
    nx, ny = 200, 96
    st = synth.static_fields(nx, ny, dt)
    edges = hipctx.get_edges(st.landfrac, st.icefrac, rule=1, bnd=hip.SB_BND_GLOBAL)
    mask = hipctx.get_dist(edges, st.landfrac, st.lon, st.lat, maxdist=MAXDIST)
    R, s, _ = _check(hipctx, mask, MAXDIST, what="whole grid")
    rmax = s[3]
    assert rmax >= 3 and s[2] == 0
    cuts = [(0, 30), (30, 63), (63, 96)]
    beyond = 0
    for h in (rmax, rmax - 1):
        for r0, r1 in cuts:
            south, north = r0 == 0, r1 == ny
            f = np.full((r1 - r0 + 2 * h, nx + 2 * h), np.nan, dt)          # what is never read: NaN would be sea side
            lo, hi = max(r0 - h, 0), min(r1 + h, ny)
            f[h - (r0 - lo):h + (hi - r0), h:h + nx] = mask[lo:hi]
            got, _, _ = _check(hipctx, f, MAXDIST, halo=h, band=(south, north), what=f"band {r0}:{r1} halo {h}")
            y = np.arange(r0, r1)
            reach = np.minimum(np.where(south, 1 << 20, y - r0 + h), np.where(north, 1 << 20, r1 - 1 - y + h))[:, None]
            want = np.where((R[r0:r1] > 0) & (R[r0:r1] > reach), -1, R[r0:r1])
            assert np.array_equal(got, want), f"band {r0}:{r1} halo {h}"
            if h == rmax:
                assert np.array_equal(got, R[r0:r1])
            else:
                beyond += int((want != R[r0:r1]).sum())
    assert beyond > 0, "no cell needed the last ghost row"


# ---- 6: no side effects on what a diag call enqueues or returns ------------------------------------------------------------

def _two_steps(dt, st, mask, table, interleave):
    """tn = 1, [search_radius], tn = 2 on a fresh context; -> (state after tn = 2, fills, launches of tn = 2)"""
    ctx = hip.Context()
    try:
        if table:
            ctx.set_table_contrast(True)
            ctx.set_table_window_cache(True)
        ny, nx = mask.shape
        nz = 2
        up = lambda a: torch.from_numpy(np.array(a, dtype=dt)).cuda()
        p, z, sg, dm = up(synth.pressure_3d(st, nz, dt)), up(st.z), up(st.sigma), up(mask)
        state = [torch.zeros((ny, nx), dtype=p.dtype, device="cuda") for _ in range(4)]
        dr = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
        ds = torch.zeros(4, dtype=torch.int64, device="cuda")
        stream = hip.torch_stream_handle(torch)
        for tn in (1, 2):
            u, v = (up(a) for a in synth.wind_step(st, nz, tn, dt))
            th = up(synth.theta_step(st, tn, dt))
            torch.cuda.synchronize()
            ctx.seabreeze_diag_dev(dt, 5400.0, tn, nx, ny, nz, 0, hip.SB_BND_GLOBAL, p.data_ptr(), u.data_ptr(), v.data_ptr(),
                                   th.data_ptr(), dm.data_ptr(), z.data_ptr(), sg.data_ptr(), *[s.data_ptr() for s in state],
                                   stream=stream, tunables=_tun(MAXDIST))
            torch.cuda.synchronize()
            if tn == 1 and interleave:
                ctx.search_radius_dev(dt, nx, ny, 0, hip.SB_BND_GLOBAL, dm.data_ptr(), dr.data_ptr(), ds.data_ptr(),
                                      maxdist=MAXDIST, stream=stream)
                torch.cuda.synchronize()
                assert ds.cpu().tolist()[0] > 0
        fills = ctx.table_cache_report()["fills"] if table else None
        return [s.cpu().numpy() for s in state], fills, ctx.last_step_report(), ctx.last_counters()
    finally:
        ctx.close()


@pytest.mark.parametrize("dt", PRECS)
@pytest.mark.parametrize("table", [True, False])
def test_no_side_effects_on_diag(coast, table, dt):
    st, mask = coast[np.dtype(dt)]
    plain = _two_steps(dt, st, mask, table, False)
    inter = _two_steps(dt, st, mask, table, True)
    if table:
        assert plain[1] == 1 and inter[1] == 1, "the second call must take its windows from the store, with or without the call between"
    assert inter[2] == plain[2] and inter[3] == plain[3]
    for a, b, nm in zip(inter[0], plain[0], ("ws", "wd", "thc", "sb_con")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), nm
