"""get_dist with search windows of 32 .. SB_DIST_MAX_WINDOW cells each way (k_dist_wide, sb_coast_kernels.hip): the
km-scale regional grids the table contrast is for, where 180 km are 113 cells.

Everything goes through the C ABI and is checked against the CPU oracle (oracle.get_dist, oracle.get_edges) under the
rule of tests/test_setup_gpu.py::_check_dist, restated here: the pattern of 12000 cells is equal, signs are equal,
|h - o| / max(|o|, 1) <= 1e-12 in fp64 and <= 2e-6 in fp32 against the oracle of the same precision.

Mask M(nx, ny): a few islands in the first third of the columns and on the seam column, no ice -- windows are empty,
one-sided, or cross the seam.  Each case asserts on the oracle's field that it reaches the branch it is there for (the
sweep-time reset of sobel.f90:188, late sources beyond 2 maxdist after a reset), so it cannot pass on an input that
skips it.
"""
import numpy as np
import pytest

from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

REL = {8: 1e-12, 4: 2e-6}
DT = {8: np.float64, 4: np.float32}
DT_S = 7200.0


@pytest.fixture(autouse=True)
def _radius_hint_back(hipctx):
    """get_dist leaves its window as the search radius hint of the following diag calls: back to the default"""
    yield
    hipctx.set_search_radius_hint(16)


def _check_dist(h, o, what, rel):
    assert np.array_equal(h >= 12000.0, o >= 12000.0), f"{what}: cells without a coast in reach differ"
    assert np.array_equal(np.sign(h), np.sign(o)), f"{what}: signs differ"
    e = np.abs(h - o) / np.maximum(np.abs(o), 1.0)
    print(f"{what}: max rel err {e.max():.3e}")
    assert e.max() <= rel, f"{what}: max rel err {e.max()}"


def _mask_m(nx, ny, dt):
    r = synth.hash_uniform((ny, nx), 5, 31)
    land = (r > 0.999) & (np.arange(nx)[None, :] < nx // 3)
    land[:, -1] = r[:, -1] > 0.97
    return np.ascontiguousarray(land, dt), np.zeros((ny, nx), dt)


def _sparse_mask(nx, ny, dt):
    """M's islands ten times as dense and on both seam columns: a grid of a few thousand cells still holds some"""
    r = synth.hash_uniform((ny, nx), 5, 12)
    land = (r > 0.99).astype(np.float64)
    land[:, 0] = r[:, 0] > 0.9
    land[:, -1] = r[:, -1] > 0.93
    return np.ascontiguousarray(land, dt), np.zeros((ny, nx), dt)


def _noise_mask(nx, ny, seed, dt):
    """Land mask with coast cells everywhere (blobs of a few cells), also across the seam and at the poles."""
    r = synth.hash_uniform((ny, nx), 3, seed)
    s = r + np.roll(r, 1, 1) + np.roll(r, 1, 0) + np.roll(r, -1, 1)
    land = (s > 2.2).astype(np.float64)
    ice = np.where(synth.hash_uniform((ny, nx), 4, seed) > 0.9, 0.35, 0.0)
    return np.ascontiguousarray(land, dt), np.ascontiguousarray(ice, dt)


# ---- 1 and 5: regional grid, 0.0135 degrees, the window derived from the spacing ------------------------------------

RNX, RNY = 704, 200
# the window comes from the spacing and 180 km (113 cells); the runs at 60 km (and at 1e6, which only says what is in
# reach) keep that window, as a model run does that lowers the band width on a distance field's grid: within 113 cells
# a first hit can lie beyond 2 x 60 km, which the window derived from 60 km itself (37 cells) cannot show
RKWIN = {180.0: -1, 60.0: 113, 1.0e6: 113}


def _regional_coords(nx, ny, dt):
    return (10.0 + 0.0135 * np.arange(nx)).astype(dt), (68.0 + 0.0135 * np.arange(ny)).astype(dt)


@pytest.fixture(scope="module")
def regional(oracles):
    """per precision: land, coast, lon, lat and the oracle's field at maxdist 180, 60 and (reach only) 1e6; never modified"""
    out = {}
    for prec in (8, 4):
        dt, orc = DT[prec], oracles[prec]
        lon, lat = _regional_coords(RNX, RNY, dt)
        land, ice = _mask_m(RNX, RNY, dt)
        coast = orc.get_edges(land, ice)
        ref = {md: orc.get_dist(coast, land, lon, lat, maxdist=md, kwin=RKWIN[md]) for md in (180.0, 60.0, 1.0e6)}
        for a in (land, ice, coast, lon, lat, *ref.values()):
            a.setflags(write=False)
        out[prec] = (land, ice, coast, lon, lat, ref)
    return out


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("maxdist", [180.0, 60.0])
def test_regional_automatic_window(hipctx, oracles, regional, maxdist, prec):
    """0.0135 degrees near 70 N: the reference's rule picks 113 cells for 180 km.  Most windows lie inside the frame (the
    per-target column cut), those within 113 columns of its edges cross the closing step of 350 degrees (every hit)."""
    land, ice, coast, lon, lat, ref = regional[prec]
    assert hip.dist_window(lon, lat) == oracles[prec].dist_window(lon, lat) == 113
    o = ref[maxdist]
    share = np.mean(o >= 12000.0)
    assert 0.25 < share < 0.5, share
    if maxdist == 60.0:
        reset = (o >= 12000.0) & (ref[1.0e6] < 12000.0)
        assert np.count_nonzero(reset) >= 1000, np.count_nonzero(reset)                  # the sweep-time reset
        late = (o < 12000.0) & (np.abs(o) > 120.0)
        assert np.count_nonzero(late) >= 1000, np.count_nonzero(late)                    # late sources after a reset
    assert np.array_equal(hipctx.get_edges(land, ice), coast)
    h = hipctx.get_dist(coast, land, lon, lat, maxdist=maxdist, kwin=RKWIN[maxdist])
    _check_dist(h, o, f"regional fp{8 * prec} maxdist={maxdist}", REL[prec])
    # a coast cell's own distance; the kept coordinate tables give the same bits
    assert np.all(np.abs(h[coast > 0]) == 0.5)
    assert np.array_equal(hipctx.get_dist(coast, land, lon, lat, maxdist=maxdist, kwin=RKWIN[maxdist]), h)


@pytest.mark.parametrize("prec", [8, 4])
def test_regional_window_derived_from_60_km(hipctx, oracles, regional, prec):
    """kwin = -1 at maxdist = 60: the rule picks 37 cells, k_dist_wide's second pass and the per-target cut again"""
    land, ice, coast, lon, lat, _ = regional[prec]
    assert hip.dist_window(lon, lat, 60.0) == oracles[prec].dist_window(lon, lat, 60.0) == 37
    o = oracles[prec].get_dist(coast, land, lon, lat, maxdist=60.0, kwin=-1)
    h = hipctx.get_dist(coast, land, lon, lat, maxdist=60.0, kwin=-1)
    _check_dist(h, o, f"regional fp{8 * prec} maxdist=60 k=37", REL[prec])


# ---- 2: global grids, explicit windows -------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny,kwin", [(640, 150, 120), (300, 64, 255), (200, 60, 120), (192, 48, 112)])
def test_global_explicit_windows(hipctx, oracles, nx, ny, kwin):
    """(640, 150, 120): a workgroup's reach fits the circle; (300, 64, 255): the limit, and with (200, 60, 120) a window
    wider than the circle; (192, 48, 112): the first width the LDS tile of k_dist could not hold."""
    dt, orc = np.float64, oracles[8]
    lon, lat = synth.grid(nx, ny)
    land, ice = _mask_m(nx, ny, dt)
    coast = orc.get_edges(land, ice)
    for maxdist in (5000.0, 1500.0):
        o = orc.get_dist(coast, land, lon, lat, maxdist=maxdist, kwin=kwin)
        if maxdist == 1500.0 and (nx, ny) == (640, 150):
            far = orc.get_dist(coast, land, lon, lat, maxdist=1.0e6, kwin=kwin)
            reset = np.count_nonzero((o >= 12000.0) & (far < 12000.0))
            late = np.count_nonzero((o < 12000.0) & (np.abs(o) > 2 * maxdist))
            assert reset > 100 and late > 100, (reset, late)
        h = hipctx.get_dist(coast, land, lon, lat, maxdist=maxdist, kwin=kwin)
        _check_dist(h, o, f"global {nx}x{ny} k={kwin} maxdist={maxdist}", 1e-12)


# ---- 3: coordinates that forbid the cuts -----------------------------------------------------------------------------

@pytest.mark.parametrize("lons", ["regional", "shuffled", "descending", "repeated", "lat-shuffled", "lat-descending"])
@pytest.mark.parametrize("ny,kwin", [(60, 40), (20, 112)])
def test_coordinates_that_forbid_the_cuts(hipctx, oracles, lons, ny, kwin):
    """The layouts of tests/test_setup_gpu.py::test_get_dist_every_hit_path at k = 40 on 420 x 60: the column cut is
    decided per target (regional, descending), off (shuffled, repeated); the row cut has its own flag (lat-shuffled).
    Again at k = 112 on 420 x 20 (islands instead of the dense coast: two or three hits per row of a window, and an oracle
    run of a second): four staging passes, windows of four words."""
    nx = 420
    dt, orc = np.float64, oracles[8]
    _, lat = synth.grid(nx, ny)
    lon = {"regional": np.linspace(100.0, 160.0, nx),                       # closing step of 300 degrees
           "shuffled": np.random.default_rng(5).permutation(np.linspace(0.0, 357.6, nx)),
           "descending": np.linspace(357.6, 0.0, nx),
           "repeated": np.repeat(np.linspace(0.0, 355.2, nx // 2), 2)}.get(lons, synth.grid(nx, ny)[0])
    if lons == "lat-shuffled":
        lat = np.random.default_rng(6).permutation(lat)
    if lons == "lat-descending":
        lat = lat[::-1].copy()
    land, ice = _noise_mask(nx, ny, 21, dt) if kwin == 40 else _sparse_mask(nx, ny, dt)
    coast = orc.get_edges(land, ice)
    o = orc.get_dist(coast, land, lon, lat, maxdist=400.0, kwin=kwin)
    h = hipctx.get_dist(coast, land, lon, lat, maxdist=400.0, kwin=kwin)
    _check_dist(h, o, lons, 1e-12)


# ---- 4: edges of the dispatch ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny,kwin,maker", [(330, 70, 31, _mask_m), (330, 70, 32, _mask_m), (391, 47, 45, _sparse_mask),
                                              (258, 20, 33, _sparse_mask)])
def test_dispatch_edges_and_ragged_sizes(hipctx, oracles, nx, ny, kwin, maker):
    """31 | 32: the last window of k_dist_bits and the first of k_dist_wide; ragged workgroups and bit words."""
    dt, orc = np.float64, oracles[8]
    lon, lat = synth.grid(nx, ny)
    land, ice = maker(nx, ny, dt)
    coast = orc.get_edges(land, ice)
    o = orc.get_dist(coast, land, lon, lat, maxdist=900.0, kwin=kwin)
    assert np.mean(o < 12000.0) > 0.05                                                   # (not an empty field)
    h = hipctx.get_dist(coast, land, lon, lat, maxdist=900.0, kwin=kwin)
    _check_dist(h, o, f"{nx}x{ny} k={kwin}", 1e-12)


@pytest.mark.parametrize("nx,ny,kwin", [(40, 30, 31), (30, 24, 20)])
def test_small_window_wider_than_the_grid_keeps_k_dist(hipctx, oracles, nx, ny, kwin):
    """k <= 31 with 2k + 1 > nx: what is left to the byte-probe kernel k_dist now that windows from 32 cells on, which
    tests/test_setup_gpu.py::test_get_dist_wide_window_lds_kernel was written for, take k_dist_wide."""
    dt, orc = np.float64, oracles[8]
    lon, lat = synth.grid(nx, ny)
    land, ice = _sparse_mask(nx, ny, dt)
    coast = orc.get_edges(land, ice)
    o = orc.get_dist(coast, land, lon, lat, maxdist=5000.0, kwin=kwin)
    assert np.mean(o < 12000.0) > 0.05
    _check_dist(hipctx.get_dist(coast, land, lon, lat, maxdist=5000.0, kwin=kwin), o, f"{nx}x{ny} k={kwin}", 1e-12)


def test_window_beyond_the_limit_is_refused(hipctx, oracles):
    nx, ny = 330, 70
    dt, orc = np.float64, oracles[8]
    lon, lat = synth.grid(nx, ny)
    land, ice = _mask_m(nx, ny, dt)
    coast = orc.get_edges(land, ice)
    with pytest.raises(hip.SeabreezeHipError) as err:
        hipctx.get_dist(coast, land, lon, lat, maxdist=900.0, kwin=hip.SB_DIST_MAX_WINDOW + 1)
    assert "255" in str(err.value) and "SB_DIST_MAX_WINDOW" in str(err.value), str(err.value)
    o = orc.get_dist(coast, land, lon, lat, maxdist=900.0, kwin=5)
    _check_dist(hipctx.get_dist(coast, land, lon, lat, maxdist=900.0, kwin=5), o, "k=5 after the refusal", 1e-12)


# ---- 6: the distance field feeds the table contrast ------------------------------------------------------------------

def test_chain_into_the_table_contrast(hipctx, oracles):
    """320 x 400 at 0.0135 degrees, land south of row 200: get_edges, get_dist (113 cells) and two diag steps with
    sb_set_table_contrast.  The oracle's diag at these radii takes minutes and is not run: k_scan reads the mask only
    through its sign and the band test, so the steps fed by the library's field and by the oracle's must give the same
    bits, and the counters follow from the geometry."""
    nx, ny, nz = 320, 400, 3
    dt, orc = np.float64, oracles[8]
    lon, lat = _regional_coords(nx, ny, dt)
    land = np.ascontiguousarray(np.broadcast_to(np.arange(ny)[:, None] < 200, (ny, nx)), dt)
    ice = np.zeros((ny, nx), dt)
    coast = orc.get_edges(land, ice, rule=0, bnd=1)
    assert np.array_equal(hipctx.get_edges(land, ice, rule=0, bnd=hip.SB_BND_GLOBAL), coast)
    assert hip.dist_window(lon, lat, 180.0) == 113
    o = orc.get_dist(coast, land, lon, lat, maxdist=180.0, kwin=-1)
    h = hipctx.get_dist(coast, land, lon, lat, maxdist=180.0, kwin=-1)
    _check_dist(h, o, "east-west coast", 1e-12)
    band = np.abs(o) <= 180.0
    assert np.array_equal(np.abs(h) <= 180.0, band) and np.array_equal(np.sign(h), np.sign(o))
    assert np.min(np.abs(np.abs(o) - 180.0)) > 9.0                                       # no cell on the knife edge
    rows = np.nonzero(band.any(axis=1))[0]
    assert (rows[0], rows[-1]) == (86, 313) and 0.5 < band.mean() < 0.6

    st = synth.static_fields(nx, ny, dt)
    p = synth.pressure_3d(st, nz, dt)
    other = hip.Context()
    try:
        res = []
        for ctx, mask in ((hipctx, h), (other, o)):
            ctx.set_table_contrast(True)
            state = [np.zeros((ny, nx), dt) for _ in range(4)]
            counters = []
            for tn in (1, 2):
                th = synth.theta_step(st, tn, dt)
                u, v = synth.wind_step(st, nz, tn, dt)
                ctx.seabreeze_diag(DT_S, tn, p, u, v, th, mask, st.z, st.sigma, *state, halo=0, bnd=hip.SB_BND_GLOBAL)
                counters.append(ctx.last_counters())
            res.append((state, counters))
    finally:
        hipctx.set_table_contrast(False)
        other.close()
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b, equal_nan=True)
    # the largest row distance to the other class over the band's cells (an east-west coast: the column does not matter)
    y = np.arange(ny)[:, None] + np.zeros((1, nx), np.int64)
    radius = np.where(y < 200, 200 - y, y - 199)
    assert radius[band].max() == 114
    for c in res[0][1] + res[1][1]:
        assert c["band_cells"] == np.count_nonzero(band), c
        assert c["global_path_cells"] == 0 and c["one_class_cells"] == 0, c
        assert c["max_radius"] == radius[band].max(), c
