"""The band-local coast setup (sb_band_get_edges_*, sb_band_get_dist_*) in one process, without a communicator: a whole
grid is cut into three latitude bands with numpy slices, every band gets a ghost-celled frame whose cut-side ghost rows
are the neighbour's rows (what swap_bounds would deliver), whose pole-side ghost rows, their latitudes and the east-west
ghost columns are NaN (never read), and whose output frames carry a sentinel (only the interior is written).  The stacked
interiors must equal

* the whole-grid GPU call on the same context BIT FOR BIT (include/seabreeze_hip.h: the rule of the band entry points);
* the CPU oracle under the tolerances of tests/test_setup_gpu.py: coast exact; distance 1e-12 (fp64) / 2e-6 (fp32)
  relative to max(|d|, 1 km), signs and "unreached" cells exact.

Shapes: the smallest that reach every kernel of sb_dist_kernel(nx, k) -- the mirror of that decision below is asserted, so
a case cannot drift to another kernel -- with odd band heights, so that the two-row workgroups of k_dist_bits and
k_dist_wide pair rows differently in a band than on the globe, and one case with halo > kwin for the offset arithmetic.

Every case asserts on its own inputs, from the oracle, that it cannot pass vacuously: coast cells within kwin rows of every
cut on both sides; cells below 12000 whose nearest source lies across a cut; and the whole-grid entry point fed a band's own
rows alone differs from the whole-grid field next to every cut.
"""
import ctypes as C

import numpy as np
import pytest

from seabreeze_param_amd import hip, synth
from band_frames import SENTINEL, band_dist, cuts_of, frame, frame_lat, interior, only_interior_written

pytestmark = pytest.mark.gpu

TOL = {8: 1e-12, 4: 2e-6}

#        id              nx  kwin halo  band heights        kernel
CASES = [("BITS32",      320, 15, 15, (33, 33, 33), "BITS32"),
         ("BITS32-halo", 320, 15, 19, (33, 33, 33), "BITS32"),        # halo > kwin: the frame offset is not the window
         ("BITS64",      320, 20, 20, (31, 36, 32), "BITS64"),
         ("BITS_SMALL",   96, 15, 15, (33, 33, 33), "BITS_SMALL"),
         ("BYTES",        24, 15, 15, (17, 21, 19), "BYTES"),
         ("WIDE",        320, 40, 40, (50, 50, 50), "WIDE"),          # two passes of WIDE_A = 31 source rows
         ("WIDE-odd",    320, 40, 40, (49, 51, 50), "WIDE")]          # ... with row pairs that straddle the cuts


def dist_kernel(nx, k):
    """sb_dist_kernel (csrc/sb_dist_plan.hpp)."""
    if k >= 32:
        return "WIDE"
    if 2 * k + 1 > nx:
        return "BYTES"
    if nx < 2 * k + 257:
        return "BITS_SMALL"
    return "BITS32" if k <= 15 else "BITS64"


def coords(nx, ny, which, dt):
    """Set 1: the full circle (NEAREST / CIRCLE cuts on where the window allows); set 2: a regional frame (INNER, ROWS)."""
    lon = 360.0 * np.arange(nx) / nx if which == 1 else 0.1 * np.arange(nx)
    lat = 30.0 + 0.1 * np.arange(ny)
    return lon.astype(dt), lat.astype(dt)


def land_ice(nx, ny, dt, seed=8, level=2.3):
    """Fractional land in small blobs on every row band (coast cells next to every cut, also across the seam), some ice
    near the rules' thresholds: rule 0 and rule 1 give different masks.  A higher level: fewer blobs (the oracle's cost
    grows with the coast cells times the window)."""
    r = synth.hash_uniform((ny, nx), 3, seed)
    s = r + np.roll(r, 1, 1) + np.roll(r, 1, 0)
    land = np.round(np.clip((s - level) / 0.4, 0, 1) * 8) / 8
    ice = np.where(synth.hash_uniform((ny, nx), 4, seed) > 0.93, 0.35, 0.0)
    return np.ascontiguousarray(land, dt), np.ascontiguousarray(ice, dt)


def band_edges(ctx, land, ice, bands, h, rule):
    ny = land.shape[0]
    rows = []
    for r0, r1 in bands:
        out = np.full((r1 - r0 + 2 * h, land.shape[1] + 2 * h), SENTINEL, dtype=land.dtype)
        ctx.band_get_edges(frame(land, r0, r1, h), frame(ice, r0, r1, h), h, r0 == 0, r1 == ny, rule=rule, out=out)
        assert only_interior_written(out, h), f"band {r0}:{r1}: ghost cells of coast were written"
        rows.append(interior(out, h).copy())
    return np.concatenate(rows)


def check_dist(h, o, what, rel):
    assert np.array_equal(h >= 12000.0, o >= 12000.0), f"{what}: cells without a coast in reach differ"
    assert np.array_equal(np.sign(h), np.sign(o)), f"{what}: signs differ"
    e = np.abs(h - o) / np.maximum(np.abs(o), 1.0)
    print(f"{what}: max rel err vs oracle {e.max():.3e}")
    assert e.max() <= rel, f"{what}: max rel err {e.max()}"


def near_cut_rows(bands, kwin, ny):
    """For every cut the rows within kwin of it, below and above."""
    return [(slice(max(c - kwin, 0), c), slice(c, min(c + kwin, ny))) for c in (b[0] for b in bands[1:])]


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("nx,heights,h", [(320, (33, 33, 33), 1), (24, (17, 21, 19), 3), (258, (7, 16, 9), 2)])
def test_band_edges_equal_whole_grid(hipctx, oracles, nx, heights, h, rule, prec):
    dt, orc = (np.float64, oracles[8]) if prec == 8 else (np.float32, oracles[4])
    bands, ny = cuts_of(heights), sum(heights)
    land, ice = land_ice(nx, ny, dt)
    o = orc.get_edges(land, ice, rule=rule, bnd=1)
    whole = hipctx.get_edges(land, ice, rule=rule, bnd=hip.SB_BND_GLOBAL)
    got = band_edges(hipctx, land, ice, bands, h, rule)
    assert np.array_equal(got, whole), f"{np.count_nonzero(got != whole)} cells differ from the whole-grid call"
    assert np.array_equal(got, o), f"{np.count_nonzero(got != o)} cells differ from the oracle"
    # not vacuous: ice is present and the rules differ; a band fed its own rows alone (clamped Sobel) is wrong at every cut
    assert np.any(ice > 0) and not np.array_equal(orc.get_edges(land, ice, rule=1 - rule, bnd=1), o)
    for r0, r1 in bands:
        alone = orc.get_edges(land[r0:r1], ice[r0:r1], rule=rule, bnd=1)
        if r0 > 0:
            assert not np.array_equal(alone[0], o[r0]), "the clamped Sobel gives the same first row: the cut is not tested"
        if r1 < ny:
            assert not np.array_equal(alone[-1], o[r1 - 1]), "the clamped Sobel gives the same last row: the cut is not tested"


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("cset", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_band_dist_equal_whole_grid(hipctx, oracles, case, cset, prec):
    _, nx, kwin, h, heights, kern = case
    assert dist_kernel(nx, kwin) == kern
    dt, orc = (np.float64, oracles[8]) if prec == 8 else (np.float32, oracles[4])
    bands, ny = cuts_of(heights), sum(heights)
    lon, lat = coords(nx, ny, cset, dt)
    land, ice = land_ice(nx, ny, dt, level=2.3 if kwin < 32 else 2.62)
    rule = 1
    coast_o = orc.get_edges(land, ice, rule=rule, bnd=1)
    o = orc.get_dist(coast_o, land, lon, lat, maxdist=180.0, kwin=kwin)

    # ---- the inputs reach what the case is about (from the oracle) ----
    for below, above in near_cut_rows(bands, kwin, ny):
        assert coast_o[below].any() and coast_o[above].any(), "no coast cell within kwin rows of a cut"
    for r0, r1 in bands:
        # (the band's own coast cells alone, swept in the same order: where that differs, the nearest source is a neighbour's)
        o_own = orc.get_dist(coast_o[r0:r1], land[r0:r1], lon, lat[r0:r1], maxdist=180.0, kwin=kwin)
        across = (np.abs(o[r0:r1]) < 12000.0) & (o_own != o[r0:r1])
        if r0 > 0:
            assert across[:kwin].any(), f"band {r0}:{r1}: no reached cell whose nearest source lies across its south cut"
        if r1 < ny:
            assert across[-kwin:].any(), f"band {r0}:{r1}: no reached cell whose nearest source lies across its north cut"

    # ---- edges, then the exchange of coast's ghost rows (numpy slices of the stacked interiors), then the distance ----
    coast = band_edges(hipctx, land, ice, bands, h, rule)
    assert np.array_equal(coast, coast_o)
    whole = hipctx.get_dist(coast, land, lon, lat, maxdist=180.0, kwin=kwin)
    got = band_dist(hipctx, coast, land, lon, lat, bands, h, kwin)
    diff = got.view(np.uint8).reshape(ny, -1) != whole.view(np.uint8).reshape(ny, -1)
    assert not diff.any(), f"rows {np.flatnonzero(diff.any(1))[:8]} differ from the whole-grid call in their bits"
    check_dist(got, o, f"{case[0]} set {cset} fp{8 * prec}", TOL[prec])

    # ---- the whole-grid entry point fed a band's own rows alone is wrong next to every cut ----
    for r0, r1 in bands:
        alone = hipctx.get_dist(coast[r0:r1], land[r0:r1], lon, lat[r0:r1], maxdist=180.0, kwin=kwin)
        if r0 > 0:
            assert not np.array_equal(alone[:kwin], whole[r0:r0 + kwin]), f"band {r0}:{r1} alone is right at its south cut"
        if r1 < ny:
            assert not np.array_equal(alone[-kwin:], whole[r1 - kwin:r1]), f"band {r0}:{r1} alone is right at its north cut"


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("nx,ny,kwin", [(320, 41, 15), (96, 37, 20), (24, 19, 15), (320, 45, 40)])
def test_one_band_owning_the_globe_without_halo(hipctx, nx, ny, kwin, prec):
    """south and north both set, halo = 0: the frame is the grid, the call is the whole-grid call."""
    dt = np.float64 if prec == 8 else np.float32
    lon, lat = coords(nx, ny, 1, dt)
    land, ice = land_ice(nx, ny, dt)
    for rule in (0, 1):
        whole = hipctx.get_edges(land, ice, rule=rule, bnd=hip.SB_BND_GLOBAL)
        assert np.array_equal(hipctx.band_get_edges(land, ice, 0, True, True, rule=rule), whole)
    coast = hipctx.get_edges(land, ice, rule=1, bnd=hip.SB_BND_GLOBAL)
    whole = hipctx.get_dist(coast, land, lon, lat, kwin=kwin)
    got = hipctx.band_get_dist(coast, land, lon, lat, 0, True, True, kwin)
    assert np.array_equal(got.view(np.uint8), whole.view(np.uint8))
    assert np.any(np.abs(whole) < 12000.0)


def test_band_dev_forms_and_kept_tables(hipctx, oracles):
    """The _dev forms on the library's own device memory; a second call with the same coordinates takes the kept tables."""
    dt, nx, heights, kwin, h = np.float64, 320, (33, 33, 33), 15, 16
    bands, ny = cuts_of(heights), sum(heights)
    lon, lat = coords(nx, ny, 1, dt)
    land, ice = land_ice(nx, ny, dt)
    coast_w = hipctx.get_edges(land, ice, rule=1, bnd=hip.SB_BND_GLOBAL)
    whole = hipctx.get_dist(coast_w, land, lon, lat, kwin=kwin)
    lib, r0, r1 = hipctx.lib, *bands[1]
    n = (r1 - r0 + 2 * h) * (nx + 2 * h)
    ptrs = []
    for _ in range(5):
        p = C.c_void_p()
        assert lib.sb_device_malloc(hipctx.h, C.c_size_t(n * 8), C.byref(p)) == 0
        ptrs.append(p)
    d_land, d_ice, d_coast, d_cd, d_cd2 = (p.value for p in ptrs)
    try:
        up = lambda d, a: hipctx._chk(lib.sb_device_upload(hipctx.h, C.c_void_p(d), hip._p(a), C.c_size_t(a.nbytes)), "upload")
        up(d_land, frame(land, r0, r1, h)); up(d_ice, frame(ice, r0, r1, h))
        sent = np.full((r1 - r0 + 2 * h, nx + 2 * h), SENTINEL, dt)
        up(d_coast, sent); up(d_cd, sent); up(d_cd2, sent)
        hipctx.band_get_edges_dev(dt, nx, r1 - r0, h, False, False, d_land, d_ice, d_coast, rule=1)
        hipctx.synchronize()
        cf = np.empty_like(sent)
        hipctx._chk(lib.sb_device_download(hipctx.h, hip._p(cf), C.c_void_p(d_coast), C.c_size_t(cf.nbytes)), "download")
        assert only_interior_written(cf, h) and np.array_equal(interior(cf, h), coast_w[r0:r1])
        up(d_coast, frame(coast_w, r0, r1, h))                    # (the exchange of coast's ghost rows)
        latf = frame_lat(lat, r0, r1, h)
        for d in (d_cd, d_cd2):
            hipctx.band_get_dist_dev(dt, nx, r1 - r0, h, False, False, d_coast, d_land, lon, latf, d, kwin)
        hipctx.synchronize()
        for d in (d_cd, d_cd2):
            out = np.empty_like(sent)
            hipctx._chk(lib.sb_device_download(hipctx.h, hip._p(out), C.c_void_p(d), C.c_size_t(out.nbytes)), "download")
            assert only_interior_written(out, h)
            assert np.array_equal(interior(out, h).view(np.uint8), whole[r0:r1].view(np.uint8))
    finally:
        for p in ptrs:
            lib.sb_device_free(hipctx.h, p)


def test_band_setup_refuses_bad_arguments(hipctx):
    dt, nx, ny, h = np.float64, 64, 12, 4
    f, m = np.zeros((ny + 2 * h, nx + 2 * h), dt), np.zeros((ny + 2 * h, nx + 2 * h), dt)
    lon, latf = coords(nx, ny + 2 * h, 1, dt)
    lib, I = hipctx.lib, C.c_int

    def dist(south, north, kwin, cdist=None):
        cd = np.zeros_like(f) if cdist is None else cdist
        return lib.sb_band_get_dist_f64(hipctx.h, I(nx), I(ny), I(h), I(south), I(north), hip._p(f), hip._p(m), hip._p(lon),
                                        hip._p(latf), C.c_double(180.0), I(kwin), hip._p(cd))

    SB_ERR_ARG = 1
    assert dist(0, 0, -1) == SB_ERR_ARG                                   # the derived window needs the global latitudes
    assert dist(1, 1, hip.SB_DIST_MAX_WINDOW + 1) == SB_ERR_ARG
    assert dist(0, 1, h + 1) == SB_ERR_ARG and dist(1, 0, h + 1) == SB_ERR_ARG   # kwin > halo with a cut side
    assert dist(1, 1, h + 1) == 0                                          # ... but not with both poles
    assert dist(0, 0, h, cdist=f) == SB_ERR_ARG                            # coast overlapping cdist
    assert dist(0, 0, h, cdist=f.reshape(-1)[8:]) == SB_ERR_ARG            # ... partly
    assert dist(0, 0, h) == 0
    z = np.zeros((ny, nx), dt)

    def edges(halo, south, north, a, rule=1):
        out = np.zeros_like(a)                                               # (held until the call has returned)
        return lib.sb_band_get_edges_f64(hipctx.h, I(nx), I(ny), I(halo), I(south), I(north), hip._p(a), hip._p(a), I(rule),
                                         hip._p(out))

    assert edges(0, 0, 1, z) == SB_ERR_ARG and edges(0, 1, 0, z) == SB_ERR_ARG   # halo < 1 with a cut side
    assert edges(0, 1, 1, z) == 0 and edges(h, 0, 0, f) == 0
    assert edges(h, 0, 0, f, rule=2) == SB_ERR_ARG
    with pytest.raises(hip.SeabreezeHipError):
        hipctx.band_get_dist(f, f, lon, latf, h, False, False, -1)
