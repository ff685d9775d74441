"""UM-layout coast setup on curvilinear (rotated-pole) grids: sb_get_edges_um_* and sb_get_dist_um_* through the C ABI,
against the numpy restatement of the UM vn10.7 copy (tests/um_setup_ref.py).  The UM file cannot be compiled, so this
parity is unpinned by nature (as for seabreeze_diag_um); test_dist_um_regular_anchor ties the arithmetic to the pinned
regular-grid oracle.

Tolerances are those of tests/test_setup_gpu.py::_check_dist: cells without a coast in reach (12000) and signs
identical, distances to 1e-12 (fp64) / 2e-6 (fp32) relative.  The coast mask is bit-exact.
"""
import numpy as np
import pytest
import torch

import um_setup_ref as ur
from conftest import relerr
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _check_dist(h, o, what, rel):
    assert np.array_equal(h >= 12000.0, o >= 12000.0), f"{what}: cells without a coast in reach differ"
    assert np.array_equal(np.sign(h), np.sign(o)), f"{what}: signs differ"
    e = np.abs(h.astype(np.float64) - o) / np.maximum(np.abs(o.astype(np.float64)), 1.0)
    assert e.max() <= rel, f"{what}: max rel err {e.max()}"


def _sentinel_field(shape, dt, hi, hj):
    """A field whose ghost cells hold SENTINEL (and whose interior holds another value) -- what must survive."""
    f = np.full(shape, SENTINEL, dt)
    f[hj:shape[0] - hj, hi:shape[1] - hi] = 3.5
    return f


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("halo", [(1, 1), (2, 5), (5, 2)])
@pytest.mark.parametrize("shape", [(258, 7), (70, 33), (513, 17), (5, 4)])
def test_edges_um_bit_exact(hipctx, shape, halo, prec):
    nx, ny = shape
    hi, hj = halo
    dt = np.float64 if prec == 8 else np.float32
    # fractional land and ice over the whole field: the ghost ring holds coast of its own, both ice branches are taken
    lf_l, ci_l = ur.noise_mask(nx + 2 * hi, ny + 2 * hj, 41, dt, frac=True)
    assert (ci_l > 0.2).any() and (ci_l <= 0.2).any()
    out = _sentinel_field(lf_l.shape, dt, hi, hj)
    h = hipctx.get_edges_um(lf_l, ci_l, hi, hj, out=out.copy())
    o = ur.edges_um(lf_l, ci_l, hi, hj, out=out)
    assert np.array_equal(h, o), f"{shape} {halo}: {np.count_nonzero(h != o)} cells differ"
    assert np.all(h[:hj] == SENTINEL) and np.all(h[:, :hi] == SENTINEL)


def _grid_for(halo):
    return sorted(ur.GRIDS)[sum(halo) % 3]


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("halo", [(0, 0), (1, 3), (5, 5), (7, 15), (15, 15), (31, 7), (31, 31)])
def test_dist_um_vs_literal(hipctx, halo, prec):
    hi, hj = halo
    nx, ny = (90, 70) if max(halo) < 31 else (100, 72)
    dt = np.float64 if prec == 8 else np.float32
    lat, lon = ur.grid_named(_grid_for(halo), nx, ny, dt)
    for maker, seed in ((ur.noise_mask, 11), (ur.sparse_mask, 12)):
        land, ice = maker(nx, ny, seed, dt)
        _, _, coast_l = ur.coast_of(land, ice, hi, hj)
        for maxdist in (180.0, 900.0):
            out = _sentinel_field(coast_l.shape, dt, hi, hj)
            h = hipctx.get_dist_um(coast_l, land, lat, lon, hi, hj, maxdist=maxdist, out=out.copy())
            o = ur.dist_um_literal(coast_l, land, lat, lon, hi, hj, maxdist=maxdist, out=out)
            ghost = out == SENTINEL
            assert np.array_equal(h[ghost], out[ghost]), "ghost cells of cdist were written"
            _check_dist(h, o, f"{maker.__name__} halo={halo} maxdist={maxdist}", 1e-12 if prec == 8 else 2e-6)


def test_dist_um_ghost_ring_sources_and_no_wrap(hipctx):
    dt, hi, hj, nx, ny = np.float64, 15, 4, 40, 12
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    land = np.zeros((ny, nx), dt)
    # coast only in the ghost cells of the input: nothing is reached
    coast_l = np.ones((ny + 2 * hj, nx + 2 * hi), dt)
    coast_l[hj:hj + ny, hi:hi + nx] = 0.0
    h = hipctx.get_dist_um(coast_l, land, lat, lon, hi, hj)
    assert np.all(h[hj:hj + ny, hi:hi + nx] == 12000.0)
    # one coast cell just inside the left edge: reaches columns 0 .. 16 of rows 1 .. 9, never the right edge (no wrap)
    coast_l[:] = 0.0
    coast_l[hj + 5, hi + 1] = 1.0
    h = hipctx.get_dist_um(coast_l, land, lat, lon, hi, hj)[hj:hj + ny, hi:hi + nx]
    reached = h < 12000.0
    assert reached[1:10, :17].all() and not reached[:, 17:].any() and not reached[0].any() and not reached[10:].any()
    o = ur.dist_um_literal(coast_l, land, lat, lon, hi, hj)[hj:hj + ny, hi:hi + nx]
    _check_dist(h, o, "one source", 1e-12)


@pytest.mark.parametrize("prec", [8, 4])
def test_dist_um_in_place(hipctx, prec):
    """cdist is coast (the UM overwrites coast): the same field as out of place, on the device."""
    dt = np.float64 if prec == 8 else np.float32
    tdt = torch.float64 if prec == 8 else torch.float32
    nx, ny, hi, hj = 300, 90, 15, 15
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    land, ice = ur.noise_mask(nx, ny, 13, dt)
    _, _, coast_l = ur.coast_of(land, ice, hi, hj)
    ref = hipctx.get_dist_um(coast_l, land, lat, lon, hi, hj)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    co, lf, la, lo = dev(coast_l), dev(land), dev(lat), dev(lon)
    assert co.dtype == tdt
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    hipctx.get_dist_um_dev(dt, nx, ny, hi, hj, co.data_ptr(), lf.data_ptr(), la.data_ptr(), lo.data_ptr(), co.data_ptr(),
                           stream=s.cuda_stream)
    s.synchronize()
    got = co.cpu().numpy()
    inner = (slice(hj, hj + ny), slice(hi, hi + nx))
    assert np.array_equal(got[inner], ref[inner])
    ghost = np.ones(coast_l.shape, bool)
    ghost[inner] = False
    assert np.array_equal(got[ghost], coast_l[ghost])


def test_dist_um_regular_anchor(hipctx, oracles):
    """A regular grid written as 2-D coordinates, every coast cell at least k cells inside every edge (so neither the
    oracle's wrap nor its clamp comes into play), longitudes below 180 (l1 and l2 coincide): get_dist_um with
    halo_i = halo_j = k is the pinned regular-grid get_dist with kwin = k."""
    dt, orc = np.float64, oracles[8]
    nx, ny = 160, 96
    lon = 100.0 + 0.25 * np.arange(nx)
    lat = -30.0 + 0.2 * np.arange(ny)
    lat2, lon2 = (np.ascontiguousarray(a) for a in np.meshgrid(lat, lon, indexing="ij"))
    land, _ = ur.noise_mask(nx, ny, 17, dt)
    for k in (3, 9, 15):
        coast = (synth.hash_uniform((ny, nx), 7, 17) > 0.97).astype(dt)
        coast[:k] = 0.0
        coast[ny - k:] = 0.0
        coast[:, :k] = 0.0
        coast[:, nx - k:] = 0.0
        for maxdist in (60.0, 180.0):
            o = orc.get_dist(coast, land, lon, lat, maxdist=maxdist, kwin=k)
            coast_l = np.ascontiguousarray(np.pad(coast, k))
            h = hipctx.get_dist_um(coast_l, land, lat2, lon2, k, k, maxdist=maxdist)[k:k + ny, k:k + nx]
            _check_dist(h, o, f"anchor k={k} maxdist={maxdist}", 1e-12)


@pytest.mark.parametrize("prec", [8, 4])
def test_um_setup_then_diag_end_to_end(hipctx, oracles, prec):
    """get_edges_um -> get_dist_um on a rotated grid, ghosts by edge padding, then seabreeze_diag_um over 3 steps against
    the oracle's raw-index flavour fed the restatement's distance field (tolerances of test_um_layout_halo2)."""
    nx, ny, nz, hs, hl = 120, 70, 6, 3, 5
    dt = np.float64 if prec == 8 else np.float32
    orc = oracles[prec]
    st = synth.static_fields(nx + 2 * hl, ny + 2 * hl, dt)                 # a bigger field whose rim serves as ghosts
    # a binary land mask without sea ice and with open sea near the edges, on a ~67 km grid: every coastal-band cell
    # then finds land and sea within hs cells, so the oracle's raw-index reads stay inside its ghost frame
    land = (st.landfrac >= 0.5).astype(dt)
    f = hl + 4
    land[:f] = 0; land[-f:] = 0; land[:, :f] = 0; land[:, -f:] = 0
    st.landfrac, st.icefrac = np.ascontiguousarray(land), np.zeros_like(land)
    lat, lon = ur.grid_named("dateline", nx, ny, dt, dlon=0.6, dlat=0.6)
    core = (slice(hl, hl + ny), slice(hl, hl + nx))
    lf = np.ascontiguousarray(st.landfrac[core])
    coast_h = hipctx.get_edges_um(st.landfrac, st.icefrac, hl, hl)
    coast_o = ur.edges_um(st.landfrac, st.icefrac, hl, hl)
    assert np.array_equal(coast_h, coast_o)
    cd_h = hipctx.get_dist_um(coast_h, lf, lat, lon, hl, hl, maxdist=180.0)
    cd_o = ur.dist_um_vectorised(coast_o, lf, lat, lon, hl, hl, maxdist=180.0)
    _check_dist(cd_h, cd_o, "end to end", 1e-12 if prec == 8 else 2e-6)
    assert np.count_nonzero(np.abs(cd_o[core]) <= 180.0) > 500          # a coastal band to work on
    cd_h = ur.pad_edge(cd_h[core], hl, hl)
    cd_o = ur.pad_edge(cd_o[core], hl, hl)
    inner = lambda a, h: np.ascontiguousarray(a[hl - h:a.shape[0] - (hl - h), hl - h:a.shape[1] - (hl - h)])
    p = synth.pressure_3d(st, nz, dt)[:, core[0], core[1]].copy()
    so = [np.zeros((ny, nx), dt) for _ in range(4)]
    sh = [np.zeros((ny, nx), dt) for _ in range(4)]
    flags = hip.SB_UM_THETA_TO_T0 | hip.SB_UM_LEVEL_WALK
    for tn in range(1, 4):
        th_l = synth.theta_step(st, tn, dt)
        u, v = (a[:, core[0], core[1]].copy() for a in synth.wind_step(st, nz, tn, dt))
        th_s, z_s, sg_s = inner(th_l, hs), inner(st.z, hs), inner(st.sigma, hs)
        orc.seabreeze_diag(7200.0, tn, p, u, v, th_s, inner(cd_o, hs), z_s, sg_s, *so, halo=hs, bnd=2, level_rule=1)
        err = hipctx.seabreeze_diag_um(7200.0, tn, p, u, v, th_s.copy(), z_s, sg_s, cd_h, *sh, halo_s=hs, halo_l=hl,
                                       flags=flags)
        assert err == 0
        for a, b, nm in zip(sh, so, ("ws", "wd", "thc", "sb_con")):
            assert np.array_equal(np.isnan(a), np.isnan(b)), (nm, tn)
            if prec == 8:
                assert relerr(a, b, floor=1e-2) < 1e-7, (nm, tn)
            elif nm in ("ws", "wd"):
                assert relerr(a, b, floor=1e-1) < 2e-5, (nm, tn)
            elif nm == "thc":
                assert np.nanmax(np.abs(a - b)) < 2e-3, tn
    c = hipctx.last_counters()
    assert c["one_class_cells"] == 0 and 1 <= c["max_radius"] <= hs


@pytest.mark.parametrize("prec", [8, 4])
def test_um_setup_dev_forms_on_torch_stream(hipctx, prec):
    """get_edges_um_dev -> get_dist_um_dev on one torch stream, no synchronisation between them: the host forms' fields."""
    dt = np.float64 if prec == 8 else np.float32
    nx, ny, hi, hj = 333, 150, 7, 12
    lf_l, ci_l = ur.noise_mask(nx + 2 * hi, ny + 2 * hj, 23, dt, frac=True)
    lat, lon = ur.grid_named("west", nx, ny, dt)
    lf = np.ascontiguousarray(lf_l[hj:hj + ny, hi:hi + nx])
    coast_ref = hipctx.get_edges_um(lf_l, ci_l, hi, hj)
    cd_ref = hipctx.get_dist_um(coast_ref, lf, lat, lon, hi, hj, maxdist=300.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    dl, dc, dlf, dla, dlo = dev(lf_l), dev(ci_l), dev(lf), dev(lat), dev(lon)
    co = torch.zeros_like(dl)
    cd = torch.zeros_like(dl)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sh = s.cuda_stream
        hipctx.get_edges_um_dev(dt, nx, ny, hi, hj, dl.data_ptr(), dc.data_ptr(), co.data_ptr(), stream=sh)
        hipctx.get_dist_um_dev(dt, nx, ny, hi, hj, co.data_ptr(), dlf.data_ptr(), dla.data_ptr(), dlo.data_ptr(),
                               cd.data_ptr(), maxdist=300.0, stream=sh)
    s.synchronize()
    assert np.array_equal(co.cpu().numpy(), coast_ref)
    assert np.array_equal(cd.cpu().numpy(), cd_ref)


def test_dist_um_full_size(hipctx):
    """2560 x 1920 rotated grid (about 4 km), halo 15, fp64: every cell against the vectorised restatement."""
    nx, ny, h, dt = 2560, 1920, 15, np.float64
    st = synth.static_fields(nx + 2 * h, ny + 2 * h, dt)
    lat, lon = ur.grid_named("dateline", nx, ny, dt, dlon=0.036, dlat=0.036)
    lf = np.ascontiguousarray(st.landfrac[h:h + ny, h:h + nx])
    coast_l = hipctx.get_edges_um(st.landfrac, st.icefrac, h, h)
    assert np.array_equal(coast_l, ur.edges_um(st.landfrac, st.icefrac, h, h))
    cd = hipctx.get_dist_um(coast_l, lf, lat, lon, h, h, maxdist=180.0)
    o = ur.dist_um_vectorised(coast_l, lf, lat, lon, h, h, maxdist=180.0)
    _check_dist(cd, o, "2560x1920 halo 15", 1e-12)
    inner = cd[h:h + ny, h:h + nx]
    assert (inner < 12000.0).sum() > 0.05 * inner.size


def test_um_setup_argument_errors(hipctx):
    dt = np.float64
    nx, ny = 40, 30
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    land = np.zeros((ny, nx), dt)
    with pytest.raises(hip.SeabreezeHipError, match="halo_i, halo_j <= 31"):
        hipctx.get_dist_um(np.zeros((ny + 64, nx + 2), dt), land, lat, lon, 1, 32)
    with pytest.raises(hip.SeabreezeHipError, match="halo_i, halo_j <= 31"):
        hipctx.get_dist_um(np.zeros((ny, nx + 64), dt), land, lat, lon, 32, 0)
    with pytest.raises(hip.SeabreezeHipError, match=">= 1"):
        hipctx.get_edges_um(np.zeros((ny + 2, nx), dt), np.zeros((ny + 2, nx), dt), 0, 1)
    with pytest.raises(hip.SeabreezeHipError, match=">= 1"):
        hipctx.get_edges_um(np.zeros((ny, nx + 2), dt), np.zeros((ny, nx + 2), dt), 1, 0)
    lib, h = hipctx.lib, hipctx.h
    import ctypes as C
    buf = np.zeros((ny + 2, nx + 2), dt)
    p = C.c_void_p(buf.ctypes.data)
    for fn in ("sb_get_dist_um_f64", "sb_get_dist_um_f64_dev"):
        args = [h, C.c_int(nx), C.c_int(ny), C.c_int(1), C.c_int(1), p, p, None, p, C.c_double(180.0), p]
        if fn.endswith("_dev"):
            args.append(None)
        assert getattr(lib, fn)(*args) == 1
    for fn in ("sb_get_edges_um_f64", "sb_get_edges_um_f64_dev"):
        args = [h, C.c_int(nx), C.c_int(ny), C.c_int(1), C.c_int(1), p, None, p]
        if fn.endswith("_dev"):
            args.append(None)
        assert getattr(lib, fn)(*args) == 1
    assert lib.sb_get_dist_um_f64(None, C.c_int(nx), C.c_int(ny), C.c_int(1), C.c_int(1), p, p, p, p, C.c_double(1.0), p) == 1
