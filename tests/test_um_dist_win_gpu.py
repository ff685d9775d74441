"""sb_get_dist_um_win_*: the UM-layout coast distance with the window (up to SB_DIST_UM_MAX_WINDOW = 255 cells each way)
stated apart from the layout's ghost width, against the numpy restatement of the UM's get_dist on a field re-padded to the
window (tests/um_win_ref.py; its inputs are shown to hold every class of cell in tests/test_um_dist_win_host.py).

Tolerances are the project's (tests/test_um_setup_gpu.py::_check_dist): 12000-cells and signs identical, distances to
1e-12 (fp64) / 2e-6 (fp32) relative with denominator max(|o|, 1).
"""
import numpy as np
import pytest
import torch

import um_setup_ref as ur
import um_win_ref as uw
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

GRIDS = sorted(ur.GRIDS)
HALOS = ((0, 0), (1, 1), (3, 2))
DT_S = 7200.0


def _dt(prec):
    return np.float64 if prec == 8 else np.float32


def _rel(prec):
    return 1e-12 if prec == 8 else 2e-6


def _parity(ctx, what, lat, lon, land, coast_l, halo, win, maxdist, prec):
    """The library against the literal restatement, ghost cells of cdist holding a sentinel that must survive."""
    (hi, hj), (wi, wj), dt = halo, win, _dt(prec)
    out = uw.sentinel_field(coast_l.shape, dt, hi, hj)
    h = ctx.get_dist_um_win(coast_l, land, lat, lon, hi, hj, wi, wj, maxdist=maxdist, out=out.copy())
    o = uw.dist_win_literal(coast_l, land, lat, lon, hi, hj, wi, wj, maxdist, out=out)
    ghost = out == uw.SENTINEL
    assert h.dtype == dt and np.array_equal(h[ghost], out[ghost]), f"{what}: ghost cells of cdist were written"
    uw.check_dist(h, o, what, _rel(prec))
    return h, o


# ---- 1: parity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("case", list(enumerate([(32, 32), (31, 32), (32, 0), (0, 40), (40, 33)])))
def test_first_wide_windows_on_dense_and_sparse_coasts(hipctx, case, prec):
    """100 x 72 at 0.11 degrees, layout halos that differ from the window"""
    k, win = case
    nx, ny, dt = 100, 72, _dt(prec)
    halo = HALOS[k % 3]
    lat, lon = ur.grid_named(GRIDS[k % 3], nx, ny, dt)
    for maker, seed in ((ur.noise_mask, 11), (ur.sparse_mask, 12)):
        land, ice = maker(nx, ny, seed, dt)
        _, _, coast_l = ur.coast_of(land, ice, *halo)
        _parity(hipctx, f"{maker.__name__} win={win} halo={halo}", lat, lon, land, coast_l, halo, win, 180.0, prec)


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("case", list(enumerate([((113, 113), 180.0), ((113, 40), 30.0), ((40, 113), 30.0)])))
def test_seven_islands_at_km_scale(hipctx, case, prec):
    """300 x 250 at 0.0135 degrees: several passes of source rows, reset cells and cells reached beyond 2*maxdist"""
    k, (win, maxdist) = case
    halo = HALOS[(k + 1) % 3]
    lat, lon, land, coast_l = uw.islands_case(GRIDS[k % 3], _dt(prec), *halo)
    h, o = _parity(hipctx, f"islands win={win}", lat, lon, land, coast_l, halo, win, maxdist, prec)
    assert (o >= 12000.0).any() and (np.abs(o) < 12000.0).any()


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("case", list(enumerate([(255, 255), (255, 3)])))
def test_the_limit_on_a_grid_narrower_than_the_window(hipctx, case, prec):
    k, win = case
    nx, ny, dt = 70, 50, _dt(prec)
    halo = HALOS[(k + 2) % 3]
    lat, lon = ur.grid_named(GRIDS[(k + 1) % 3], nx, ny, dt)
    for maker, seed in ((ur.noise_mask, 21), (ur.sparse_mask, 22)):
        land, ice = maker(nx, ny, seed, dt)
        _, _, coast_l = ur.coast_of(land, ice, *halo)
        _parity(hipctx, f"{maker.__name__} win={win}", lat, lon, land, coast_l, halo, win, 180.0, prec)


@pytest.mark.parametrize("prec", [8, 4])
def test_ragged_workgroups_sharing_sources(hipctx, prec):
    """333 x 41 at 0.036 degrees, window 40: a ragged last workgroup and last bit word, six workgroup columns"""
    nx, ny, dt, halo = 333, 41, _dt(prec), (1, 1)
    lat, lon = ur.grid_named("polar", nx, ny, dt, dlon=0.036, dlat=0.036)
    land, ice = ur.sparse_mask(nx, ny, 31, dt)
    _, _, coast_l = ur.coast_of(land, ice, *halo)
    _parity(hipctx, "333x41", lat, lon, land, coast_l, halo, (40, 40), 180.0, prec)


# ---- 2, 3: windows of at most 31 cells ---------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("halo", [(15, 15), (31, 7)])
def test_window_equal_to_halo_is_get_dist_um(hipctx, halo, prec):
    hi, hj = halo
    nx, ny, dt = 100, 72, _dt(prec)
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    land, ice = ur.noise_mask(nx, ny, 11, dt)
    _, _, coast_l = ur.coast_of(land, ice, hi, hj)
    a = hipctx.get_dist_um_win(coast_l, land, lat, lon, hi, hj, hi, hj, maxdist=180.0)
    b = hipctx.get_dist_um(coast_l, land, lat, lon, hi, hj, maxdist=180.0)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("win,halo", [((15, 7), (2, 20)), ((5, 31), (0, 0))])
def test_small_window_with_another_halo(hipctx, win, halo, prec):
    nx, ny, dt = 100, 72, _dt(prec)
    lat, lon = ur.grid_named("west", nx, ny, dt)
    land, ice = ur.noise_mask(nx, ny, 11, dt)
    _, _, coast_l = ur.coast_of(land, ice, *halo)
    _parity(hipctx, f"win={win} halo={halo}", lat, lon, land, coast_l, halo, win, 180.0, prec)


# ---- 4: in place -------------------------------------------------------------------------------------------------------

def test_in_place(hipctx):
    """out is coast_l (the UM overwrites coast), window (113, 40)"""
    halo, win, dt = (3, 2), (113, 40), np.float64
    lat, lon, land, coast_l = uw.islands_case("west", dt, *halo)
    ref = hipctx.get_dist_um_win(coast_l, land, lat, lon, *halo, *win, maxdist=30.0)
    field = coast_l.copy()
    got = hipctx.get_dist_um_win(field, land, lat, lon, *halo, *win, maxdist=30.0, out=field)
    assert got is field and np.array_equal(field, ref)
    uw.check_dist(field, uw.dist_win_literal(coast_l, land, lat, lon, *halo, *win, 30.0), "in place", 1e-12)


# ---- 5: refusals -------------------------------------------------------------------------------------------------------

def test_windows_beyond_the_limit_are_refused(hipctx):
    nx, ny, dt = 40, 30, np.float64
    lat, lon = ur.grid_named("dateline", nx, ny, dt)
    land, ice = ur.noise_mask(nx, ny, 7, dt)
    _, _, coast_l = ur.coast_of(land, ice, 1, 1)
    for win in ((hip.SB_DIST_UM_MAX_WINDOW + 1, 3), (3, hip.SB_DIST_UM_MAX_WINDOW + 1), (-1, 3), (3, -1)):
        with pytest.raises(hip.SeabreezeHipError) as err:
            hipctx.get_dist_um_win(coast_l, land, lat, lon, 1, 1, *win)
        assert "255" in str(err.value) and "SB_DIST_UM_MAX_WINDOW" in str(err.value), str(err.value)
    _parity(hipctx, "after the refusals", lat, lon, land, coast_l, (1, 1), (33, 5), 180.0, 8)


# ---- 6: the _dev form --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [8, 4])
def test_dev_forms_on_torch_stream(hipctx, prec):
    """get_edges_um_dev -> get_dist_um_win_dev on one torch stream, no synchronisation between them: the host forms' fields"""
    dt = _dt(prec)
    nx, ny, hi, hj, wi, wj = 333, 150, 7, 12, 40, 36
    lf_l, ci_l = ur.noise_mask(nx + 2 * hi, ny + 2 * hj, 23, dt, frac=True)
    lat, lon = ur.grid_named("west", nx, ny, dt)
    lf = np.ascontiguousarray(lf_l[hj:hj + ny, hi:hi + nx])
    coast_ref = hipctx.get_edges_um(lf_l, ci_l, hi, hj)
    cd_ref = hipctx.get_dist_um_win(coast_ref, lf, lat, lon, hi, hj, wi, wj, maxdist=300.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    dl, dc, dlf, dla, dlo = dev(lf_l), dev(ci_l), dev(lf), dev(lat), dev(lon)
    co = torch.zeros_like(dl)
    cd = torch.zeros_like(dl)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sh = s.cuda_stream
        hipctx.get_edges_um_dev(dt, nx, ny, hi, hj, dl.data_ptr(), dc.data_ptr(), co.data_ptr(), stream=sh)
        hipctx.get_dist_um_win_dev(dt, nx, ny, hi, hj, wi, wj, co.data_ptr(), dlf.data_ptr(), dla.data_ptr(), dlo.data_ptr(),
                                   cd.data_ptr(), maxdist=300.0, stream=sh)
    s.synchronize()
    assert np.array_equal(co.cpu().numpy(), coast_ref)
    assert np.array_equal(cd.cpu().numpy(), cd_ref)
    assert (np.abs(cd_ref[hj:hj + ny, hi:hi + nx]) < 12000.0).any()


# ---- 7: the distance field feeds the table contrast ------------------------------------------------------------------------

def test_chain_into_the_table_contrast(hipctx):
    """A rotated 320 x 400 grid at 0.0135 degrees, land south of the middle row: get_edges_um, get_dist_um_win (113 cells)
    and two seabreeze_diag_um steps with sb_set_table_contrast, 116 ghost cells so that no window is cut.  k_scan reads
    the mask only through its sign and the band test, and no reference distance lies near maxdist
    (tests/test_um_dist_win_host.py::test_chain_field_is_off_the_knife_edge), so the steps fed by the library's field and by
    the reference's must give the same bits and the same counters."""
    c, g = uw.CHAIN, uw.chain_case()
    nx, ny, h, w, nz, dt = c["nx"], c["ny"], c["halo"], c["win"], 3, np.float64
    coast_l = hipctx.get_edges_um(g["lf_l"], g["ci_l"], h, h)
    assert np.array_equal(coast_l, g["coast_l"])
    cd = hipctx.get_dist_um_win(coast_l, g["lf"], g["lat"], g["lon"], h, h, w, w, maxdist=c["maxdist"])
    core = (slice(h, h + ny), slice(h, h + nx))
    uw.check_dist(cd[core], g["ref"][core], "chain", 1e-12)
    cd = ur.pad_edge(cd[core], h, h)

    st = synth.static_fields(nx + 2 * h, ny + 2 * h, dt)                   # a bigger field whose rim serves as ghosts
    p = synth.pressure_3d(st, nz, dt)[:, core[0], core[1]].copy()
    flags = hip.SB_UM_THETA_TO_T0 | hip.SB_UM_LEVEL_WALK
    other = hip.Context()
    try:
        res = []
        for ctx, mask in ((hipctx, cd), (other, g["ref"])):
            ctx.set_table_contrast(True)
            state = [np.zeros((ny, nx), dt) for _ in range(4)]
            counters = []
            for tn in (1, 2):
                th = synth.theta_step(st, tn, dt)
                u, v = (a[:, core[0], core[1]].copy() for a in synth.wind_step(st, nz, tn, dt))
                assert ctx.seabreeze_diag_um(DT_S, tn, p, u, v, th.copy(), st.z, st.sigma, mask, *state, halo_s=h, halo_l=h,
                                             flags=flags) == 0
                counters.append(ctx.last_counters())
            res.append((state, counters))
    finally:
        hipctx.set_table_contrast(False)
        other.close()
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b, equal_nan=True)
    assert res[0][1] == res[1][1]
    band = np.abs(g["ref"][core]) <= c["maxdist"]
    for cnt in res[0][1]:
        assert cnt["band_cells"] >= np.count_nonzero(band) and cnt["max_radius"] <= h, cnt
