"""search_radius without a GPU: the numpy model (tests/radius_ref.py) against the CPU oracle's own expanding windows, the
model against a cell-by-cell restatement of the loop, and the C ABI's new entry points."""
import ctypes as C

import numpy as np
import pytest

import radius_ref as rr
from seabreeze_param_amd import hip, synth

MAXDIST = 700.0


def _oracle_mask(orc, nx, ny, dt):
    st = synth.static_fields(nx, ny, dt)
    coast = orc.get_edges(st.landfrac, st.icefrac)
    return st, orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=MAXDIST)


@pytest.mark.parametrize("prec,dt", [(8, np.float64), (4, np.float32)])
@pytest.mark.parametrize("shape", [(96, 72), (200, 72)])
def test_model_largest_radius_is_the_oracles(oracles, prec, dt, shape):
    """The largest radius of the model's plane is the largest final nn of the oracle's windows, for the host-model flavour
    (SB_BND_GLOBAL) and for the f2py flavour (the wrapper rule: the column quirk, no band cell in the last row)."""
    nx, ny = shape
    nz = 2
    orc = oracles[prec]
    st, cdist = _oracle_mask(orc, nx, ny, dt)
    th = synth.theta_step(st, 1, dt)
    u, v = synth.wind_step(st, nz, 1, dt)
    tun = hip.Tunables()
    hip.load_library().sb_default_tunables(C.byref(tun))

    state = [np.zeros((ny, nx), dt) for _ in range(4)]
    orc.seabreeze_diag(5400.0, 1, synth.pressure_3d(st, nz, dt), u, v, th, cdist, st.z, st.sigma, *state, halo=0, bnd=1)
    r = rr.search_radius(cdist, tun.maxdist_km, 0, rr.BND_GLOBAL)
    s = rr.summary_of(r)
    assert s[3] >= 2 and s[2] == 0, s
    assert s[3] == orc.last_nn_max

    state = [np.zeros((ny, nx), dt) for _ in range(3)]
    orc.diag(1, synth.pressure_1d(nz, dt), st.z, st.sigma, th, v, u, cdist, *state, maxdist=MAXDIST, timestep=90.0)
    r = rr.search_radius(cdist, MAXDIST, 0, rr.BND_WRAPPER)
    s = rr.summary_of(r)
    assert s[3] >= 2 and s[2] == 0, s
    assert s[3] == orc.last_nn_max
    assert not r[ny - 1].any()                       # the wrapper rule: the last row is not a band row


def test_model_is_the_loop_cell_by_cell():
    """The ring-by-ring planes against contrast_global's loop at single cells: seams, poles, frames, bands."""
    rng = np.random.default_rng(7)
    for ny, nx, h in ((9, 13, 0), (20, 70, 0), (5, 130, 2), (12, 66, 3)):
        for p in (0.03, 0.5):
            m = np.where(rng.random((ny + 2 * h, nx + 2 * h)) < p, 1.0, -1.0)
            cells = [(int(rng.integers(nx)), int(rng.integers(ny))) for _ in range(8)] + [(nx - 1, 0), (0, ny - 1), (nx - 1, ny - 2)]
            variants = [(rr.BND_HALO, None), (rr.BND_HALO, (1, 0)), (rr.BND_HALO, (0, 1)), (rr.BND_HALO, (0, 0))]
            if h == 0:
                variants += [(rr.BND_GLOBAL, None), (rr.BND_WRAPPER, None)]
            for bnd, band in variants:
                plane = rr.search_radius(m, 1e9, h, bnd, band)
                for (x, y), r in rr.brute(m, 1e9, h, bnd, band, cells).items():
                    assert plane[y, x] == r, (ny, nx, h, p, bnd, band, x, y)


def test_model_classes_and_summary():
    m = -np.ones((6, 10))
    m[2, 3] = -0.0                                   # land side
    m[4, 7] = np.nan                                 # sea side, and a band cell whatever maxdist
    m[0, 0] = -5.0                                   # |mask| == maxdist: a band cell
    m[0, 1] = -5.0000001
    r = rr.search_radius(m, 5.0, 0, rr.BND_GLOBAL)
    assert r[2, 3] == 1 and r[4, 7] == 4 and r[0, 0] == 3 and r[0, 1] == 0
    assert rr.summary_of(r) == [int((np.abs(np.nan_to_num(m)) <= 5.0).sum()), int((r > 0).sum()), 0, int(r.max())]
    h = rr.hist_of(np.array([[0, -1, 1, 2, 2, 9]]), 4)
    assert h.tolist() == [1, 1, 2, 1]
    assert rr.regimes_of(np.array([16, 17, 32, 33, 127, 128, -1, 0])) == dict(strip=1, wide=2, table=2, beyond=1, none=1)
    assert hip.contrast_regimes(rr.hist_of(np.array([16, 17, 32, 33, 127, 128, 300, -1, 0]), 129)) == \
        dict(strip=1, wide=2, table=2, beyond=2, none=1)
    with pytest.raises(ValueError):
        hip.contrast_regimes(np.zeros(128))


def test_abi_exports_search_radius():
    lib = hip.load_library()
    for stem in ("sb_search_radius", "sb_band_search_radius"):
        for sfx in ("f32", "f64", "f32_dev", "f64_dev"):
            assert hasattr(lib, f"{stem}_{sfx}"), f"{stem}_{sfx} not exported"
    m = np.zeros((4, 4))
    r = np.zeros((4, 4), np.int32)
    s = (C.c_longlong * 4)()
    rc = lib.sb_search_radius_f64(None, C.c_int(4), C.c_int(4), C.c_int(0), C.c_int(1), m.ctypes.data_as(C.c_void_p),
                                  C.c_double(180.0), r.ctypes.data_as(C.c_void_p), s, None, C.c_int(0))
    assert rc == 1                                   # SB_ERR_ARG: no context
    rc = lib.sb_band_search_radius_f32(None, C.c_int(4), C.c_int(4), C.c_int(0), C.c_int(1), C.c_int(1), None,
                                       C.c_float(180.0), None, None, None, C.c_int(0))
    assert rc == 1
