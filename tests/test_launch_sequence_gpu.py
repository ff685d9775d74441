"""Which kernels a plain diag call launches: the launch plan (sb_diag_plan.hpp, the table in DESIGN.md section 2.3) as the
device sees it.  sb_last_step_report counts the launches, and the per-kernel timers of sb_profile_begin / sb_profile_end
answer 0.0 for a kernel the calls did not launch; the results are the oracle's under every sequence."""
import numpy as np
import pytest

from conftest import relerr
from oracle import fp32_criterion as crit
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

NX, NY, NZ, KWIN = 200, 96, 3, 5
f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


@pytest.fixture(scope="module")
def fields(oracles):
    """Static fields and coast distance per precision (fp32: the fp64 oracle's on the fp32-representable inputs)."""
    out = {}
    for dt in (np.float64, np.float32):
        st = synth.static_fields(NX, NY, dt)
        coast = oracles[8].get_edges(f8(st.landfrac), f8(st.icefrac))
        cd = oracles[8].get_dist(coast, f8(st.landfrac), st.lon, st.lat, maxdist=900.0, kwin=KWIN)
        cd[np.abs(cd) > 180.0] = 12000.0
        out[dt] = (st, cd.astype(dt))
    return out


def _kernels(ctx):
    ms, ncalls = ctx.profile_end()
    assert ncalls == 2
    return {k for k, v in ms.items() if v > 0.0}


# dtype, radius hint, fold, wide strip -> launches per call, kernels timed
GENERIC = [
    (np.float64, 6, True, True, 3, {"k_scan", "k_thc", "k_wind"}),                       # strip kernel does k_prep's work
    (np.float64, 6, False, True, 4, {"k_scan", "k_prep", "k_thc", "k_wind"}),
    (np.float64, 24, True, True, 4, {"k_scan", "k_prep", "k_thc", "k_wind"}),            # tile kernel
    (np.float32, 24, True, True, 3, {"k_scan", "k_thc", "k_wind"}),                      # 96-column strip kernel
    (np.float32, 24, True, False, 4, {"k_scan", "k_prep", "k_thc", "k_wind"}),           # tile kernel
]


@pytest.mark.parametrize("dt,hint,fold,wide,launches,kernels", GENERIC,
                         ids=["fp64-fold", "fp64-kprep", "fp64-tiles", "fp32-strip32", "fp32-tiles"])
def test_host_model_call(oracles, fields, dt, hint, fold, wide, launches, kernels):
    orc8 = oracles[8]
    st, cd = fields[dt]
    p = synth.pressure_3d(st, NZ, dt)
    sh = [np.zeros((NY, NX), dt) for _ in range(4)]
    so = [np.zeros((NY, NX), np.float64) for _ in range(4)]
    band = np.abs(f8(cd)) <= 180.0
    ctx = hip.Context(0)
    try:
        ctx.set_search_radius_hint(hint)
        ctx.set_fold(fold)
        ctx.set_wide_strip(wide)
        ctx.profile_begin(2)
        for tn in (1, 2):
            th = synth.theta_step(st, tn, dt)
            u, v = synth.wind_step(st, NZ, tn, dt)
            gp, op = [a.copy() for a in sh], [a.copy() for a in so]
            ctx.seabreeze_diag(5400.0, tn, p, u, v, th, cd, st.z, st.sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
            assert ctx.last_step_report() == dict(kernel_launches=launches, rccl_ops=0, rccl_groups=0, d2d_copies=0)
            orc8.seabreeze_diag(5400.0, tn, f8(p), f8(u), f8(v), f8(th), f8(cd), f8(st.z), f8(st.sigma), *so, halo=0, bnd=1)
            if dt == np.float64:
                for nm, a, b in zip(("ws", "wd", "thc", "sb_con"), sh, so):
                    assert relerr(a, b, floor=1e-2) < 1e-7, f"step {tn} {nm}"
            else:
                res = crit.check_step(tn, gp, sh, op, so, band, timestep=5400.0)
                assert crit.merge([res])["ok"], res
        assert _kernels(ctx) == kernels
    finally:
        ctx.close()


def test_f2py_call(oracles, fields):
    """The f2py entry point: k_t0 writes the t0 plane between k_prep and the contrast kernel -- five launches."""
    dt, orc = np.float64, oracles[8]
    st, cd = fields[dt]
    p = synth.pressure_1d(NZ, dt)
    wh = [np.zeros((NY, NX), dt) for _ in range(3)]
    wo = [np.zeros((NY, NX), dt) for _ in range(3)]
    ctx = hip.Context(0)
    try:
        ctx.set_search_radius_hint(6)
        ctx.profile_begin(2)
        for tn in (1, 2):
            th = synth.theta_step(st, tn, dt)
            u, v = synth.wind_step(st, NZ, tn, dt)
            oh = ctx.diag(tn, p, st.z, st.sigma, th, v, u, cd, *wh)
            assert ctx.last_step_report()["kernel_launches"] == 5
            oo = orc.diag(tn, p, st.z, st.sigma, th, v, u, cd, *wo)
            for k, nm in enumerate(("sb_con", "t0", "windspeed", "winddir")):
                assert relerr(oh[k, :-1], oo[k, :-1], floor=1e-2) < 1e-7, f"step {tn} {nm}"
            for nm, a, b in zip(("ws", "wd", "thc"), wh, wo):
                assert relerr(a, b, floor=1e-2) < 1e-7, f"step {tn} state {nm}"
        assert _kernels(ctx) == {"k_scan", "k_prep", "k_t0", "k_thc", "k_wind"}
    finally:
        ctx.close()
