"""The marching-strip kernels answer a window from exact integer sums, so thc does not depend on the plan (claim (c) of
sb_strip_kernel.hip's header): the call that plans -- `query` finds every radius in the LDS tables and lists the cells --
and the calls that march by the stored plan -- `query` takes radius, count and class from the stored lists -- leave the
same bits, and so does a call that plans again.  The planner and the lists are shared code (sb_strip_common.hpp); the
two paths of `query` are each kernel's own.  ref: generic/sea_breeze_diag.f90:188-216."""
import numpy as np
import pytest

from seabreeze_param_amd import hip, synth
from test_strip32_gpu import _case

pytestmark = pytest.mark.gpu


def _thc_of_four_calls(ctx, st, cd, dt):
    """thc after three calls on identical inputs (plan, stored plan, stored plan) and a fourth that plans again"""
    ny, nx = cd.shape
    nz = 2
    p = synth.pressure_3d(st, nz, dt)
    th = synth.theta_step(st, 1, dt)
    u, v = synth.wind_step(st, nz, 1, dt)
    state = [np.zeros((ny, nx), dt) for _ in range(4)]
    out = []
    try:
        ctx.set_plan_cache(True)
        for tn in (1, 2, 3, 4):
            if tn == 4:
                ctx.set_plan_cache(False)
            ctx.seabreeze_diag(7200.0, tn, p, u, v, th, cd, st.z, st.sigma, *state, halo=0, bnd=hip.SB_BND_GLOBAL)
            out.append(state[2].copy())
    finally:
        ctx.set_plan_cache(True)
    return out


def _assert_same_bits(out, dt):
    bits = np.uint64 if dt == np.float64 else np.uint32
    assert np.count_nonzero(out[0]) > 0               # (a contrast was formed at all)
    for k in (1, 2, 3):
        differ = np.count_nonzero(out[k].view(bits) != out[0].view(bits))
        print(f"call {k + 1} against call 1: {differ} cells differ")
        assert np.array_equal(out[k].view(bits), out[0].view(bits)), f"call {k + 1}: {differ} cells differ"


def test_k_strip_thc_is_independent_of_the_plan(hipctx, oracles):
    nx, ny, dt, orc = 256, 192, np.float64, oracles[8]
    st = synth.static_fields(nx, ny, dt)
    coast = orc.get_edges(st.landfrac, st.icefrac)
    cd = orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=700.0)
    cd[np.abs(cd) > 180.0] = 12000.0                  # the host model's distance field holds the fill beyond maxdist
    hipctx.set_search_radius_hint(16)                 # (the default)
    _assert_same_bits(_thc_of_four_calls(hipctx, st, cd, dt), dt)


def test_k_strip32_thc_is_independent_of_the_plan(hipctx, oracles):
    dt = np.float32
    st, cd = _case(oracles[8], 256, 192, kwin=27)
    hipctx.set_search_radius_hint(30)
    try:
        out = _thc_of_four_calls(hipctx, st, cd, dt)
        assert 16 < hipctx.last_counters()["max_radius"] <= 31      # (k_strip32's radii)
    finally:
        hipctx.set_search_radius_hint(16)
    _assert_same_bits(out, dt)
