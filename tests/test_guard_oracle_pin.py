"""The yardstick of tests/test_nonfinite_guard_gpu.py on missing and non-finite temperatures, before anything is held to it.

On 96 x 72 with the bad cells of that file's cases in theta (and z), oracle/sb_oracle.f90's library and the reference's own
wrapper files compiled unmodified (oracle/_ref; skipped where it is not built) agree bit for bit, in both precisions: the
positions of NaN, the positions AND signs of Inf, every other value.  The window search is pinnable through the f2py twin
only (tests/test_oracle_pin.py), so the second test carries the pin over to what the GPU tests actually call: the oracle's
host-model flavour, its ghost-celled form and its all-core point loop return, on the band cells, the f2py twin's bits.
"""
import numpy as np
import pytest

from oracle.pyoracle import Oracle, Reference, reference_available
from seabreeze_param_amd import synth

import guard_ref as gr
import radius_ref as rr

NX, NY, NZ = 96, 72, 3
NAN, INF, MISSING = gr.NAN, gr.INF, gr.MISSING


def _same(a, b, what):
    """bit for bit, NaN payloads aside: NaN in the same cells, everything else equal -- the sign of an Inf included"""
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN positions"
    assert np.array_equal(np.where(np.isnan(a), 0, a), np.where(np.isnan(b), 0, b)), what
    assert np.array_equal(np.signbit(a) & np.isinf(a), np.signbit(b) & np.isinf(b)), what + ": Inf signs"


def _fields(impl, maxdist=700.0):
    dt = impl.dt
    st = synth.static_fields(NX, NY, dt, fractional_coast=True)
    coast = impl.get_edges(st.landfrac, st.icefrac)
    return st, impl.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=maxdist)


def _cases(cd, maxdist):
    radius = rr.search_radius(cd, maxdist, 0, rr.BND_WRAPPER)
    isband = radius != 0
    cases = gr.directed(cd >= 0, isband, radius)
    cases.pop("d_nan_strip_block_corner")                # (a matter of the kernels' block grid)
    return cases, isband, radius


def _run_wrapper(impl, st, cd, spec, maxdist):
    dt = impl.dt
    p = synth.pressure_1d(NZ, dt)
    state = [np.zeros((NY, NX), dt) for _ in range(3)]
    res = {}
    for tn in (1, 2, 3):
        th = synth.theta_step(st, tn, dt)
        z = st.z
        if tn == 2:
            th, z = gr.poison(th, z, spec)
        u, v = synth.wind_step(st, NZ, tn, dt)
        out = impl.diag(tn, p, z, st.sigma, th, v, u, cd, *state, maxdist=maxdist, timestep=90.0)
        res[tn] = (out[:, :-1].copy(), [a.copy() for a in state])
    return res


@pytest.mark.parametrize("prec", [8, 4])
def test_oracle_follows_the_compiled_reference_on_bad_cells(prec):
    if not reference_available(prec):
        pytest.skip("oracle/_ref is not built here")
    orc, ref = Oracle(prec), Reference(prec)
    st, cd = _fields(orc)
    _same(cd, _fields(ref)[1], "cdist")
    cases, isband, _ = _cases(cd, 700.0)
    seen = set()
    for name, spec in cases.items():
        a, b = _run_wrapper(orc, st, cd, spec, 700.0), _run_wrapper(ref, st, cd, spec, 700.0)
        for tn in (1, 2, 3):
            _same(a[tn][0], b[tn][0], f"{name} step {tn} output")
            for nm, x, y in zip(("ws", "wd", "thc"), a[tn][1], b[tn][1]):
                _same(x, y, f"{name} step {tn} {nm}")
        thc, sb = a[2][1][2], a[2][0][0]
        seen |= {k for k, m in (("nan", np.isnan(thc)), ("+inf", np.isposinf(thc)), ("-inf", np.isneginf(thc)),
                                ("huge", np.isfinite(thc) & (np.abs(thc) > 1e15)), ("sb_nan", np.isnan(sb[isband[:-1]]))) if m.any()}
        assert np.isfinite(a[3][1][2][isband]).all(), name          # step 3: the bad cell is gone
    # the cases between them show every kind of answer: NaN, Inf of either sign (a bad centre gives +-Inf, not NaN), the
    # missing value's 2e20 / n, and the NaN sb_con of Inf / Inf
    assert seen == {"nan", "+inf", "-inf", "huge", "sb_nan"}, seen


@pytest.mark.parametrize("prec", [8, 4])
def test_host_model_forms_of_the_oracle_return_the_twins_bits(prec):
    """sbo_seabreeze_diag_x with the wrapper's rule (bnd 0), the same through ghost cells copied from the field under the
    global rule against the global rule itself (bnd 2 against bnd 1), and the all-core loop against the serial one."""
    orc, omp = Oracle(prec), Oracle(prec, omp=True)
    dt = orc.dt
    st, cd = _fields(orc, maxdist=600.0)
    cd[np.abs(cd) > 180.0] = 12000.0
    cases, isband, radius = _cases(cd, 180.0)
    assert isband.sum() > 300 and radius.max() >= 2
    p1 = synth.pressure_1d(NZ, dt)
    p3 = np.ascontiguousarray(np.broadcast_to(p1[:, None, None], (NZ, NY, NX)))
    th0 = synth.theta_step(st, 1, dt)
    u, v = synth.wind_step(st, NZ, 1, dt)
    h = int(radius.max())
    rows, cols = np.clip(np.arange(-h, NY + h), 0, NY - 1), np.arange(-h, NX + h) % NX
    frame = lambda a: np.ascontiguousarray(a[np.ix_(rows, cols)])
    for name, spec in cases.items():
        th, z = gr.poison(th0, st.z, spec)
        sw = [np.zeros((NY, NX), dt) for _ in range(3)]
        out = orc.diag(1, p1, z, st.sigma, th, v, u, cd, *sw, timestep=24.0)
        sg = [np.zeros((NY, NX), dt) for _ in range(4)]
        orc.seabreeze_diag(1440.0, 1, p3, u, v, th, cd, z, st.sigma, *sg, halo=0, bnd=0)
        _same(out[0][isband], sg[3][isband], name + " sb_con")
        _same(sw[2][isband], sg[2][isband], name + " thc")
        glob = [np.zeros((NY, NX), dt) for _ in range(4)]
        orc.seabreeze_diag(1440.0, 1, p3, u, v, th, cd, z, st.sigma, *glob, halo=0, bnd=1)
        par = [np.zeros((NY, NX), dt) for _ in range(4)]
        omp.seabreeze_diag(1440.0, 1, p3, u, v, th, cd, z, st.sigma, *par, halo=0, bnd=1, omp=True)
        sd, r = orc.sigmoid_scalars(st.sigma)
        halo = [np.zeros((NY, NX), dt) for _ in range(4)]
        orc.seabreeze_diag(1440.0, 1, p3, u, v, frame(th), frame(cd), frame(z), frame(st.sigma), *halo, halo=h, bnd=2,
                           ext_stats=(sd, r))
        for nm, a, b, c in zip(("ws", "wd", "thc", "sb_con"), glob, par, halo):
            _same(a, b, f"{name} {nm}: all-core against serial")
            _same(a, c, f"{name} {nm}: ghost cells against the global rule")
