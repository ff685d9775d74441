"""The table contrast through the Python surface: seabreezediag.diag(..., table_contrast=True[, keep_windows=True]) over the
f2py extension's set_table_contrast (python_wrapper/seabreeze_f2py.f90; sb_set_table_contrast with
sb_set_table_contrast_f2py, include/seabreeze_hip.h).  Skipped where the extension is not built, as
tests/test_python_surface.py is.

Six steps on the block grid of tests/test_table_contrast_gpu.py (160 x 112, radii up to 40, every cell in the band).  The
driver derives its distance field from the land mask; here it is handed the block grid's signed field instead
(seabreezediag._coast_distance is replaced for the test), so that the windows are those tests/test_table_f2py_gpu.py holds
to tests/radius_ref.py.

The driver returns the state of the last step only, and never this flavour's thc (what it hands back under that name is the
t0 plane, ref: python_wrapper/seabreezediag/__init__.py:244).  The single-precision criterion (oracle/fp32_criterion.py)
needs every step's winds and contrast, so it is applied to the same six steps through sb_diag_f32 on a context of the
test's own with the same switches -- the same kernels on the same inputs -- and the driver's sb_con planes and final state
are required to equal that run's bit for bit.  timestep = target_time: every step stores its winds (ref:
seabreeze_diag_python.f90:268-273), so the carried state shows the mean wind speed the criterion derives from it.
"""
import os
import sys

import numpy as np
import pytest

import table_ref as tr
from conftest import ROOT
from oracle import fp32_criterion as crit
from seabreeze_param_amd import synth

PW = os.path.join(ROOT, "python_wrapper")
NX, NY, W = tr.BLOCK
NT, NZ = 6, 3
KW = dict(timestep=360.0, target_time=6.0)
f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


def _built():
    return any(f.startswith("seabreeze.") and f.endswith(".so") for f in os.listdir(PW))


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _built(), reason="python_wrapper extension not built")]


def _import_surface():
    if PW not in sys.path:
        sys.path.insert(0, PW)
    import seabreeze
    import seabreezediag
    assert os.path.dirname(seabreeze.__file__) == PW, seabreeze.__file__
    return seabreeze, seabreezediag


@pytest.fixture(scope="module")
def case():
    dt = np.float32
    st = synth.static_fields(NX, NY, dt)
    pres = synth.pressure_1d(NZ, dt)
    t = np.stack([synth.theta_step(st, k + 1, dt) for k in range(NT)])
    uv = [synth.wind_step(st, NZ, k + 1, dt) for k in range(NT)]
    u = np.stack([a for a, _ in uv]); v = np.stack([b for _, b in uv])
    mask = tr.mask_of(tr.block_land(NX, NY, W, NX), dt)
    return st, pres, u, v, t, mask


@pytest.fixture
def sbd(monkeypatch, case):
    ext, mod = _import_surface()
    assert mod._HAVE_STREAM and hasattr(ext, "set_table_contrast")
    mask = case[5]
    monkeypatch.setattr(mod, "_coast_distance", lambda *a, **k: mask)
    monkeypatch.delenv("SEABREEZE_NO_STREAM", raising=False)
    return ext, mod


def _drive(mod, case, **kw):
    st, pres, u, v, t, _ = case
    return mod.diag(1, st.landfrac, st.z, st.sigma, st.lon, st.lat, pres, u, v, t, None, **KW, **kw)


def _same(a, b, what):
    """(the last latitude row of every plane is never written)"""
    assert a[0] == b[0] == 1 + NT
    assert np.array_equal(a[1][:, :-1].view(np.int64), b[1][:, :-1].view(np.int64)), f"{what}: sb_con"
    for k, nm in ((2, "t0"), (3, "ws"), (4, "wd")):
        assert np.array_equal(np.asarray(a[k])[:-1].view(np.int32), np.asarray(b[k])[:-1].view(np.int32)), f"{what}: {nm}"


def test_streamed_stepwise_and_kept_windows_agree_and_the_switches_are_reset(sbd, case, monkeypatch):
    ext, mod = sbd
    plain = _drive(mod, case)
    assert ext.last_launches() == 5
    streamed = _drive(mod, case, table_contrast=True)
    assert ext.last_launches() == 6
    kept = _drive(mod, case, table_contrast=True, keep_windows=True)
    assert ext.last_launches() == 6
    monkeypatch.setenv("SEABREEZE_NO_STREAM", "1")
    stepwise = _drive(mod, case, table_contrast=True)
    assert ext.last_launches() == 6
    stepwise_plain = _drive(mod, case)                       # after the call returned: the flavour's five launches again
    assert ext.last_launches() == 5
    monkeypatch.delenv("SEABREEZE_NO_STREAM")
    after = _drive(mod, case)
    assert ext.last_launches() == 5
    _same(streamed, stepwise, "streamed against step by step")
    _same(kept, streamed, "keep_windows")
    _same(after, plain, "plain call after the table calls")
    _same(stepwise_plain, plain, "plain step-by-step call after the table calls")
    # keep_windows without table_contrast is no table call
    alone = _drive(mod, case, keep_windows=True)
    assert ext.last_launches() == 5
    _same(alone, plain, "keep_windows alone")


def test_against_the_oracle_under_the_fp32_criterion(sbd, case, oracles):
    from seabreeze_param_amd import hip
    ext, mod = sbd
    st, pres, u, v, t, mask = case
    streamed = _drive(mod, case, table_contrast=True)
    ctx = hip.Context()
    try:
        ctx.set_table_contrast(True)
        ctx.set_table_contrast_f2py(True)
        gs = tr.zeros(3, np.float32, NY, NX)
        os_ = tr.zeros(3, np.float64, NY, NX)
        gp, op = tr.zeros(4, np.float32, NY, NX), tr.zeros(4, np.float64, NY, NX)
        band = np.ones((NY, NX), bool)
        band[NY - 1] = False                                 # the row the flavour does not process
        res = []
        for k in range(NT):
            out = ctx.diag(k + 1, pres, st.z, st.sigma, t[k], v[k], u[k], mask, *gs, **KW)
            assert ctx.last_step_report()["kernel_launches"] == 6
            c = ctx.last_counters()
            oo = oracles[8].diag(k + 1, f8(pres), f8(st.z), f8(st.sigma), f8(t[k]), f8(v[k]), f8(u[k]), f8(mask), *os_, **KW)
            assert c["global_path_cells"] == 0 and c["max_radius"] == oracles[8].last_nn_max == 40, c
            gn, on = [a.copy() for a in gs] + [out[0].copy()], [a.copy() for a in os_] + [oo[0].copy()]
            res.append(crit.check_step(k + 1, gp, gn, op, on, band, timestep=KW["timestep"] * 60.0))
            gp, op = gn, on
            # the driver's plane of this step: the same kernels on the same inputs
            assert np.array_equal(streamed[1][k, :-1], out[0][:-1].astype(np.float64)), k
        merged = crit.merge(res)
        assert merged["ok"] and merged["cells_compared"] > 0, merged
        for a, b, nm in ((streamed[2], out[1], "t0"), (streamed[3], out[2], "ws"), (streamed[4], out[3], "wd")):
            assert np.array_equal(np.asarray(a)[:-1], b[:-1]), nm
    finally:
        ctx.close()
