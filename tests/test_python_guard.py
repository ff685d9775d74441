"""The guard for missing and non-finite temperatures through the Python surface: seabreezediag.diag(..., guard_nonfinite=True)
over the f2py extension's set_nonfinite_guard (python_wrapper/seabreeze_f2py.f90; sb_set_nonfinite_guard,
include/seabreeze_hip.h), and the `guard_nonfinite` entry of a run configuration.

The host part runs without a GPU, as tests/test_python_table_host.py does.  On the GPU, three steps on the 160 x 96 coast
grid of tests/test_nonfinite_guard_gpu.py with a NaN and several +Inf in the temperature of step 2: the driver returns every
step's sb_con, whose NaN cells (Inf / Inf under the trigger rule, ref: generic/sea_breeze_diag.f90:255) must be the
oracle's -- streamed and step by step -- and are not without the keyword.
"""
import os
import sys

import numpy as np
import pytest

import guard_ref as gr
import radius_ref as rr
from conftest import ROOT, gpu_visible
from seabreeze_param_amd import synth

PW = os.path.join(ROOT, "python_wrapper")
NT, NZ = 3, 3
KW = dict(timestep=360.0, target_time=6.0)


def _built():
    return any(f.startswith("seabreeze.") and f.endswith(".so") for f in os.listdir(PW))


def _import_surface():
    if PW not in sys.path:
        sys.path.insert(0, PW)
    import seabreeze
    import seabreezediag
    assert os.path.dirname(seabreeze.__file__) == PW, seabreeze.__file__
    return seabreeze, seabreezediag


def test_run_configuration_entry(tmp_path):
    """run.conf.example shows the entry commented out; uncommented it reads as a boolean, absent it is off; the file driver
    hands it to diag under its own name"""
    import importlib.util
    import types
    text = open(os.path.join(PW, "run.conf.example")).read()
    assert "# guard_nonfinite = true" in text
    pkg = types.ModuleType("sb_cfg_pkg_guard")
    pkg.__path__ = [os.path.join(PW, "seabreezediag")]
    sys.modules["sb_cfg_pkg_guard"] = pkg
    try:
        spec = importlib.util.spec_from_file_location("sb_cfg_pkg_guard.configdir", os.path.join(PW, "seabreezediag", "configdir.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["sb_cfg_pkg_guard.configdir"] = mod
        spec.loader.exec_module(mod)
        off = tmp_path / "off.conf"
        off.write_text(text)
        assert mod.Config(str(off)).get("guard_nonfinite", False) is False
        on = tmp_path / "on.conf"
        on.write_text(text.replace("# guard_nonfinite = true", "guard_nonfinite = true"))
        cfg = mod.Config(str(on))
        assert cfg.guard_nonfinite is True and cfg.get("table_contrast", False) is False
    finally:
        for k in [k for k in sys.modules if k.startswith("sb_cfg_pkg_guard")]:
            del sys.modules[k]
    driver = open(os.path.join(PW, "run_seabreeze.py")).read()
    assert '"guard_nonfinite"' in driver and "**table" in driver


@pytest.mark.skipif(not _built(), reason="python_wrapper extension not built")
def test_extension_routine_and_keyword():
    seabreeze, sbd = _import_surface()
    assert seabreeze.set_nonfinite_guard.__doc__.splitlines()[0].strip() == "set_nonfinite_guard(on)"
    if gpu_visible():
        return                      # (the rest is test_diag_with_the_keyword_follows_the_oracle)
    # without a GPU the keyword reaches the extension, whose sb_create fails: the Python layer raises, before any step
    z = np.zeros((6, 8), np.float32)
    with pytest.raises(RuntimeError, match="set_nonfinite_guard"):
        sbd.diag(1, z, z, z, np.arange(8.0), np.arange(6.0), np.array([700.0]), z[None, None], z[None, None], z[None], None,
                 guard_nonfinite=True)


@pytest.mark.gpu
@pytest.mark.skipif(not _built(), reason="python_wrapper extension not built")
def test_diag_with_the_keyword_follows_the_oracle(monkeypatch, oracles):
    ext, mod = _import_surface()
    assert hasattr(ext, "set_nonfinite_guard")
    dt, orc = np.float32, oracles[4]
    st, cd = gr.global_field(orc, dt)
    cd = cd.astype(dt)
    nx, ny = gr.GRID
    radius = rr.search_radius(cd, 180.0, 0, rr.BND_WRAPPER)
    isband = radius != 0
    _, sea = gr.coast_cells(cd >= 0, isband)
    land, _ = gr.coast_cells(cd >= 0, isband)
    pres = synth.pressure_1d(NZ, dt)
    t = np.stack([synth.theta_step(st, k + 1, dt) for k in range(NT)])
    uv = [synth.wind_step(st, NZ, k + 1, dt) for k in range(NT)]
    u = np.stack([a for a, _ in uv]); v = np.stack([b for _, b in uv])
    t[1][land[len(land) // 2]] = np.nan
    for y, x in sea[::max(1, len(sea) // 12)]:
        t[1][y, x] = np.inf
    monkeypatch.setattr(mod, "_coast_distance", lambda *a, **k: cd)
    # the oracle, step by step
    state = [np.zeros((ny, nx), dt) for _ in range(3)]
    want = np.stack([orc.diag(k + 1, pres, st.z, st.sigma, t[k], v[k], u[k], cd, *state, **KW)[0].copy() for k in range(NT)])
    assert np.isnan(want[1][:-1]).any() and not np.isnan(want[0][:-1]).any() and not np.isnan(want[2][:-1]).any()

    def drive(**kw):
        return mod.diag(1, st.landfrac, st.z, st.sigma, st.lon, st.lat, pres, u, v, t, None, **KW, **kw)

    def pattern(sb):
        return np.isnan(sb[:, :-1]), np.isposinf(sb[:, :-1]), np.isneginf(sb[:, :-1])

    monkeypatch.delenv("SEABREEZE_NO_STREAM", raising=False)
    streamed = drive(guard_nonfinite=True)
    assert ext.last_launches() == 5 + 4
    monkeypatch.setenv("SEABREEZE_NO_STREAM", "1")
    stepwise = drive(guard_nonfinite=True)
    assert ext.last_launches() == 5 + 4
    plain = drive()
    assert ext.last_launches() == 5                          # the switch was taken back when the call returned
    for got, what in ((streamed, "streamed"), (stepwise, "step by step")):
        for a, b in zip(pattern(got[1]), pattern(want)):
            assert np.array_equal(a, b), what
    assert np.array_equal(streamed[1][:, :-1].view(np.int64), stepwise[1][:, :-1].view(np.int64))
    assert not all(np.array_equal(a, b) for a, b in zip(pattern(plain[1]), pattern(want)))
    # with the tables beside it
    both = drive(guard_nonfinite=True, table_contrast=True)
    assert ext.last_launches() == 6 + 4
    for a, b in zip(pattern(both[1]), pattern(want)):
        assert np.array_equal(a, b), "tables"
