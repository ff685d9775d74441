"""fortran/dummy_model.f90 in mode `radius`: the Fortran surface of search_radius and band_search_radius
(fortran/sea_breeze_diag_mod.F90).  The program forms the window radii of a 96x72 grid with the whole-grid routine, then of
three bands in ghost-celled frames it cuts itself, and stops with an error at the first band cell that is neither the
grid's radius (where that is within reach of the band's ghost rows) nor -1 (where it is not); the whole-grid plane it writes
is checked against the numpy model on the CPU oracle's distance field here, so that "consistent" is not two wrong planes."""
import os
import subprocess

import numpy as np
import pytest

import radius_ref as rr
from conftest import ROOT
from seabreeze_param_amd import synth

pytestmark = pytest.mark.gpu

EXE = {4: os.path.join(ROOT, "fortran", "build", "r4", "dummy_model"),
       8: os.path.join(ROOT, "fortran", "build", "r8", "dummy_model")}


@pytest.mark.parametrize("prec", [8, 4])
def test_dummy_model_radius(tmp_path, oracles, prec):
    assert os.path.exists(EXE[prec]), "fortran/build missing: __graft_entry__.build() makes it"
    nx, ny, nz, halo = 96, 72, 1, 2
    dt = np.float64 if prec == 8 else np.float32
    st = synth.static_fields(nx, ny, dt)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([nx, ny, nz, halo], dtype=np.int32).tofile(f)
        for a in (st.lon, st.lat, st.landfrac, st.icefrac, st.z, st.sigma, synth.pressure_3d(st, nz, dt)):
            np.ascontiguousarray(a, dtype=dt).tofile(f)
    r = subprocess.run([EXE[prec], str(fin), str(fout), "0", "radius"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "radius ok" in r.stdout, r.stdout + r.stderr
    orc = oracles[prec]
    coast = orc.get_edges(st.landfrac, st.icefrac, rule=1, bnd=1)
    cdist = orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=180.0, kwin=halo)
    want = rr.search_radius(cdist, 180.0, 0, rr.BND_GLOBAL)
    assert rr.summary_of(want)[3] > halo             # some windows are wider than the bands' ghost frame
    raw = np.fromfile(fout, dtype=np.uint8)
    nb = nx * ny * np.dtype(dt).itemsize
    assert raw.size == nb + nx * ny * 4
    got = raw[nb:].view(np.int32).reshape(ny, nx)
    assert np.array_equal(got, want)
