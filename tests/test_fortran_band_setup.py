"""fortran/dummy_model.f90 in mode `bandsetup`: the Fortran surface of the band-local coast setup (band_get_edges,
band_get_dist of fortran/sea_breeze_diag_mod.F90).  The program computes coast and distance of a 96x72 grid with the
whole-grid routines, then of three bands in ghost-celled frames it cuts itself, and stops with an error at the first cell
whose bits differ; the whole-grid field it writes is checked against the CPU oracle here, so that "equal" is not two
wrong fields."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, relerr
from seabreeze_param_amd import synth

pytestmark = pytest.mark.gpu

EXE = {4: os.path.join(ROOT, "fortran", "build", "r4", "dummy_model"),
       8: os.path.join(ROOT, "fortran", "build", "r8", "dummy_model")}


@pytest.mark.parametrize("prec", [8, 4])
def test_dummy_model_bandsetup(tmp_path, oracles, prec):
    assert os.path.exists(EXE[prec]), "fortran/build missing: __graft_entry__.build() makes it"
    nx, ny, nz, halo = 96, 72, 1, 4
    dt = np.float64 if prec == 8 else np.float32
    st = synth.static_fields(nx, ny, dt)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([nx, ny, nz, halo], dtype=np.int32).tofile(f)
        for a in (st.lon, st.lat, st.landfrac, st.icefrac, st.z, st.sigma, synth.pressure_3d(st, nz, dt)):
            np.ascontiguousarray(a, dtype=dt).tofile(f)
    r = subprocess.run([EXE[prec], str(fin), str(fout), "0", "bandsetup"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bandsetup ok" in r.stdout, r.stdout + r.stderr
    orc = oracles[prec]
    coast = orc.get_edges(st.landfrac, st.icefrac, rule=1, bnd=1)
    cdist = orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=180.0, kwin=halo)
    # the cuts of the program (rows 23 and 50) are tested: coast cells lie within the window of each, on both sides
    for c in (ny // 3 - 1, 2 * (ny // 3) + 2):
        assert coast[c - halo:c].any() and coast[c:c + halo].any()
    out = np.fromfile(fout, dtype=dt).reshape(ny, nx)
    assert relerr(out, cdist, floor=1e-2) < (1e-7 if prec == 8 else 2e-6)
