"""`dummy_model ... um2d`: the UM copy's whole chain through the Fortran module -- get_edges_um, get_dist_um on 2-D
coordinates (the broadcast of the input's 1-D lon, lat) with a window of +-(halo + 3) cells, then seabreeze_diag_um
every step -- against the numpy restatement of the UM setup (tests/um_setup_ref.py) and the oracle's raw-index diag
with the UM level rule.  The UM file cannot be compiled: parity unpinned by nature, as for the `um` mode."""
import os
import subprocess

import numpy as np
import pytest

import um_setup_ref as ur
from conftest import ROOT, relerr
from seabreeze_param_amd import synth

EXE = {4: os.path.join(ROOT, "fortran", "build", "r4", "dummy_model"),
       8: os.path.join(ROOT, "fortran", "build", "r8", "dummy_model")}


def _write_input(path, prec, nx, ny, nz, halo, nsteps):
    """The input format of fortran/dummy_model.f90 (unchanged)."""
    dt = np.float64 if prec == 8 else np.float32
    st = _static(nx, ny, halo, dt)
    p = synth.pressure_3d(st, nz, dt)
    steps = []
    with open(path, "wb") as f:
        np.array([nx, ny, nz, halo], dtype=np.int32).tofile(f)
        for a in (st.lon, st.lat, st.landfrac, st.icefrac, st.z, st.sigma, p):
            np.ascontiguousarray(a, dtype=dt).tofile(f)
        for t in range(1, nsteps + 1):
            th = synth.theta_step(st, t, dt)
            u, v = synth.wind_step(st, nz, t, dt)
            for a in (th, u, v):
                a.tofile(f)
            steps.append((th, u, v))
    return st, p, steps


def _static(nx, ny, halo, dt):
    """bench.py's static fields with a binary land mask, no sea ice, and open sea within halo + 5 cells of the edge:
    then every coastal-band cell of the sub-domain finds land and sea within the small halo (so the oracle's raw-index
    reads stay inside its ghost frame; the test below checks it)."""
    st = synth.static_fields(nx, ny, dt)
    land = (st.landfrac >= 0.5).astype(dt)
    f = halo + 5
    land[:f] = 0; land[-f:] = 0; land[:, :f] = 0; land[:, -f:] = 0
    st.landfrac = np.ascontiguousarray(land)
    st.icefrac = np.zeros_like(land)
    return st


def _expected_cdist(st, nx, ny, hl):
    """The restatement of what um2d's setup makes: interior landfrac / icefrac of the sub-domain, their ring the edge
    cells (get_edges_um of the Fortran module), 2-D coordinates, ghost cells of the distance field the edge cells."""
    lf = np.ascontiguousarray(st.landfrac[hl:ny - hl, hl:nx - hl])
    ci = np.ascontiguousarray(st.icefrac[hl:ny - hl, hl:nx - hl])
    lat2, lon2 = (np.ascontiguousarray(a) for a in np.meshgrid(st.lat[hl:ny - hl], st.lon[hl:nx - hl], indexing="ij"))
    coast_l = ur.edges_um(ur.pad_edge(lf, hl, hl), ur.pad_edge(ci, hl, hl), hl, hl)
    cd = ur.dist_um_vectorised(coast_l, lf, lat2, lon2, hl, hl, 180.0)
    return ur.pad_edge(cd[hl:-hl, hl:-hl], hl, hl)


def _max_radius(m, hs):
    """The contrast window a coastal-band cell (|m| <= 180) needs to see both signs (None: more than hs)."""
    ny, nx = m.shape[0] - 2 * hs, m.shape[1] - 2 * hs
    worst = 0
    for j, i in zip(*np.nonzero(np.abs(m[hs:hs + ny, hs:hs + nx]) <= 180.0)):
        for r in range(1, hs + 1):
            w = m[hs + j - r:hs + j + r + 1, hs + i - r:hs + i + r + 1]
            if (w >= 0).any() and (w < 0).any():
                break
        else:
            return None
        worst = max(worst, r)
    return worst


def test_um2d_input_stays_within_the_small_halo():
    """CPU precondition of the GPU test below: every coastal-band cell of the sub-domain finds both signs within hs
    cells, so the oracle's raw-index reads stay inside its ghost frame."""
    nx, ny, halo = 96, 72, 2
    hs, hl = halo + 1, halo + 3
    st = _static(nx, ny, halo, np.float64)
    assert np.count_nonzero(st.landfrac) > 200
    cd = _expected_cdist(st, nx, ny, hl)
    r = _max_radius(np.ascontiguousarray(cd[hl - hs:cd.shape[0] - (hl - hs), hl - hs:cd.shape[1] - (hl - hs)]), hs)
    assert r is not None and r <= hs


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [8, 4])
def test_dummy_model_um2d_mode(tmp_path, oracles, prec):
    assert all(os.path.exists(p) for p in EXE.values())
    nx, ny, nz, halo, nsteps = 96, 72, 5, 2, 3
    hs, hl = halo + 1, halo + 3
    nxi, nyi = nx - 2 * hl, ny - 2 * hl
    dt = np.float64 if prec == 8 else np.float32
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    st, p, steps = _write_input(fin, prec, nx, ny, nz, halo, nsteps)
    r = subprocess.run([EXE[prec], str(fin), str(fout), str(nsteps), "um2d"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, dtype=dt)
    nl = (nxi + 2 * hl) * (nyi + 2 * hl)
    cd_h = raw[:nl].reshape(nyi + 2 * hl, nxi + 2 * hl)
    cd_o = _expected_cdist(st, nx, ny, hl)
    assert np.array_equal(cd_h >= 12000.0, cd_o >= 12000.0) and np.array_equal(np.sign(cd_h), np.sign(cd_o))
    e = np.abs(cd_h.astype(np.float64) - cd_o) / np.maximum(np.abs(cd_o.astype(np.float64)), 1.0)
    assert e.max() <= (1e-12 if prec == 8 else 2e-6)
    small = lambda a: np.ascontiguousarray(a[hl - hs:ny - hl + hs, hl - hs:nx - hl + hs])
    core = lambda a: np.ascontiguousarray(a[..., hl:ny - hl, hl:nx - hl])
    mask_s = np.ascontiguousarray(cd_o[hl - hs:cd_o.shape[0] - (hl - hs), hl - hs:cd_o.shape[1] - (hl - hs)])
    orc = oracles[prec]
    so = [np.zeros((nyi, nxi), dt) for _ in range(4)]
    per = nxi * nyi
    off = nl
    for t, (th, u, v) in enumerate(steps, start=1):
        orc.seabreeze_diag(1440.0, t, core(p), core(u), core(v), small(th), mask_s, small(st.z), small(st.sigma), *so,
                           halo=hs, bnd=2, level_rule=1)
        sb, ws, wd, thc = (raw[off + i * per: off + (i + 1) * per].reshape(nyi, nxi) for i in range(4))
        off += 4 * per
        if prec == 8:
            for a, b, nm in ((ws, so[0], "ws"), (wd, so[1], "wd"), (thc, so[2], "thc"), (sb, so[3], "sb_con")):
                assert relerr(a, b, floor=1e-2) < 1e-7, (t, nm)
        else:
            assert relerr(ws, so[0], floor=1e-3) < 2e-6 and np.max(np.abs(thc - so[2])) < 2e-3
    assert off == raw.size
