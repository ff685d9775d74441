"""`dummy_model ... um2dice`: um2d's sub-domain with sea ice that differs from step to step, through the Fortran module --
um_coast_open once, um_ice ahead of every seabreeze_diag_um -- against the numpy chain (tests/um_setup_ref.py) stepped with
the same ice frames and the oracle's raw-index diag with the UM level rule.  Step s ices (0.6) the sea cells of the
sub-domain that touch land and whose row j (1-based) has mod(j + s, 3) == 0: the coast moves out by a cell there, and every
coastal-band cell still finds land within the small halo.  Bounds: the project's for this chain (tests/test_fortran_um2d.py).
"""
import os
import subprocess

import numpy as np
import pytest

import um_setup_ref as ur
from conftest import relerr
from test_fortran_um2d import EXE, _max_radius, _static, _write_input

NX, NY, NZ, HALO, NSTEPS = 96, 72, 5, 2, 3
HS, HL = HALO + 1, HALO + 3


def _built():
    return all(os.path.exists(p) for p in EXE.values())


def _ice_of_step(lf, step):
    """the sub-domain's icefrac of step `step` (1-based), as fortran/dummy_model.f90 (run_um2dice) makes it"""
    nyi, nxi = lf.shape
    land = np.pad(lf > 0, 1)
    near = np.zeros((nyi, nxi), bool)
    for dj in (0, 1, 2):
        for di in (0, 1, 2):
            near |= land[dj:dj + nyi, di:di + nxi]
    shore = (lf == 0) & near
    rows = ((np.arange(1, nyi + 1) + step) % 3 == 0)[:, None]
    return np.where(shore & rows, lf.dtype.type(0.6), lf.dtype.type(0.0)).astype(lf.dtype)


def _expected_cdist(st, step):
    lf = np.ascontiguousarray(st.landfrac[HL:NY - HL, HL:NX - HL])
    ci = _ice_of_step(lf, step)
    lat2, lon2 = (np.ascontiguousarray(a) for a in np.meshgrid(st.lat[HL:NY - HL], st.lon[HL:NX - HL], indexing="ij"))
    coast_l = ur.edges_um(ur.pad_edge(lf, HL, HL), ur.pad_edge(ci, HL, HL), HL, HL)
    cd = ur.dist_um_vectorised(coast_l, lf, lat2, lon2, HL, HL, 180.0)
    return ur.pad_edge(cd[HL:-HL, HL:-HL], HL, HL), coast_l


def test_um2dice_input_moves_the_coast_within_the_small_halo():
    """CPU preconditions of the GPU test below: the ice frames differ from step to step and so do the coasts, and every
    coastal-band cell of every step finds both signs within hs cells (the oracle's raw-index reads stay inside its frame)."""
    st = _static(NX, NY, HALO, np.float64)
    coasts = []
    for step in range(1, NSTEPS + 1):
        cd, coast_l = _expected_cdist(st, step)
        coasts.append(coast_l)
        r = _max_radius(np.ascontiguousarray(cd[HL - HS:cd.shape[0] - (HL - HS), HL - HS:cd.shape[1] - (HL - HS)]), HS)
        assert r is not None and r <= HS, step
    lf = st.landfrac[HL:NY - HL, HL:NX - HL]
    assert all(_ice_of_step(lf, s).any() for s in (1, 2, 3))
    assert not np.array_equal(coasts[0], coasts[1]) and not np.array_equal(coasts[1], coasts[2])


@pytest.mark.gpu
@pytest.mark.skipif(not _built(), reason="fortran/build not made (run __graft_entry__.build())")
@pytest.mark.parametrize("prec", [8, 4])
def test_dummy_model_um2dice_mode(tmp_path, oracles, prec):
    nxi, nyi = NX - 2 * HL, NY - 2 * HL
    dt = np.float64 if prec == 8 else np.float32
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    st, p, steps = _write_input(fin, prec, NX, NY, NZ, HALO, NSTEPS)
    r = subprocess.run([EXE[prec], str(fin), str(fout), str(NSTEPS), "um2dice"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # calls, calls after the first whose coast differed, tiles marked by the last call, tiles
    rep = [int(v) for v in r.stdout.split("um2dice: ice report")[1].split()[:4]]
    assert rep[0] == NSTEPS and rep[1] == NSTEPS - 1 and 0 < rep[2] <= rep[3] == -(-nyi // 4) * -(-nxi // 64), rep
    raw = np.fromfile(fout, dtype=dt)
    nl = (nxi + 2 * HL) * (nyi + 2 * HL)
    small = lambda a: np.ascontiguousarray(a[HL - HS:NY - HL + HS, HL - HS:NX - HL + HS])
    core = lambda a: np.ascontiguousarray(a[..., HL:NY - HL, HL:NX - HL])
    orc = oracles[prec]
    so = [np.zeros((nyi, nxi), dt) for _ in range(4)]
    per = nxi * nyi
    off = 0
    for t, (th, u, v) in enumerate(steps, start=1):
        cd_h = raw[off:off + nl].reshape(nyi + 2 * HL, nxi + 2 * HL)
        off += nl
        cd_o, _ = _expected_cdist(st, t)
        assert np.array_equal(cd_h >= 12000.0, cd_o >= 12000.0) and np.array_equal(np.sign(cd_h), np.sign(cd_o)), t
        e = np.abs(cd_h.astype(np.float64) - cd_o) / np.maximum(np.abs(cd_o.astype(np.float64)), 1.0)
        assert e.max() <= (1e-12 if prec == 8 else 2e-6), (t, e.max())
        mask_s = np.ascontiguousarray(cd_o[HL - HS:cd_o.shape[0] - (HL - HS), HL - HS:cd_o.shape[1] - (HL - HS)])
        orc.seabreeze_diag(1440.0, t, core(p), core(u), core(v), small(th), mask_s, small(st.z), small(st.sigma), *so,
                           halo=HS, bnd=2, level_rule=1)
        sb, ws, wd, thc = (raw[off + i * per: off + (i + 1) * per].reshape(nyi, nxi) for i in range(4))
        off += 4 * per
        if prec == 8:
            for a, b, nm in ((ws, so[0], "ws"), (wd, so[1], "wd"), (thc, so[2], "thc"), (sb, so[3], "sb_con")):
                assert relerr(a, b, floor=1e-2) < 1e-7, (t, nm)
        else:
            assert relerr(ws, so[0], floor=1e-3) < 2e-6 and np.max(np.abs(thc - so[2])) < 2e-3
    assert off == raw.size
