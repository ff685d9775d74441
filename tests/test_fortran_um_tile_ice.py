"""`dummy_model ... umtileice`: umtile's 2 x 2 cut of um2d's sub-domain under um2dice's ice planes, through the Fortran
module -- per tile um_tile_coast_open once, then per plane the copy of icefrac in the role of swap_bounds and um_tile_ice --
against the whole-domain get_edges_um + get_dist_um_win of the same run, plane by plane (0 differing cells: the tile kernel
shares the wide kernel's arithmetic), and against the numpy restatement (tests/um_setup_ref.py, the project's bounds for this
chain)."""
import os
import subprocess

import numpy as np
import pytest

import um_tile_ref as ut
import um_win_ref as uw
from test_fortran_um2d import EXE, _static, _write_input
from test_fortran_um_ice import _ice_of_step

NX, NY, NZ, HALO, NPLANES = 96, 72, 3, 2, 3
HL = HALO + 3


def _built():
    return all(os.path.exists(p) for p in EXE.values())


def _case(dt, step):
    st = _static(NX, NY, HALO, dt)
    lf = np.ascontiguousarray(st.landfrac[HL:NY - HL, HL:NX - HL])
    lat2, lon2 = (np.ascontiguousarray(a) for a in np.meshgrid(st.lat[HL:NY - HL], st.lon[HL:NX - HL], indexing="ij"))
    return dict(land=lf, lat=lat2, lon=lon2, coast=ut._coast(lf, _ice_of_step(lf, step)))


def _tiles(nxi, nyi):
    return ut.tiles(((0, nxi // 2, nxi), (0, nyi // 2, nyi)))


def test_umtileice_input_moves_coasts_across_the_seams():
    """CPU precondition: the coast differs from plane to plane inside every tile's source rectangle (so every ice call after
    a tile's first is counted), and on every plane the interior-only rule per tile differs from the whole-domain field while
    the model on the source rectangle meets it."""
    cases = [_case(np.float64, s) for s in range(1, NPLANES + 1)]
    nyi, nxi = cases[0]["land"].shape
    for g in cases:
        whole = ut.whole_dist(g["coast"], g["land"], g["lat"], g["lon"], HL, HL, 180.0)
        missed = 0
        for t in _tiles(nxi, nyi):
            x0, x1, y0, y1 = t
            assert np.array_equal(ut.tile_dist(g["coast"], g["land"], g["lat"], g["lon"], t, HL, HL, 180.0), whole[y0:y1, x0:x1])
            own = ut.tile_dist(g["coast"], g["land"], g["lat"], g["lon"], t, HL, HL, 180.0, reach=(0, 0))
            missed += np.count_nonzero(own != whole[y0:y1, x0:x1])
        assert missed > 0
    for a, b in zip(cases, cases[1:]):
        for t in _tiles(nxi, nyi):
            ex0, ex1, ey0, ey1 = ut.extended(t, nxi, nyi, HL, HL)
            assert not np.array_equal(a["coast"][ey0:ey1, ex0:ex1], b["coast"][ey0:ey1, ex0:ex1]), t


@pytest.mark.gpu
@pytest.mark.skipif(not _built(), reason="fortran/build not made (run __graft_entry__.build())")
@pytest.mark.parametrize("prec", [8, 4])
def test_dummy_model_umtileice_mode(tmp_path, prec):
    dt = np.float64 if prec == 8 else np.float32
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    _write_input(fin, prec, NX, NY, NZ, HALO, 0)
    r = subprocess.run([EXE[prec], str(fin), str(fout), str(NPLANES), "umtileice"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split("umtileice: differing cells")[1].split()
    assert int(words[0]) == 0 and float(words[3]) == 0.0, r.stdout
    nxi, nyi = NX - 2 * HL, NY - 2 * HL
    tiles = _tiles(nxi, nyi)
    # summed over the tiles: calls, calls after the first whose coast differed, tiles marked by the last call, tiles
    rep = [int(v) for v in r.stdout.split("umtileice: ice report")[1].split()[:4]]
    ntiles = sum(-(-(t[3] - t[2]) // 4) * -(-(t[1] - t[0]) // 64) for t in tiles)
    assert rep[0] == 4 * NPLANES and rep[1] == 4 * (NPLANES - 1) and 4 <= rep[2] <= rep[3] == ntiles, rep
    raw = np.fromfile(fout, dtype=dt)
    assert raw.size == 2 * NPLANES * nxi * nyi
    fields = raw.reshape(NPLANES, 2, nyi, nxi)
    refs = []
    for s in range(NPLANES):
        whole, tiled = fields[s]
        assert np.array_equal(whole, tiled), s + 1
        g = _case(dt, s + 1)
        ref = ut.whole_dist(g["coast"], g["land"], g["lat"], g["lon"], HL, HL, 180.0)
        uw.check_dist(tiled, ref, f"umtileice plane {s + 1}", 1e-12 if prec == 8 else 2e-6)
        assert (np.abs(ref) < 12000.0).any()
        refs.append(ref)
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
