"""`dummy_model ... umtile`: um2d's sub-domain cut into 2 x 2 tiles through the Fortran module -- every tile's frames copied
out of the whole fields in the role of swap_bounds, tile_get_edges_um and tile_get_dist_um per tile, reassembled -- against
the whole-domain get_edges_um + get_dist_um_win of the same run (0 differing cells: the tile kernel shares the wide
kernel's arithmetic) and against the numpy restatement (tests/um_setup_ref.py, the project's bounds for this chain)."""
import os
import subprocess

import numpy as np
import pytest

import um_tile_ref as ut
import um_win_ref as uw
from test_fortran_um2d import EXE, _static, _write_input

NX, NY, NZ, HALO = 96, 72, 3, 2
HL = HALO + 3


def _built():
    return all(os.path.exists(p) for p in EXE.values())


def _case(dt):
    st = _static(NX, NY, HALO, dt)
    lf = np.ascontiguousarray(st.landfrac[HL:NY - HL, HL:NX - HL])
    lat2, lon2 = (np.ascontiguousarray(a) for a in np.meshgrid(st.lat[HL:NY - HL], st.lon[HL:NX - HL], indexing="ij"))
    coast = ut._coast(lf, np.zeros_like(lf))
    return dict(land=lf, lat=lat2, lon=lon2, coast=coast)


def test_umtile_input_has_coasts_across_the_seams():
    """CPU precondition: on this input the interior-only rule per tile differs from the whole-domain field, so 0 differing
    cells is not met by a tile call that misses its ghost sources; the model on the extended rectangle meets it."""
    g = _case(np.float64)
    nyi, nxi = g["land"].shape
    whole = ut.whole_dist(g["coast"], g["land"], g["lat"], g["lon"], HL, HL, 180.0)
    missed = 0
    for t in ut.tiles(((0, nxi // 2, nxi), (0, nyi // 2, nyi))):
        x0, x1, y0, y1 = t
        got = ut.tile_dist(g["coast"], g["land"], g["lat"], g["lon"], t, HL, HL, 180.0)
        assert np.array_equal(got, whole[y0:y1, x0:x1])
        own = ut.tile_dist(g["coast"], g["land"], g["lat"], g["lon"], t, HL, HL, 180.0, reach=(0, 0))
        missed += np.count_nonzero(own != whole[y0:y1, x0:x1])
    assert missed > 0


@pytest.mark.gpu
@pytest.mark.skipif(not _built(), reason="fortran/build not made (run __graft_entry__.build())")
@pytest.mark.parametrize("prec", [8, 4])
def test_dummy_model_umtile_mode(tmp_path, prec):
    dt = np.float64 if prec == 8 else np.float32
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    _write_input(fin, prec, NX, NY, NZ, HALO, 0)
    r = subprocess.run([EXE[prec], str(fin), str(fout), "0", "umtile"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split("umtile: differing cells")[1].split()
    assert int(words[0]) == 0 and float(words[3]) == 0.0, r.stdout
    nxi, nyi = NX - 2 * HL, NY - 2 * HL
    raw = np.fromfile(fout, dtype=dt)
    assert raw.size == 2 * nxi * nyi
    whole, tiled = raw[:nxi * nyi].reshape(nyi, nxi), raw[nxi * nyi:].reshape(nyi, nxi)
    assert np.array_equal(whole, tiled)
    g = _case(dt)
    ref = ut.whole_dist(g["coast"], g["land"], g["lat"], g["lon"], HL, HL, 180.0)
    uw.check_dist(tiled, ref, "umtile", 1e-12 if prec == 8 else 2e-6)
    assert (np.abs(ref) < 12000.0).any()
