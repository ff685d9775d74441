"""The directed ice planes of the UM layout's moving coast (tests/um_ice_cases.py) do what their names say -- shown on the
numpy restatement alone (tests/um_setup_ref.edges_um, tests/um_ice_ref.py), on the CPU, for the grid sizes, halos and windows
tests/test_um_ice_gpu.py uses.  Nothing here runs the code under test.
"""
import numpy as np
import pytest

import um_ice_cases as uic
import um_ice_ref as uir
import um_setup_ref as ur

IDS = [s[0] for s in uic.SETS]


def coasts(lf_l, planes, halo, nx, ny):
    hi, hj = halo
    return [ur.edges_um(lf_l, ci, hi, hj)[hj:hj + ny, hi:hi + nx] for ci in planes]


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("cset", uic.SETS, ids=IDS)
def test_planes_do_what_they_say(cset, dt):
    name, nx, ny, win, halo, maxdist, kern = cset
    assert uic.kernel_of(win, halo) == kern
    hi, hj = halo
    land, lf_l, planes = uic.make(nx, ny, halo, dt)
    assert len(planes) == len(uic.PLANES) == 12 and all(p.dtype == dt and p.shape == lf_l.shape for p in planes)
    co = coasts(lf_l, planes, halo, nx, ny)
    flags = [ur.land_um(lf_l, ci) for ci in planes]
    lay = uic.layout(nx, ny)
    inner = lambda f: f[hj:hj + ny, hi:hi + nx]
    empty = np.zeros_like(co[0])
    # every case except 2, 3 and 7 changes at least one word; 2, 3 and 7 change none
    for n in range(12):
        words = uir.words_of(uir.changed_cells(co[n], co[n - 1] if n else empty))
        if n in uic.UNCHANGED:
            assert not words, uic.PLANES[n]
        else:
            assert words, uic.PLANES[n]
    # 1: no ice, and a coast
    assert not planes[0].any() and co[0].any()
    # 2: the same plane
    assert np.array_equal(planes[1], planes[0])
    # 3: values move, no class flips -- 0.10 over open sea and 0.3 over landfrac 0.1; 0.10 -> 0.15 in the planes behind it
    assert not np.array_equal(planes[2], planes[1]) and np.array_equal(flags[2], flags[1])
    assert inner(planes[2])[lay["patch"]].min() == dt(0.10) and inner(planes[3])[lay["patch"]].min() == dt(0.15)
    assert inner(planes[2])[lay["lf01"]] == dt(0.3) and land[lay["lf01"]] == dt(0.1)
    # 4: one sea cell next to the coast, mid-grid
    d = inner(flags[3]) != inner(flags[2])
    assert d.sum() == 1 and d[lay["mid"]] and co[2][lay["mid"]] > 0, "not a coast cell's sea side"
    assert np.array_equal(flags[3] != flags[2], np.pad(d, ((hj, hj), (hi, hi))))
    # 5: interior cells (0, 0) and (nx-1, ny-1)
    d = inner(flags[4]) != inner(flags[3])
    assert d.sum() == 2 and d[0, 0] and d[ny - 1, nx - 1]
    # 6: the ghost ring only, column -1; the Sobel of interior column 0 changes
    d = flags[5] != flags[4]
    assert d.sum() == 1 and d[lay["ring_row"] + hj, hi - 1] and not inner(d).any()
    ch = uir.changed_cells(co[5], co[4])
    assert ch and all(x == 0 for x, _ in ch)
    # 7: two cells out -- where the frame has such a cell -- changes nothing
    d = flags[6] != flags[5]
    assert d.sum() == (1 if max(halo) >= 2 else 0) and not d[hj - 1:hj + ny + 1, hi - 1:hi + nx + 1].any()
    # 8: a block of ice in open sea; where the window allows it, farther than the window from any land, so that targets
    # whose windows held no coast get one
    r0, r1, b0, b1 = lay["block"]
    d = inner(flags[7]) != inner(flags[6])
    assert d[r0:r1, b0:b1].all() and d.sum() == (r1 - r0) * (b1 - b0)
    if name in ("a", "b", "f"):
        far = np.ones((ny, nx), bool)
        far[max(r0 - win[1] - 1, 0):r1 + win[1] + 1, max(b0 - win[0] - 1, 0):b1 + win[0] + 1] = False
        assert not (inner(flags[6]) & ~far).any(), "land within the window of the block"
        lo = uir.brute_marks(nx, ny, *win, uir.changed_cells(co[6], empty))
        new = uir.brute_marks(nx, ny, *win, uir.changed_cells(co[7], co[6]))
        assert (new & ~lo).any(), "no workgroup without a coast in reach gets one"
    # 9: the block's edge moved by one row across word boundaries
    e0, e1 = lay["edge_cols"]
    d = inner(flags[8]) != inner(flags[7])
    assert d[r1, e0:e1].all() and d.sum() == e1 - e0
    if nx >= 200:
        assert e1 - e0 == 100 and e0 // 64 != (e1 - 1) // 64
    assert len({x0 for x0, _ in uir.words_of(uir.changed_cells(co[8], co[7]))}) >= (2 if nx >= 130 else 1)
    # 10: back to 1
    assert np.array_equal(planes[9], planes[0]) and np.array_equal(co[9], co[0])
    # 11: one more iced cell in every 4 x 64 tile
    d = inner(flags[10]) != inner(flags[9])
    assert np.array_equal(d.reshape(-1).sum(), uir.groups(ny) * uir.tiles(nx))
    padded = np.zeros((uir.groups(ny) * 4, uir.tiles(nx) * 64), bool)
    padded[:ny, :nx] = d
    assert (padded.reshape(uir.groups(ny), 4, uir.tiles(nx), 64).sum(axis=(1, 3)) == 1).all()
    assert uir.word_marks(nx, ny, *win, uir.changed_cells(co[10], co[9])).all()
    # 12: the knife edges, in the working precision
    (a, b), (c, e) = lay["lf04"], lay["lf025"]
    p, f = inner(planes[11]), inner(flags[11])
    assert p[a] == dt(0.2) and not f[a] and p[b] > dt(0.2) and p[b] == np.nextafter(dt(0.2), dt(1)) and f[b]
    assert land[c] + p[c] == dt(0.5) and f[c] and land[e] + p[e] == np.nextafter(dt(0.5), dt(0)) and not f[e]
    assert (inner(flags[11]) != inner(flags[0])).sum() == 2


def test_model_counts_are_ordered():
    """brute force <= the words' marks <= the cap, for every plane of every set"""
    for name, nx, ny, win, halo, maxdist, kern in uic.SETS:
        land, lf_l, planes = uic.make(nx, ny, halo, np.float64)
        co = coasts(lf_l, planes, halo, nx, ny)
        for n in range(1, 12):
            ch = uir.changed_cells(co[n], co[n - 1])
            lo, mid, cap = (f(nx, ny, *win, ch) for f in (uir.brute_marks, uir.word_marks, uir.cap_marks))
            assert not (lo & ~mid).any() and not (mid & ~cap).any(), (name, uic.PLANES[n])
