"""The guard's specified taint against the exact affected set, on the CPU (tests/guard_ref.py; sb_guard_kernels.hip).

A superset costs time only, a subset is a bug: on every directed field of tests/test_nonfinite_guard_gpu.py and for every
contrast kernel's reach, each band cell whose final window holds a bad cell and whose radius the kernel answers itself, and
each band cell that is bad itself, is in the specified taint.  Where every radius of the field lies within the reach -- all
of them on these fields but the table grid under the strip kernels' reaches -- that is the exact set, whole.  Band cells
beyond the reach take the global-memory search whatever the guard does.
"""
import numpy as np
import pytest

import guard_ref as gr
import radius_ref as rr
from seabreeze_param_amd import synth

KERNELS = {"strip": dict(reach=16), "strip32": dict(reach=31), "tile24": dict(tile=(32, 32, 24)), "tile32": dict(tile=(32, 16, 32)),
           "table": dict(reach=127)}


def _check(bad, mask_f, halo, bnd, what, expect_hit=True):
    exact, radius, isband = gr.affected(bad, mask_f, 180.0, halo, bnd)
    assert exact.any() == expect_hit, (what, int(exact.sum()))
    for name, kw in KERNELS.items():
        taint = gr.specified_taint(bad, isband, halo, bnd, **kw)
        assert not (taint & ~isband).any()
        need = gr.must_cover(exact, radius, bad, isband, halo, bnd, **kw)
        assert not (need & ~taint).any(), (what, name, np.argwhere(need & ~taint)[:4])
        r = kw.get("reach", kw.get("tile", (0, 0, 0))[2])
        if radius.max() <= r:
            assert not (exact & ~taint).any(), (what, name)
        if not expect_hit:
            assert not taint.any(), (what, name)
    return exact, isband


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_global_cases(oracles, dt):
    orc = oracles[np.dtype(dt).itemsize]
    st, cd = gr.global_field(orc, dt)
    nx, ny = gr.GRID
    radius = rr.search_radius(cd, 180.0, 0, rr.BND_GLOBAL)
    isband, land = radius != 0, cd >= 0
    th = synth.theta_step(st, 2, dt)
    cases = gr.directed(land, isband, radius)
    assert set(c[0] for c in cases) == set("abcdehik")
    for name, spec in cases.items():
        t, z = gr.poison(th, st.z, spec)
        bad = gr.bad_plane(t, z)
        assert int(bad.sum()) == len(spec), name
        exact, _ = _check(bad, cd, 0, rr.BND_GLOBAL, name)
        if name.startswith("c_"):               # not a band cell itself, inside band cells' windows
            (_, y, x, _), = spec
            assert not isband[y, x] and exact.any()
        if name.startswith("e_"):               # the cell in the last column is inside windows on both sides of the seam
            one = gr.affected(gr.bad_plane(*gr.poison(th, st.z, spec[2:])), cd, 180.0, 0, rr.BND_GLOBAL)[0]
            cols = np.unique(np.argwhere(one)[:, 1])
            assert (cols >= nx - 2).any() and (cols <= 1).any(), cols
    # (j) no bad cell: nothing marked, nothing tainted
    bad = gr.bad_plane(th, st.z)
    assert not bad.any()
    _check(bad, cd, 0, rr.BND_GLOBAL, "j", expect_hit=False)


def test_wrapper_rule_last_column_and_seam(oracles):
    """(f) the f2py flavour's index rule never reads the last column -- an offset that lands there reads column 1 (index 0) --
    so a NaN there changes nothing; a NaN in column 1 is seen from both sides of the seam, the last column's cells included"""
    dt = np.float64
    st, cd = gr.global_field(oracles[8], dt)
    nx, ny = gr.GRID
    radius = rr.search_radius(cd, 180.0, 0, rr.BND_WRAPPER)
    isband = radius != 0
    th = synth.theta_step(st, 2, dt)
    rows = np.flatnonzero(isband[:, nx - 1] | isband[:, 0] | isband[:, 1] | isband[:, nx - 2])
    assert rows.size
    y = int(rows[0])
    bad = gr.bad_plane(*gr.poison(th, st.z, [("theta", y, nx - 1, gr.NAN)]))
    _check(bad, cd, 0, rr.BND_WRAPPER, "last column", expect_hit=False)
    bad = gr.bad_plane(*gr.poison(th, st.z, [("theta", y, 0, gr.NAN)]))
    exact, _ = _check(bad, cd, 0, rr.BND_WRAPPER, "column 1")
    cols = np.unique(np.argwhere(exact)[:, 1])
    assert (cols >= nx - 2).any() and (cols <= 1).any(), cols


def test_um_ghost_cell(oracles):
    """(g) SB_BND_HALO: a NaN in a ghost cell of theta's frame reaches the band cells whose windows extend into the ghost ring"""
    dt = np.float64
    hs = 2
    st, cd_l, inner = gr.um_field(oracles[8], dt, hs=hs)
    cd_s = inner(cd_l, hs)
    radius = rr.search_radius(cd_s, 180.0, hs, rr.BND_HALO)
    Y, X = gr.um_ghost_cell(radius != 0, radius, hs)
    th = inner(synth.theta_step(st, 2, dt), hs)
    z = inner(st.z, hs)
    th[Y, X] = np.nan
    _check(gr.bad_plane(th, z), cd_s, hs, rr.BND_HALO, "ghost cell")


def test_table_grid_block(oracles):
    """the table grid: radii far beyond the strip kernels' reach; the 40 x 40 block of missing values across a coast"""
    import table_ref as tr
    dt = np.float64
    nx, ny = gr.TABLE_GRID
    land = gr.table_land()
    st, p, per, mask = tr.inputs(nx, ny, land, dt, steps=(2,))
    radius = rr.search_radius(mask, 180.0, 0, rr.BND_GLOBAL)
    assert 32 < radius.max() <= 127
    th = per[2][0]
    for name, spec in (("one", [("theta", 20, 150, gr.NAN)]),
                       ("block", [("theta", y, x, gr.MISSING) for y in range(20, 60) for x in range(120, 160)])):
        _check(gr.bad_plane(*gr.poison(th, st.z, spec)), mask, 0, rr.BND_GLOBAL, name)
