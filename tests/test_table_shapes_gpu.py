"""The table contrast (sb_set_table_contrast, sb_table_kernels.hip) at the sizes where its loops
iterate.  ref: generic/sea_breeze_diag.f90:188-216.

tests/test_table_contrast_gpu.py stays within 176 x 128 cells and radius 40: one row chunk, one column block, at most two
row blocks, whole groups of eight rows, tables that never wrap.  Here, from the kernels' constants:

  big grid, 1100 x 900        nxh > 1024: a second, ragged row chunk (carries, the re-zeroed block sums, the index of S);
                              five column blocks; fifteen row blocks (0 .. 56 blocks of S above); 900 % 8 == 4: the clamped
                              loads and the guard of the eight-row pipeline; a frame that sums to more than 2^64.  One 80 x 80
                              square of land across column 1024 and row 832: the bisection, radii up to 40.
  the same as a frame         8 ghost cells, SB_BND_HALO: 1116 columns, the cell offset on a row of two chunks
  the same in fp32
  the reach, 320 x 10         radius 127 from the tables, 128 from the fallback; pole rows repeated up to 127 times
  t0 of both signs            signed fixed point: A and L wrap from the first negative cell

Everything goes through the C ABI.  Yardsticks, unchanged: the CPU oracle (oracle/sb_oracle.f90) on the same inputs;
fp64 |a - ref| <= 1e-7 max(|ref|, 1e-2), NaN only where the reference has NaN (table_ref.close64); fp32 the shared rule
of oracle/fp32_criterion.py against the oracle's fp64 build.  Every cell is in the band (mask = +-100), two levels, zero
initial state, six launches per call.  tests/test_table_format_model.py holds a numpy model of the format to the oracle
on the same inputs, without a GPU.
"""
import numpy as np
import pytest

import table_ref as tr
from oracle import fp32_criterion as crit
from seabreeze_param_amd import hip

pytestmark = pytest.mark.gpu

f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


@pytest.fixture
def table(hipctx):
    hipctx.set_table_contrast(True)
    yield hipctx
    hipctx.set_table_contrast(False)
    hipctx.set_search_radius_hint(16)


def _oracle_steps(oracle, st, p, per, mask, halo=0, bnd=1):
    """the fp64 oracle from zero state over the steps of `per`: {tn: (state, largest radius)}, never modified"""
    ny, nx = p.shape[1:]
    so = tr.zeros(4, np.float64, ny, nx)
    out = {}
    for tn in sorted(per):
        th, u, v = per[tn]
        oracle.seabreeze_diag(tr.DT_S, tn, f8(p), f8(u), f8(v), f8(th), f8(mask), f8(st.z), f8(st.sigma), *so, halo=halo, bnd=bnd)
        out[tn] = ([a.copy() for a in so], oracle.last_nn_max)
        for a in out[tn][0]:
            a.setflags(write=False)
    return out


def _run(ctx, st, p, per, mask, halo=0, bnd=hip.SB_BND_GLOBAL):
    """the library from zero state over the steps of `per`: {tn: (state, counters)}; six launches per call"""
    ny, nx = p.shape[1:]
    sh = tr.zeros(4, p.dtype, ny, nx)
    out = {}
    for tn in sorted(per):
        th, u, v = per[tn]
        ctx.seabreeze_diag(tr.DT_S, tn, p, u, v, th, mask, st.z, st.sigma, *sh, halo=halo, bnd=bnd)
        assert ctx.last_step_report()["kernel_launches"] == tr.TABLE_LAUNCHES
        out[tn] = ([a.copy() for a in sh], ctx.last_counters())
    return out


def _assert_close(got, ref, what):
    for a, b, nm in zip(got, ref, tr.NAMES):
        tr.close64(a, b, f"{what} {nm}")


# ---- 1, 3: the big global grid

@pytest.fixture(scope="module")
def big_inputs():
    nx, ny = tr.BIG
    return tr.inputs(nx, ny, tr.big_land(), np.float64)


@pytest.fixture(scope="module")
def big_ref(oracles, big_inputs):
    ref = _oracle_steps(oracles[8], *big_inputs)
    assert ref[1][1] == 40 and not np.isnan(ref[2][0][2]).any() and np.count_nonzero(ref[2][0][3]) > 0
    return ref


def test_big_grid_fp64(table, oracles, big_inputs, big_ref):
    """Two row chunks, five column blocks, fifteen row blocks, the ragged tails of 900 rows, radii up to 40 across the
    chunk and block boundaries -- on a table whose last entry has passed 2^64 (asserted on the inputs first)."""
    nx, ny = tr.BIG
    st, p, per, mask = big_inputs
    assert nx > 1024 and nx % 64 and -(-nx // 256) == 5 and -(-ny // 64) == 15 and ny % 8 == 4 and ny % 16 == 4
    s = tr.frame_sum_over_2_64(tr.t0_of(oracles[8], per[1][0], st.z, st.sigma))
    assert s >= 1.05, f"the fixed-point frame sums to {s} x 2^64: table A does not wrap"
    got = _run(table, *big_inputs)
    for tn in (1, 2):
        state, c = got[tn]
        ref, nn_max = big_ref[tn]
        _assert_close(state, ref, f"big tn={tn}")
        assert c["global_path_cells"] == 0 and c["one_class_cells"] == 0 and c["band_cells"] == nx * ny, c
        assert c["max_radius"] == nn_max == 40, (c, nn_max)


def test_big_grid_fp32_against_the_fp64_oracle(table, oracles):
    """The same land in single precision: one format for both precisions, every fp32 t0 exact in it."""
    nx, ny = tr.BIG
    dt = np.float32
    st, p, per, mask = tr.inputs(nx, ny, tr.big_land(), dt)
    sh, so = tr.zeros(4, dt, ny, nx), tr.zeros(4, np.float64, ny, nx)
    band = np.ones((ny, nx), bool)                           # no cell is masked
    steps = []
    for tn in (1, 2):
        th, u, v = per[tn]
        gp, op = [a.copy() for a in sh], [a.copy() for a in so]
        oracles[8].seabreeze_diag(tr.DT_S, tn, f8(p), f8(u), f8(v), f8(th), f8(mask), f8(st.z), f8(st.sigma), *so, halo=0, bnd=1)
        table.seabreeze_diag(tr.DT_S, tn, p, u, v, th, mask, st.z, st.sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
        assert table.last_step_report()["kernel_launches"] == tr.TABLE_LAUNCHES
        steps.append(crit.check_step(tn, gp, sh, op, so, band, timestep=tr.DT_S))
        c = table.last_counters()
        assert c["global_path_cells"] == 0 and c["max_radius"] == oracles[8].last_nn_max == 40, c
    res = crit.merge(steps)
    assert res["ok"], res


# ---- 2: the big grid as a frame

def test_big_frame_halo(table, oracles):
    """SB_BND_HALO, 8 ghost cells, stripes only: 1116 columns keep two row chunks, and a cell's column is its place in
    the row less the ghost width.  No window leaves the frame (radii <= 6 < 8, asserted), so the oracle reads the same
    cells."""
    nx, ny = tr.BIG
    h = tr.BIG_HALO
    st, p, per, mask = tr.inputs(nx, ny, tr.stripes_land(nx + 2 * h, ny + 2 * h), np.float64, halo=h)
    assert nx + 2 * h > 1024
    ref = _oracle_steps(oracles[8], st, p, per, mask, halo=h, bnd=2)
    assert max(ref[tn][1] for tn in (1, 2)) <= 6 < h
    got = _run(table, st, p, per, mask, halo=h, bnd=hip.SB_BND_HALO)
    for tn in (1, 2):
        state, c = got[tn]
        assert not any(np.isnan(a).any() for a in state)
        _assert_close(state, ref[tn][0], f"frame tn={tn}")
        assert c["global_path_cells"] == 0 and c["band_cells"] == nx * ny, c


# ---- 4: the reach

@pytest.mark.parametrize("w, radius, fallback_columns", [(253, 127, 0), (255, 128, 1)])
def test_reach(table, oracles, w, radius, fallback_columns):
    """A land block of w columns over all ten rows, across the seam: its middle column is (w + 1) // 2 cells from the
    sea.  127 is the last radius the tables answer; at 128 that one column, and only it, takes the global-memory search.
    Ten rows: a wide window repeats each pole row up to 127 times, and 10 % 8 != 0."""
    nx, ny = tr.REACH_GRID
    assert (w + 1) // 2 == radius and (nx - 1) // 2 >= tr.TAB_REACH and ny % 8
    st, p, per, mask = tr.inputs(nx, ny, tr.reach_land(w), np.float64, steps=(1,))
    ref, nn_max = _oracle_steps(oracles[8], st, p, per, mask)[1]
    assert nn_max == radius
    state, c = _run(table, st, p, per, mask)[1]
    _assert_close(state, ref, f"reach w={w}")
    assert c["global_path_cells"] == fallback_columns * ny and c["one_class_cells"] == 0, c
    assert c["max_radius"] == radius and c["band_cells"] == nx * ny, c


# ---- 5: negative and mixed-sign t0

def test_mixed_sign_t0(table, oracles):
    """The block grid of tests/test_table_contrast_gpu.py with theta - 290 K: t0 of about -5 .. 33, signed fixed point."""
    nx, ny, w = tr.BLOCK
    st, p, per, mask = tr.inputs(nx, ny, tr.block_land(nx, ny, w, nx), np.float64, shift=tr.CELSIUS)
    t0 = tr.t0_of(oracles[8], per[1][0], st.z, st.sigma)
    assert t0.min() < 0 < t0.max(), (t0.min(), t0.max())
    ref = _oracle_steps(oracles[8], st, p, per, mask)
    got = _run(table, st, p, per, mask)
    for tn in (1, 2):
        state, c = got[tn]
        _assert_close(state, ref[tn][0], f"mixed sign tn={tn}")
        assert c["global_path_cells"] == 0 and c["one_class_cells"] == 0, c
        assert c["max_radius"] == ref[tn][1] == 40, (c, ref[tn][1])
