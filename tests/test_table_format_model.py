"""The format of the table contrast as a numpy model, tests/table_ref.py::table_thc, against the
CPU oracle's thc -- without a GPU, on the inputs of tests/test_table_shapes_gpu.py: the big grid whose table A wraps, a
radius of 127 with pole rows repeated 127 times, and t0 of both signs (thc near the floor of the rule: the rounding to 36
fractional bits is the whole error budget there; DESIGN derives 2.1e-10 against the 1e-9 allowed).

Yardstick: |a - ref| <= 1e-7 max(|ref|, 1e-2), NaN where the oracle has NaN (table_ref.close64).  If a GPU case fails,
this says whether the format or a kernel is at fault.
"""
import numpy as np

import table_ref as tr


def _oracle_thc(oracle, st, p, step, mask):
    th, u, v = step
    ny, nx = mask.shape
    so = tr.zeros(4, np.float64, ny, nx)
    oracle.seabreeze_diag(tr.DT_S, 1, p, u, v, th, mask, st.z, st.sigma, *so, halo=0, bnd=1)
    assert not np.isnan(so[2]).any()
    return so[2], oracle.last_nn_max


def _model_against_oracle(oracle, nx, ny, land, nn_max, shift=0.0):
    st, p, per, mask = tr.inputs(nx, ny, land, np.float64, steps=(1,), shift=shift)
    ref, nn_ref = _oracle_thc(oracle, st, p, per[1], mask)
    t0 = tr.t0_of(oracle, per[1][0], st.z, st.sigma)
    thc, nn = tr.table_thc(t0, land)
    assert nn.min() >= 1 and nn.max() == nn_ref == nn_max, (nn.min(), nn.max(), nn_ref)
    e = np.abs(thc - ref)
    print(f"max |model - oracle| = {e.max():.3e}, smallest |thc| = {np.abs(ref).min():.3e}")
    tr.close64(thc, ref, "model thc")
    return t0


def test_big_grid_whose_table_wraps(oracles):
    nx, ny = tr.BIG
    t0 = _model_against_oracle(oracles[8], nx, ny, tr.big_land(), 40)
    s = tr.frame_sum_over_2_64(t0)
    assert s >= 1.05, f"the frame sums to {s} x 2^64: table A does not wrap"


def test_radius_127_with_pole_rows_repeated(oracles):
    nx, ny = tr.REACH_GRID
    _model_against_oracle(oracles[8], nx, ny, tr.reach_land(253), tr.TAB_REACH)


def test_mixed_sign_t0(oracles):
    nx, ny, w = tr.BLOCK
    t0 = _model_against_oracle(oracles[8], nx, ny, tr.block_land(nx, ny, w, nx), 40, shift=tr.CELSIUS)
    assert t0.min() < 0 < t0.max(), (t0.min(), t0.max())


def test_fixed_point_matches_the_row_pass_rounding():
    """The row pass rounds by an fma into the mantissa of 1.5 x 2^52: round to nearest, ties to even, of the exact
    product -- np.rint of t0 * 2^36 (a power of two: the product is exact)."""
    t = np.array([0.0, 1.0, -1.0, 2.0 ** -37, -(2.0 ** -37), 3 * 2.0 ** -37, 300.125, -4.75, 2047.999])
    want = [0, 1 << 36, -(1 << 36), 0, 0, 2, int(300.125 * 2 ** 36), int(-4.75 * 2 ** 36), round(2047.999 * 2 ** 36)]
    assert tr.fixed_point(t).tolist() == want


def test_a_wrapped_table_still_gives_exact_window_sums():
    """Entries of both signs, up to 13 x 2^58, on a frame whose sum passes 2^64 hundreds of times: every window sum of
    the model's prefix table equals the direct sum over the window, modulo 2^64."""
    fx = (np.arange(40 * 50, dtype=np.int64).reshape(40, 50) % 17 - 3) << 58
    assert sum(int(v) for v in fx.ravel()) > 100 << 64
    P = tr._prefix(fx.view(np.uint64), np.uint64)
    y, x = np.array([5, 20, 39]), np.array([7, 25, 49])
    for r in (1, 3):
        got = tr._rect(P, x - r, np.minimum(x + r, 49), y - r, np.minimum(y + r, 39)).view(np.int64)
        for k in range(3):
            win = fx[y[k] - r:y[k] + r + 1, x[k] - r:x[k] + r + 1]
            want = sum(int(v) for v in win.ravel()) % (1 << 64)
            assert int(got[k]) % (1 << 64) == want
