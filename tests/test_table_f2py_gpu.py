"""The table contrast for the f2py flavour (sb_set_table_contrast_f2py beside sb_set_table_contrast; sb_table_kernels.hip,
DESIGN section 2.4d): sb_diag_* under the wrapper's index rule -- latitude clamped, column max(1, modulo(jj, nlons)) -- from
tables built over the EFFECTIVE row, whose last column holds column 1's value and land-side bit.  Six launches (k_scan,
k_prep, the row pass -- which writes the t0 plane, no k_t0 --, the column pass, the query, k_wind) where the flavour runs
five.  ref: python_wrapper/seabreezediag/seabreeze_diag_python.f90:165-285.

Everything goes through the C ABI, the device-pointer entry point sb_diag_*_dev (arrays that keep their address, and an
`output` whose every word the test owns).  Yardsticks: the CPU oracle's wrapper flavour (oracle/sb_oracle.f90) on the same
inputs -- fp64 under table_ref.close64, fp32 under oracle/fp32_criterion.py against the oracle's fp64 build -- and the same
call with the new switch off, as integer views where the sums are exact.

The block grids: that of tests/test_table_contrast_gpu.py (160 x 112, every cell in the band, land an 80 x 80 block across
the longitude seam that touches row 1), and its mirror image, whose block touches the LAST row -- the row the flavour never
processes and windows still read, with multiplicity, through the latitude clamp.  Expected radii: tests/radius_ref.py under
the wrapper rule.
"""
import numpy as np
import pytest
import torch  # before the library is loaded: one HIP runtime (seabreeze_param_amd/hip.py)

import radius_ref as rr
import table_ref as tr
from conftest import relerr
from oracle import fp32_criterion as crit
from seabreeze_param_amd import hip, synth

pytestmark = pytest.mark.gpu

NX, NY, W = tr.BLOCK
NZ = 3
F2PY_LAUNCHES = 5           # SCAN PREP T0 CONTRAST WIND
SENTINEL = -777.25
NAMES = ("ws", "wd", "thc", "sb_con", "t0", "out_ws", "out_wd")
f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


def _bits(a):
    return a.view(np.int64 if a.itemsize == 8 else np.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


@pytest.fixture
def f2py_table(hipctx):
    hipctx.set_table_contrast(True)
    hipctx.set_table_contrast_f2py(True)
    yield hipctx
    hipctx.set_table_window_cache(False)
    hipctx.set_table_contrast_f2py(False)
    hipctx.set_table_contrast(False)
    hipctx.set_search_radius_hint(16)


def _inputs(nx, ny, dt, steps=(1, 2)):
    st = synth.static_fields(nx, ny, dt)
    per = {tn: (synth.theta_step(st, tn, dt),) + synth.wind_step(st, NZ, tn, dt) for tn in steps}
    return st, synth.pressure_1d(NZ, dt), per


@pytest.fixture(scope="module")
def grids():
    """the two block grids: inputs, masks, and what the CPU says about them -- asserted here, once"""
    inp = _inputs(NX, NY, np.float64, steps=(1, 2, 3))
    first = tr.block_land(NX, NY, W, NX)
    land = {"row0": first, "lastrow": np.ascontiguousarray(first[::-1])}
    assert land["row0"][0].any() and not land["row0"][NY - 1].any() and land["lastrow"][NY - 1].any()
    masks = {k: tr.mask_of(v, np.float64) for k, v in land.items()}
    radius = {k: rr.search_radius(m, bnd=rr.BND_WRAPPER) for k, m in masks.items()}
    for k, r in radius.items():
        assert r.max() == 40 and (r[:NY - 1] >= 1).all() and (r[NY - 1] == 0).all(), k   # beyond 32; no cell is one-class
    return inp, masks, radius


def _oracle(oracle, inp, mask, steps=(1, 2), theta_of=None, **kw):
    """the oracle's wrapper flavour from zero state: per step [ws, wd, thc, sb_con, t0, out_ws, out_wd], never modified"""
    st, p1, per = inp
    ws, wd, thc = tr.zeros(3, np.float64, *mask.shape)
    out = {}
    for tn in steps:
        th, u, v = per[tn]
        th = th if theta_of is None else theta_of(th)
        o = oracle.diag(tn, f8(p1), f8(st.z), f8(st.sigma), f8(th), f8(v), f8(u), f8(mask), ws, wd, thc, **kw)
        out[tn] = ([ws.copy(), wd.copy(), thc.copy()] + [o[k].copy() for k in range(4)], oracle.last_nn_max)
        for a in out[tn][0]:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def block_ref(oracles, grids):
    inp, masks, _ = grids
    ref = {k: _oracle(oracles[8], inp, m) for k, m in masks.items()}
    for k in masks:
        assert ref[k][1][1] == 40 and np.count_nonzero(ref[k][1][0][3][:NY - 1]) > 0, k      # sb_con is not all zero
        assert not np.isnan(ref[k][1][0][2]).any()
    return ref


class Dev:
    """device copies of a case's inputs, a state and an `output` of its own (filled with a sentinel); one call -> what it left"""

    def __init__(self, ctx, inp, dt=np.float64, **kw):
        st, p1, per = inp
        self.ctx, self.dt, self.kw = ctx, np.dtype(dt), kw
        self.ny, self.nx = st.z.shape
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=self.dt)).cuda()
        self.p, self.z, self.sg = up(p1), up(st.z), up(st.sigma)
        self.per = {tn: tuple(up(a) for a in v) for tn, v in per.items()}
        self.mask = None
        self.state = [torch.zeros((self.ny, self.nx), dtype=self.p.dtype, device="cuda") for _ in range(3)]
        self.out = torch.full((4, self.ny, self.nx), SENTINEL, dtype=self.p.dtype, device="cuda")
        torch.cuda.synchronize()

    def set_mask(self, mask):
        m = torch.from_numpy(np.ascontiguousarray(mask, dtype=self.dt))
        if self.mask is None:
            self.mask = m.cuda()
        else:
            self.mask.copy_(m)
        torch.cuda.synchronize()

    def call(self, tn, mask=None, theta=None):
        if mask is not None:
            self.set_mask(mask)
        th, u, v = self.per[tn]
        if theta is not None:
            th = torch.from_numpy(np.ascontiguousarray(theta, dtype=self.dt)).cuda()
        self.ctx.diag_dev(self.dt, tn, NZ, self.nx, self.ny, self.p.data_ptr(), self.z.data_ptr(), self.sg.data_ptr(), th.data_ptr(),
                          v.data_ptr(), u.data_ptr(), self.mask.data_ptr(), *[s.data_ptr() for s in self.state], self.out.data_ptr(),
                          stream=hip.torch_stream_handle(torch), **self.kw)
        torch.cuda.synchronize()
        o = self.out.cpu().numpy()
        return dict(vals=[s.cpu().numpy() for s in self.state] + [o[k] for k in range(4)], c=self.ctx.last_counters(),
                    launches=self.ctx.last_step_report()["kernel_launches"], rep=self.ctx.table_cache_report())


def _run(ctx, inp, mask, steps=(1, 2), **kw):
    d = Dev(ctx, inp, **kw)
    return {tn: d.call(tn, mask if tn == steps[0] else None) for tn in steps}


def _assert_close(r, ref, what):
    """state planes whole; the planes of `output` over the rows the flavour writes, the sentinel in the last"""
    ny = r["vals"][0].shape[0]
    for a, b, nm in zip(r["vals"], ref, NAMES):
        rows = slice(None) if nm in NAMES[:3] else slice(0, ny - 1)
        tr.close64(a[rows], b[rows], f"{what} {nm}")
    for a, nm in zip(r["vals"][3:], NAMES[3:]):
        assert (a[ny - 1] == SENTINEL).all(), f"{what}: row nlats of {nm} was written"


def _assert_same(r, t, what, counters=True):
    for a, b, nm in zip(r["vals"], t["vals"], NAMES):
        _same_bits(a, b, f"{what} {nm}")
    assert not counters or r["c"] == t["c"], (what, r["c"], t["c"])


# ---- 1: fp64 against the oracle

@pytest.mark.parametrize("grid", ["row0", "lastrow"])
def test_fp64_block_grids_against_the_oracle(f2py_table, grids, block_ref, grid):
    """Seam split over the effective row, the clamp at row 1 and at the unprocessed last row with multiplicity, radii up to
    40 from the tables alone, the flavour's state update behind them."""
    inp, masks, radius = grids
    got = _run(f2py_table, inp, masks[grid])
    for tn in (1, 2):
        r = got[tn]
        _assert_close(r, block_ref[grid][tn][0], f"{grid} tn={tn}")
        assert r["c"]["global_path_cells"] == 0 and r["c"]["one_class_cells"] == 0, r["c"]
        assert r["c"]["max_radius"] == block_ref[grid][tn][1] == int(radius[grid].max()) == 40, r["c"]
        assert r["c"]["band_cells"] == NX * (NY - 1)
        assert r["launches"] == tr.TABLE_LAUNCHES, r["launches"]


# ---- 2: the t0 plane, the last row

def test_t0_plane_has_k_t0s_bits_and_row_nlats_is_untouched(f2py_table, grids):
    inp, masks, _ = grids
    on = _run(f2py_table, inp, masks["lastrow"])
    f2py_table.set_table_contrast_f2py(False)
    off = _run(f2py_table, inp, masks["lastrow"])
    f2py_table.set_table_contrast_f2py(True)
    for tn in (1, 2):
        assert on[tn]["launches"] == tr.TABLE_LAUNCHES and off[tn]["launches"] == F2PY_LAUNCHES
        t0_on, t0_off = on[tn]["vals"][4], off[tn]["vals"][4]
        _same_bits(t0_on, t0_off, f"t0 plane tn={tn}")
        assert not (t0_on[:NY - 1] == SENTINEL).any()
        for r in (on[tn], off[tn]):
            for a in r["vals"][3:]:
                assert (a[NY - 1] == SENTINEL).all()
        # the winds pass through no window: the same bits; the contrast to the rounding of the window means
        for k in (0, 1, 5, 6):
            _same_bits(on[tn]["vals"][k], off[tn]["vals"][k], f"{NAMES[k]} tn={tn}")
        tr.close64(on[tn]["vals"][2], off[tn]["vals"][2], f"thc on against off tn={tn}")


# ---- 3: the last-column rule, directed

def test_last_column_never_enters_a_window(f2py_table, oracles, grids):
    """theta + 7 K in column nx: the wrapper rule reads that column for no window, not even for its own cells, and the sums
    are exact -- thc keeps its bits everywhere; only the t0 plane's last column moves.  A truly periodic reading of the same
    inputs (the oracle's host-model flavour, bnd = 1) does change thc: the test shows something."""
    inp, masks, _ = grids
    st, p1, per = inp
    mask = masks["row0"]
    th, u, v = per[1]
    th7 = th.copy()
    th7[:, NX - 1] += 7.0
    base = Dev(f2py_table, inp).call(1, mask)
    moved = Dev(f2py_table, inp).call(1, mask, theta=th7)
    assert base["launches"] == moved["launches"] == tr.TABLE_LAUNCHES
    for k in (0, 1, 2, 3, 5, 6):
        _same_bits(base["vals"][k], moved["vals"][k], NAMES[k])
    assert base["c"] == moved["c"]
    d = moved["vals"][4] - base["vals"][4]
    assert (d[:NY - 1, :NX - 1] == 0).all() and (np.abs(d[:NY - 1, NX - 1] - 7.0) < 1e-9).all()
    p3 = synth.pressure_3d(st, NZ, np.float64)
    thc = []
    for theta in (th, th7):
        so = tr.zeros(4, np.float64, NY, NX)
        oracles[8].seabreeze_diag(tr.DT_S, 1, p3, u, v, theta, mask, st.z, st.sigma, *so, halo=0, bnd=1)
        thc.append(so[2].copy())
    assert relerr(thc[1], thc[0], floor=1e-2) > 1e-7


# ---- 4: single precision

def test_fp32_block_grid_against_the_fp64_oracle(f2py_table, oracles, grids):
    """timestep = target_time = 6 h: every step is one on which the flavour stores this step's winds (ref :268-273), so
    the carried state shows the mean wind speed the criterion derives from it (oracle/fp32_criterion.mean_wind)."""
    dt = np.float32
    inp = _inputs(NX, NY, dt)
    st, p1, per = inp
    mask = tr.mask_of(tr.block_land(NX, NY, W, NX), dt)
    kw = dict(timestep=360.0, target_time=6.0)
    ref = _oracle(oracles[8], inp, mask, **kw)
    d = Dev(f2py_table, inp, dt=dt, **kw)
    band = np.ones((NY, NX), bool)
    band[NY - 1] = False                                     # the row the flavour does not process
    res = []
    gp = tr.zeros(4, dt, NY, NX)
    op = tr.zeros(4, np.float64, NY, NX)
    for tn in (1, 2):
        r = d.call(tn, mask if tn == 1 else None)
        gn, on = r["vals"][:4], ref[tn][0][:4]
        res.append(crit.check_step(tn, gp, gn, op, on, band, timestep=360.0 * 60.0))
        gp, op = gn, on
        assert r["c"]["global_path_cells"] == 0 and r["c"]["max_radius"] == ref[tn][1] == 40, r["c"]
        assert r["launches"] == tr.TABLE_LAUNCHES
    out = crit.merge(res)
    assert out["ok"] and out["cells_compared"] > 0, out


# ---- 5: cells the tables do not answer

def test_window_wider_than_the_circle(f2py_table, oracles):
    """48 columns: the tables answer radii up to 23.  Land over rows 1 .. 30, sea beyond: rows 1 .. 6 are 25 .. 30 cells
    from the sea and take the global-memory search -- with the switch on as with it off, the same code, the same bits.
    Rows 7 .. 14 (radii 17 .. 24: the tables' or the global-memory search's with the switch on, the LDS kernel's or the
    global-memory search's with it off) are kept out of the band, so the counters of the two calls are equal."""
    nx, ny = 48, 40
    inp = _inputs(nx, ny, np.float64)
    y = np.arange(ny)[:, None] + np.zeros((1, nx), int)
    mask = np.where(y < 30, 100.0, -100.0)
    mask[(y >= 6) & (y < 14)] = 1000.0
    radius = rr.search_radius(mask, bnd=rr.BND_WRAPPER)
    slow = radius > 23
    assert slow.sum() == 6 * nx and radius.max() == 30 and not ((radius > 16) & ~slow).any() and (radius >= 0).all()
    ref = _oracle(oracles[8], inp, mask)
    on = _run(f2py_table, inp, mask)
    f2py_table.set_table_contrast_f2py(False)
    off = _run(f2py_table, inp, mask)
    f2py_table.set_table_contrast_f2py(True)
    for tn in (1, 2):
        _assert_close(on[tn], ref[tn][0], f"circle tn={tn}")
        assert on[tn]["launches"] == tr.TABLE_LAUNCHES and off[tn]["launches"] == F2PY_LAUNCHES
        assert on[tn]["c"] == off[tn]["c"], (on[tn]["c"], off[tn]["c"])
        assert on[tn]["c"]["global_path_cells"] == 6 * nx and on[tn]["c"]["one_class_cells"] == 0 and on[tn]["c"]["max_radius"] == 30
        for k in (2, 3):
            _same_bits(np.where(slow, on[tn]["vals"][k], 0.0), np.where(slow, off[tn]["vals"][k], 0.0), f"tn={tn} {NAMES[k]}, slow cells")


def test_one_class_grid(f2py_table):
    """All land: every band cell is NaN and counted, with the switch on as with it off: the same bits, the same counters."""
    nx, ny = 48, 40
    inp = _inputs(nx, ny, np.float64)
    mask = np.full((ny, nx), 100.0)
    on = _run(f2py_table, inp, mask)
    f2py_table.set_table_contrast_f2py(False)
    off = _run(f2py_table, inp, mask)
    f2py_table.set_table_contrast_f2py(True)
    for tn in (1, 2):
        assert np.isnan(on[tn]["vals"][2][:ny - 1]).all() and not np.isnan(on[tn]["vals"][2][ny - 1]).any()
        assert on[tn]["c"]["global_path_cells"] == on[tn]["c"]["one_class_cells"] == nx * (ny - 1), on[tn]["c"]
        _assert_same(on[tn], off[tn], f"all land tn={tn}")
        assert on[tn]["launches"] == tr.TABLE_LAUNCHES and off[tn]["launches"] == F2PY_LAUNCHES


# ---- 6: the switches

def test_switch_semantics(f2py_table, grids):
    """The new switch alone is ignored; on, off and on again on one context gives the first run's bits; a host-model call
    does not know the switch."""
    inp, masks, _ = grids
    st, p1, per = inp
    mask = masks["row0"]
    ctx = f2py_table

    def host_model():
        sh = tr.zeros(4, np.float64, NY, NX)
        th, u, v = per[1]
        ctx.seabreeze_diag(tr.DT_S, 1, synth.pressure_3d(st, NZ, np.float64), u, v, th, mask, st.z, st.sigma, *sh, halo=0,
                           bnd=hip.SB_BND_GLOBAL)
        return sh, ctx.last_counters(), ctx.last_step_report()["kernel_launches"]

    first = _run(ctx, inp, mask)
    hm_on = host_model()
    ctx.set_table_contrast_f2py(False)
    hm_off = host_model()
    plain_table = _run(ctx, inp, mask)                       # (sb_set_table_contrast alone: the flavour ignores it)
    ctx.set_table_contrast(False)
    plain = _run(ctx, inp, mask)
    ctx.set_table_contrast_f2py(True)
    alone = _run(ctx, inp, mask)                             # the new switch alone
    ctx.set_table_contrast(True)
    again = _run(ctx, inp, mask)
    for tn in (1, 2):
        assert first[tn]["launches"] == again[tn]["launches"] == tr.TABLE_LAUNCHES
        assert plain[tn]["launches"] == alone[tn]["launches"] == plain_table[tn]["launches"] == F2PY_LAUNCHES
        assert plain[tn]["c"]["global_path_cells"] > 0 and first[tn]["c"]["global_path_cells"] == 0
        _assert_same(alone[tn], plain[tn], f"the new switch alone, tn={tn}")
        _assert_same(plain_table[tn], plain[tn], f"the table switch alone, tn={tn}")
        _assert_same(again[tn], first[tn], f"on again, tn={tn}")
    assert hm_on[2] == hm_off[2] == tr.TABLE_LAUNCHES and hm_on[1] == hm_off[1]
    for a, b, nm in zip(hm_on[0], hm_off[0], tr.NAMES):
        _same_bits(a, b, f"host-model call {nm}")


# ---- 7: stored windows

def test_stored_windows(f2py_table, oracles, grids, block_ref):
    """sb_set_table_window_cache for the flavour: the first call searches and stores, the next read W -- the same bits and
    counters as without the cache; the block moved by (7, 3) makes the next call search again; a host-model table call in
    between drops the windows (its planes are others') and is itself correct."""
    inp, masks, _ = grids
    st, p1, per = inp
    m1 = masks["row0"]
    m2 = tr.mask_of(tr.block_land(NX, NY, W, NX, dx=7, dy=3), np.float64)
    band = NX * (NY - 1)
    seq = [(1, m1), (2, None), (3, m2)]
    twin_d = Dev(f2py_table, inp)
    twin = [twin_d.call(tn, m) for tn, m in seq]
    assert all(t["rep"]["stored_cells"] == 0 and t["rep"]["searched_cells"] == 0 for t in twin)
    f2py_table.set_table_window_cache(True)
    d = Dev(f2py_table, inp)
    want = [dict(fills=1, searched_cells=band, stored_cells=0, calls=1), dict(fills=1, searched_cells=0, stored_cells=band, calls=2),
            dict(fills=2, searched_cells=band, stored_cells=0, calls=3)]
    for (tn, m), t, w in zip(seq, twin, want):
        r = d.call(tn, m)
        assert r["rep"] == w, (tn, r["rep"])
        assert r["launches"] == tr.TABLE_LAUNCHES
        _assert_same(r, t, f"cache tn={tn}")
    _assert_close(twin[1], block_ref["row0"][2][0], "tn=2")
    r = d.call(2)
    assert r["rep"]["stored_cells"] == band and r["rep"]["fills"] == 2, r["rep"]
    # a host-model table call on the same context: correct, and the flavour's next call searches again
    p3 = synth.pressure_3d(st, NZ, np.float64)
    th, u, v = per[1]
    sh, so = tr.zeros(4, np.float64, NY, NX), tr.zeros(4, np.float64, NY, NX)
    f2py_table.seabreeze_diag(tr.DT_S, 1, p3, u, v, th, m2, st.z, st.sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
    assert f2py_table.last_step_report()["kernel_launches"] == tr.TABLE_LAUNCHES
    rep = f2py_table.table_cache_report()
    assert rep["searched_cells"] == NX * NY and rep["stored_cells"] == 0, rep
    oracles[8].seabreeze_diag(tr.DT_S, 1, p3, u, v, th, m2, st.z, st.sigma, *so, halo=0, bnd=1)
    for a, b, nm in zip(sh, so, tr.NAMES):
        tr.close64(a, b, f"host-model call in between, {nm}")
    r = d.call(3)
    assert r["rep"]["searched_cells"] == band and r["rep"]["stored_cells"] == 0, r["rep"]
    r = d.call(3)
    assert r["rep"]["stored_cells"] == band and r["rep"]["searched_cells"] == 0, r["rep"]
