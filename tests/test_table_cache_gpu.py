"""The window cache of the table contrast (sb_set_table_window_cache, sb_table_kernels.hip): a table
call that searches leaves every band cell's window (radius, land-side count) in plane W; while k_scan finds both bit planes
standing, later calls neither build nor read the count table.  ref: generic/sea_breeze_diag.f90:188-216.

Everything goes through the C ABI; the device-pointer entry point unless a test says otherwise (arrays that keep their
address, as a host model's do).  Two yardsticks:
  * the CPU oracle (oracle/sb_oracle.f90) on the same inputs and carried state: fp64 under table_ref.close64, fp32 under
    oracle/fp32_criterion.py;
  * the same sequence of table calls with the switch off, on state arrays of its own: equal as integer views, NaN payloads
    included.  tests/test_table_contrast_gpu.py and tests/test_table_shapes_gpu.py hold that path to the oracle.
The report (sb_table_cache_report) says which calls searched: `searched_cells` == band cells on a fill, `stored_cells` ==
the band cells the tables answer on every other call.  Input families: those the existing table tests assert on the
oracle (table_ref.inputs, block_land, reach_land, big_land).  Six launches per call, switch on or off.
"""
import types

import numpy as np
import pytest
import torch  # before the library is loaded: one HIP runtime (seabreeze_param_amd/hip.py)

import table_ref as tr
from oracle import fp32_criterion as crit
from seabreeze_param_amd import hip, synth
from test_table_contrast_gpu import HBIG, _cut, framed  # noqa: F401  (the framed block case, a module-scoped fixture)

pytestmark = pytest.mark.gpu

NX, NY, W = tr.BLOCK
f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


@pytest.fixture
def cached(hipctx):
    hipctx.set_table_contrast(True)
    hipctx.set_table_window_cache(True)
    yield hipctx
    hipctx.set_table_window_cache(False)
    hipctx.set_table_contrast(False)
    hipctx.set_static_sigma(False)
    hipctx.set_search_radius_hint(16)


def _land(dx=0, dy=0):
    return tr.block_land(NX, NY, W, NX, dx=dx, dy=dy)


@pytest.fixture(scope="module")
def block():
    """the block grid, seven steps, and the two coasts of test_coast_that_moves"""
    st, p, per, m1 = tr.inputs(NX, NY, _land(), np.float64, steps=range(1, 8))
    m2 = tr.mask_of(_land(dx=7, dy=3), np.float64)
    assert not np.array_equal(m1, m2)
    return st, p, per, m1, m2


def _oracle(oracle, st, p, per, seq, halo=0, bnd=1):
    """the fp64 oracle from zero state over seq = [(tn, mask)]: per call (state, largest radius), never modified"""
    ny, nx = p.shape[1:]
    so = tr.zeros(4, np.float64, ny, nx)
    out = []
    for tn, mask in seq:
        th, u, v = per[tn]
        oracle.seabreeze_diag(tr.DT_S, tn, f8(p), f8(u), f8(v), f8(th), f8(mask), f8(st.z), f8(st.sigma), *so, halo=halo, bnd=bnd)
        out.append(([a.copy() for a in so], oracle.last_nn_max))
        for a in out[-1][0]:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def moved_ref(oracles, block):
    """stand, stand, stand, move, stand, move back, stand"""
    st, p, per, m1, m2 = block
    ref = _oracle(oracles[8], st, p, per, [(1, m1), (2, m1), (3, m1), (4, m2), (5, m2), (6, m1), (7, m1)])
    assert ref[0][1] == 40 and not np.isnan(ref[0][0][2]).any() and np.count_nonzero(ref[0][0][3]) > 0
    return ref


@pytest.fixture(scope="module")
def inval_ref(oracles, block):
    """M1, then M2 twice"""
    st, p, per, m1, m2 = block
    return _oracle(oracles[8], st, p, per, [(1, m1), (2, m2), (3, m2)])


class Dev:
    """device copies of a case's inputs and a state of its own; one call -> what the call left"""

    def __init__(self, ctx, st, p, per, halo=0, bnd=hip.SB_BND_GLOBAL):
        self.torch, self.ctx, self.halo, self.bnd = torch, ctx, halo, bnd
        self.dt = p.dtype
        self.nz, self.ny, self.nx = p.shape
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=self.dt)).cuda()
        self.p, self.z, self.sg = up(p), up(st.z), up(st.sigma)
        self.per = {tn: tuple(up(a) for a in v) for tn, v in per.items()}
        self.mask = None
        self.state = [torch.zeros((self.ny, self.nx), dtype=self.p.dtype, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()

    def set_mask(self, mask):
        """same array, new content"""
        m = self.torch.from_numpy(np.ascontiguousarray(mask, dtype=self.dt))
        if self.mask is None:
            self.mask = m.cuda()
        else:
            self.mask.copy_(m)
        self.torch.cuda.synchronize()

    def call(self, tn, mask=None):
        if mask is not None:
            self.set_mask(mask)
        th, u, v = self.per[tn]
        self.ctx.seabreeze_diag_dev(self.dt, tr.DT_S, tn, self.nx, self.ny, self.nz, self.halo, self.bnd, self.p.data_ptr(),
                                    u.data_ptr(), v.data_ptr(), th.data_ptr(), self.mask.data_ptr(), self.z.data_ptr(),
                                    self.sg.data_ptr(), *[s.data_ptr() for s in self.state],
                                    stream=hip.torch_stream_handle(torch))
        self.torch.cuda.synchronize()
        return _left(self.ctx, [s.cpu().numpy() for s in self.state])


def _left(ctx, state):
    out = dict(state=state, c=ctx.last_counters(), rep=ctx.table_cache_report(), launches=ctx.last_step_report()["kernel_launches"])
    assert out["launches"] == tr.TABLE_LAUNCHES, out["launches"]
    return out


def _assert_fill(r, fills=None):
    rep, band = r["rep"], r["c"]["band_cells"]
    assert rep["searched_cells"] == band > 0 and rep["stored_cells"] == 0, (rep, band)
    assert fills is None or rep["fills"] == fills, rep


def _assert_stored(r, fills=None, fallback=0):
    rep, band = r["rep"], r["c"]["band_cells"]
    assert rep["stored_cells"] == band - fallback and rep["searched_cells"] == 0 and band > 0, (rep, band)
    assert fills is None or rep["fills"] == fills, rep


def _assert_close(r, ref, what):
    for a, b, nm in zip(r["state"], ref, tr.NAMES):
        tr.close64(a, b, f"{what} {nm}")


def _assert_same_bits(r, twin, what):
    for a, b, nm in zip(r["state"], twin["state"], tr.NAMES):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.itemsize == 8 else np.int32),
                                                     b.view(np.int64 if b.itemsize == 8 else np.int32)), f"{what} {nm}"
    assert r["c"] == twin["c"], (what, r["c"], twin["c"])


def _twin(ctx, make, seq):
    """the sequence with the cache switched off, on a state of its own"""
    ctx.set_table_window_cache(False)
    d = make()
    out = [d.call(tn, mask) for tn, mask in seq]
    assert all(r["rep"]["stored_cells"] == 0 and r["rep"]["searched_cells"] == 0 for r in out)
    ctx.set_table_window_cache(True)
    return out


# ---- 1: the coast stands

def test_block_grid_fp64(cached, block, moved_ref):
    """tn = 1 searches and stores, tn = 2, 3 read the stored windows: the oracle every step, radii up to 40 from W."""
    st, p, per, m1, _ = block
    d = Dev(cached, st, p, per)
    for i, tn in enumerate((1, 2, 3)):
        r = d.call(tn, m1 if tn == 1 else None)
        _assert_close(r, moved_ref[i][0], f"tn={tn}")
        assert r["c"]["global_path_cells"] == 0 and r["c"]["one_class_cells"] == 0 and r["c"]["band_cells"] == NX * NY, r["c"]
        assert r["c"]["max_radius"] == moved_ref[i][1] == 40, r["c"]
        if tn == 1:
            _assert_fill(r, fills=1)
        else:
            _assert_stored(r, fills=1)
        assert r["rep"]["calls"] == tn


# ---- 2: the coast moves

def test_coast_that_moves(cached, block, moved_ref):
    """Same array, new content: k_scan finds the planes changed, the call searches again and stores; back likewise."""
    st, p, per, m1, m2 = block
    d = Dev(cached, st, p, per)
    seq = [(1, m1, True), (2, None, False), (3, None, False), (4, m2, True), (5, None, False), (6, m1, True), (7, None, False)]
    fills = 0
    for i, (tn, mask, fill) in enumerate(seq):
        r = d.call(tn, mask)
        fills += fill
        (_assert_fill if fill else _assert_stored)(r, fills=fills)
        _assert_close(r, moved_ref[i][0], f"call {tn}")
        assert r["c"]["global_path_cells"] == 0 and r["c"]["max_radius"] == moved_ref[i][1], (r["c"], moved_ref[i][1])


# ---- 3: what only the host knows

@pytest.mark.parametrize("other", ["table_contrast_off", "wrapper_flavour", "other_grid", "cache_off_and_on"])
def test_host_side_invalidation(cached, block, inval_ref, other):
    """A table call with M1, another call that leaves M2's planes behind, a table call with M2: its k_scan sees no change
    (or a change that is not the one that matters), and the windows in W are M1's.  The host has dropped them."""
    st, p, per, m1, m2 = block
    d = Dev(cached, st, p, per)
    r = d.call(1, m1)
    _assert_fill(r)
    _assert_close(r, inval_ref[0][0], "M1")
    if other == "table_contrast_off":
        cached.set_table_contrast(False)
        d.set_mask(m2)
        th, u, v = d.per[2]
        cached.seabreeze_diag_dev(d.dt, tr.DT_S, 2, NX, NY, d.nz, 0, hip.SB_BND_GLOBAL, d.p.data_ptr(), u.data_ptr(), v.data_ptr(),
                                  th.data_ptr(), d.mask.data_ptr(), d.z.data_ptr(), d.sg.data_ptr(), *[s.data_ptr() for s in d.state],
                                  stream=hip.torch_stream_handle(torch))
        d.torch.cuda.synchronize()
        assert cached.last_step_report()["kernel_launches"] < tr.TABLE_LAUNCHES
        rep = cached.table_cache_report()
        assert rep["stored_cells"] == 0 and rep["searched_cells"] == 0, rep
        cached.set_table_contrast(True)
        nxt = 3
    elif other == "cache_off_and_on":
        cached.set_table_window_cache(False)
        r = d.call(2, m2)
        assert r["rep"]["stored_cells"] == 0 and r["rep"]["searched_cells"] == 0, r["rep"]
        _assert_close(r, inval_ref[1][0], "M2, cache off")
        cached.set_table_window_cache(True)
        nxt = 3
    elif other == "wrapper_flavour":
        nz = 3
        w = tr.zeros(3, np.float64, NY, NX)
        u, v = synth.wind_step(st, nz, 1, np.float64)
        cached.diag(1, synth.pressure_1d(nz, np.float64), st.z, st.sigma, per[1][0], v, u, m2, *w)
        assert cached.last_step_report()["kernel_launches"] < tr.TABLE_LAUNCHES
        nxt = 2
    else:
        nx, ny = 64, 40
        st2, p2, per2, mk = tr.inputs(nx, ny, tr.stripes_land(nx, ny), np.float64, steps=(1,))
        r = Dev(cached, st2, p2, per2).call(1, mk)
        _assert_fill(r)
        nxt = 2
    for tn in range(nxt, 4):
        r = d.call(tn, m2)
        (_assert_fill if tn == nxt else _assert_stored)(r)
        _assert_close(r, inval_ref[tn - 1][0], f"{other}: M2, tn={tn}")
        assert r["c"]["global_path_cells"] == 0 and r["c"]["max_radius"] == inval_ref[tn - 1][1], r["c"]


# ---- 4: cells the tables do not answer

@pytest.mark.parametrize("w, radius, fallback_columns", [(255, 128, 1), (253, 127, 0)])
def test_fallback_cells_stay_fallback(cached, w, radius, fallback_columns):
    """The reach cases of tests/test_table_shapes_gpu.py: at 128 cells from the sea one column takes the global-memory
    search, on the fill and on every call after it (W holds 0 there: t0 changes, the search runs again); at 127 the radius
    comes from a stored window."""
    nx, ny = tr.REACH_GRID
    st, p, per, mask = tr.inputs(nx, ny, tr.reach_land(w), np.float64, steps=(1, 2, 3))
    seq = [(1, mask), (2, None), (3, None)]
    twin = _twin(cached, lambda: Dev(cached, st, p, per), [(1, mask), (2, mask), (3, mask)])
    d = Dev(cached, st, p, per)
    for (tn, m), t in zip(seq, twin):
        r = d.call(tn, m)
        _assert_same_bits(r, t, f"reach w={w} tn={tn}")
        assert r["c"]["global_path_cells"] == fallback_columns * ny and r["c"]["one_class_cells"] == 0, r["c"]
        assert r["c"]["max_radius"] == radius and r["c"]["band_cells"] == nx * ny, r["c"]
        if tn == 1:
            _assert_fill(r)
        else:
            _assert_stored(r, fallback=fallback_columns * ny)


def test_one_class_grid(cached):
    """All land (test_fallback_one_class_grid): every band cell NaN and counted in every call, none answered from W."""
    nx, ny = 64, 40
    st, p, per, _ = tr.inputs(nx, ny, np.ones((ny, nx), bool), np.float64, steps=(1, 2, 3))
    mask = np.full((ny, nx), 100.0)
    d = Dev(cached, st, p, per)
    for tn in (1, 2, 3):
        r = d.call(tn, mask if tn == 1 else None)
        assert np.isnan(r["state"][2]).all()
        assert r["c"]["global_path_cells"] == r["c"]["one_class_cells"] == nx * ny, r["c"]
        assert r["rep"]["stored_cells"] == 0 and r["rep"]["searched_cells"] == (nx * ny if tn == 1 else 0), r["rep"]
        assert r["rep"]["fills"] == 1


# ---- 5: SB_BND_HALO, the UM entry point

def test_halo_frame(cached, framed):
    """8 ghost cells: cells whose square would leave the frame find one class only -- NaN, counted, W = 0 -- on the fill
    and on the stored calls alike; the others from W.  The same bits as with the cache off."""
    h = 8
    st, p, mask, steps = framed
    cut = lambda a: _cut(a, h)
    S = types.SimpleNamespace(z=cut(st.z), sigma=cut(st.sigma))
    per = {tn: (cut(th), u, v) for tn, (th, u, v) in steps.items()}
    make = lambda: Dev(cached, S, p, per, halo=h, bnd=hip.SB_BND_HALO)
    seq = [(1, cut(mask)), (2, None), (1, None)]
    twin = _twin(cached, make, [(tn, cut(mask)) for tn, _ in seq])
    d = make()
    n_nan = None
    for (tn, m), t in zip(seq, twin):
        r = d.call(tn, m)
        _assert_same_bits(r, t, f"halo tn={tn}")
        nan = int(np.isnan(r["state"][2]).sum())
        n_nan = nan if n_nan is None else n_nan
        assert 0 < nan == n_nan < NX * NY and r["c"]["one_class_cells"] == nan == r["c"]["global_path_cells"], (r["c"], nan)
    _assert_stored(r, fills=1, fallback=n_nan)


def test_um_entry_point(cached, framed):
    """sb_seabreeze_diag_um_f64 (host pointers): theta, z, sigma with 4 ghost cells, mask with 8."""
    hs, hl = 4, 8
    flags = hip.SB_UM_THETA_TO_T0 | hip.SB_UM_LEVEL_WALK
    st, p, mask, steps = framed
    z_s, sg_s, mask_l = _cut(st.z, hs), _cut(st.sigma, hs), _cut(mask, hl)

    def run():
        sh = tr.zeros(4, np.float64, NY, NX)
        out = []
        for tn in (1, 2, 1):
            th, u, v = steps[tn]
            assert cached.seabreeze_diag_um(tr.DT_S, tn, p, u, v, _cut(th, hs).copy(), z_s, sg_s, mask_l, *sh, halo_s=hs, halo_l=hl,
                                            flags=flags) == 0
            out.append(_left(cached, [a.copy() for a in sh]))
        return out
    cached.set_table_window_cache(False)
    twin = run()
    cached.set_table_window_cache(True)
    got = run()
    nan = int(np.isnan(got[0]["state"][2]).sum())
    assert 0 < nan < NX * NY
    for i, (r, t) in enumerate(zip(got, twin)):
        _assert_same_bits(r, t, f"UM call {i}")
        assert r["c"]["one_class_cells"] == nan
        if i == 0:
            _assert_fill(r)
        else:
            _assert_stored(r, fills=1, fallback=nan)


# ---- 6: single precision

def test_fp32_block_grid_against_the_fp64_oracle(cached, oracles):
    dt = np.float32
    st, p, per, mask = tr.inputs(NX, NY, _land(), dt, steps=(1, 2, 3))
    d = Dev(cached, st, p, per)
    so = tr.zeros(4, np.float64, NY, NX)
    band = np.ones((NY, NX), bool)                           # no cell is masked
    res = []
    for tn in (1, 2, 3):
        th, u, v = per[tn]
        gp, op = [s.cpu().numpy() for s in d.state], [a.copy() for a in so]
        oracles[8].seabreeze_diag(tr.DT_S, tn, f8(p), f8(u), f8(v), f8(th), f8(mask), f8(st.z), f8(st.sigma), *so, halo=0, bnd=1)
        r = d.call(tn, mask if tn == 1 else None)
        res.append(crit.check_step(tn, gp, r["state"], op, so, band, timestep=tr.DT_S))
        (_assert_fill if tn == 1 else _assert_stored)(r, fills=1)
        assert r["c"]["global_path_cells"] == 0 and r["c"]["max_radius"] == oracles[8].last_nn_max == 40, r["c"]
    out = crit.merge(res)
    assert out["ok"], out


# ---- 7: where the passes iterate

def test_big_grid_same_bits_as_the_switch_off(cached):
    """1100 x 900: two row chunks, fifteen row blocks.  Fill, stored, moved coast, stored against the path with the cache
    off: a skipped count table that disturbed the carries of A and L or the block sums, or three kernels that did not
    agree on `fill`, would show here."""
    nx, ny = tr.BIG
    land = tr.big_land()
    st, p, per, m1 = tr.inputs(nx, ny, land, np.float64, steps=(1, 2, 3, 4))
    m2 = tr.mask_of(np.roll(land, (5, 7), axis=(0, 1)), np.float64)
    seq = [(1, m1, True), (2, None, False), (3, m2, True), (4, None, False)]
    make = lambda: Dev(cached, st, p, per)
    twin = _twin(cached, make, [(1, m1), (2, m1), (3, m2), (4, m2)])
    d = make()
    for (tn, m, fill), t in zip(seq, twin):
        r = d.call(tn, m)
        (_assert_fill if fill else _assert_stored)(r)
        _assert_same_bits(r, t, f"big call {tn}")
        assert r["c"]["global_path_cells"] == 0 and r["c"]["band_cells"] == nx * ny and r["c"]["max_radius"] >= 40, r["c"]
    assert r["rep"]["fills"] == 2 and r["rep"]["calls"] == 4


# ---- 8: beside static sigma

def test_with_static_sigma(cached, block, moved_ref):
    """sb_set_static_sigma(1): k_scan stops reading sigma from the second call on and still watches both planes."""
    st, p, per, m1, m2 = block
    cached.set_static_sigma(True)
    d = Dev(cached, st, p, per)
    fills = 0
    for i, (tn, mask, fill) in enumerate([(1, m1, True), (2, None, False), (3, None, False), (4, m2, True), (5, None, False)]):
        r = d.call(tn, mask)
        fills += fill
        (_assert_fill if fill else _assert_stored)(r, fills=fills)
        _assert_close(r, moved_ref[i][0], f"static sigma, call {tn}")
        assert r["c"]["max_radius"] == moved_ref[i][1], r["c"]


# ---- 9: staged copies have no identity, the planes do

def test_host_pointer_entry_point(cached, block, moved_ref):
    st, p, per, m1, m2 = block
    sh = tr.zeros(4, np.float64, NY, NX)
    for i, (tn, mask, fill) in enumerate([(1, m1, True), (2, m1.copy(), False), (3, m1.copy(), False), (4, m2, True), (5, m2.copy(), False)]):
        th, u, v = per[tn]
        cached.seabreeze_diag(tr.DT_S, tn, p, u, v, th, mask, st.z, st.sigma, *sh, halo=0, bnd=hip.SB_BND_GLOBAL)
        r = _left(cached, [a.copy() for a in sh])
        (_assert_fill if fill else _assert_stored)(r)
        _assert_close(r, moved_ref[i][0], f"host pointers, call {tn}")
