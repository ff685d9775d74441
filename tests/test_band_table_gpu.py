"""The table contrast in band steps (sb_set_table_contrast_bands beside sb_set_table_contrast): the contrast of a latitude
band from summed-area tables over the band's own ghost-celled frame -- radii beyond what the LDS kernels reach, on both
multi-band transports: the torch transport of BandRunner.step (a whole diag call with SB_BND_HALO and gathered moments)
and the native band step (sb_band_seabreeze_diag_*, phases 1 and 2 round the join with the communication stream).

The grid: 160 x 120 cells, three levels, every cell in the coastal band, land the 80 x 80 block of
tests/test_table_contrast_gpu.py -- across the longitude seam, touching row 0.  Sea columns 79 / 80 are 40 cells from the
land in the rows below 80 and row 119 is 40 rows from the block, so every band of a two- or three-way even cut holds cells
of radius exactly 40 (asserted below from a numpy Chebyshev search): a ghost width of 40 is necessary and enough.

Yardstick: the CPU oracle (oracle/sb_oracle.f90) on the whole grid (halo = 0, bnd = 1); in double precision under the
project's rule |a - ref| <= 1e-7 max(|ref|, 1e-2), NaN only where the reference has NaN; in single precision the shared rule
of oracle/fp32_criterion.py against the oracle's fp64 build.

Launch sequences (tests/test_band_table_plan.py): the gathered call SCAN PREP WIND MERGE TABLE_ROWS
TABLE_COLS CONTRAST, seven launches, six where static sigma lets the scalars stand; the native band step the ghost fill of
theta, SCAN PREP WIND | join | MERGE TABLE_ROWS TABLE_COLS CONTRAST, eight and seven.
"""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu

NX, NY, NZ, W, HALO = 160, 120, 3, 80, 40
DT_S = 7200.0
STEPS = (1, 2, 3)
NAMES = ("ws", "wd", "thc", "sb_con")
GATHERED_LAUNCHES = 7       # SCAN PREP WIND MERGE TABLE_ROWS TABLE_COLS CONTRAST
BAND_LAUNCHES = 1 + 3 + 4   # the ghost fill of theta | SCAN PREP WIND | MERGE TABLE_ROWS TABLE_COLS CONTRAST
TILE_BAND_LAUNCHES = 1 + 3 + 1      # without the tables (fp64, radius hint beyond 16: the tile kernel): fill | SCAN PREP WIND | CONTRAST
TABLE_LAUNCHES = 6          # a whole single-domain table call: SCAN PREP TABLE_ROWS TABLE_COLS CONTRAST WIND
f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _radius(land):
    """per cell: the smallest Chebyshev radius whose square holds both classes under the whole-grid rule (longitude
    periodic, latitude clamped: a row beyond a pole is the edge row again) -- plain numpy, no library code"""
    ny, nx = land.shape
    nn = np.zeros((ny, nx), np.int64)
    for r in range(1, max(nx, ny)):
        rows = np.clip(np.arange(-r, ny + r), 0, ny - 1)
        cols = np.arange(-r, nx + r) % nx
        P = np.pad(np.cumsum(np.cumsum(land[np.ix_(rows, cols)].astype(np.int64), axis=0), axis=1), ((1, 0), (1, 0)))
        k = 2 * r + 1
        cnt = P[k:, k:] - P[:-k, k:] - P[k:, :-k] + P[:-k, :-k]
        hit = (nn == 0) & (cnt > 0) & (cnt < k * k)
        nn[hit] = r
        if nn.all():
            break
    return nn


def _inputs(dt):
    """-> (st, p, {tn: (theta, u, v)}, mask, land) of the grid in the working precision"""
    import table_ref as tr
    from seabreeze_param_amd import synth
    st = synth.static_fields(NX, NY, dt)
    p = synth.pressure_3d(st, NZ, dt)
    per = {tn: (synth.theta_step(st, tn, dt),) + tuple(synth.wind_step(st, NZ, tn, dt)) for tn in STEPS}
    land = tr.block_land(NX, NY, W, NX)
    return st, p, per, tr.mask_of(land, dt), land


def _oracle_steps(orc, st, p, per, mask):
    """the fp64 oracle on the whole grid: the state after every step; the grid's properties the tests rest on"""
    so = [np.zeros((NY, NX)) for _ in range(4)]
    out = {}
    for tn in STEPS:
        th, u, v = per[tn]
        orc.seabreeze_diag(DT_S, tn, f8(p), f8(u), f8(v), f8(th), f8(mask), f8(st.z), f8(st.sigma), *so, halo=0, bnd=1)
        assert orc.last_nn_max == 40, orc.last_nn_max
        assert not np.isnan(so[2]).any()
        assert all(np.count_nonzero(so[3][r:r + 40]) >= 4300 for r in (0, 40, 80)), [np.count_nonzero(so[3][r:r + 40]) for r in (0, 40, 80)]
        assert np.min(np.abs(np.abs(so[2]) - 0.75)) > 1e-6
        out[tn] = [a.copy() for a in so]
    return out


def _close64(a, b, what):
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs"
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), 1e-2)
    d[np.isnan(b)] = 0.0
    assert d.max() < 1e-7, f"{what}: rel err {d.max()}"


def test_every_band_holds_radius_40():
    """the inputs, not on trust: every band of the two- and the three-way even cut has cells of radius exactly 40, none beyond"""
    from seabreeze_param_amd.bands import split_rows
    _, _, _, _, land = _inputs(np.float64)
    nn = _radius(land)
    assert nn.max() == 40 and nn.min() >= 1
    for world in (2, 3):
        for r0, r1 in split_rows(NY, world):
            assert nn[r0:r1].max() == 40, (world, r0, r1, nn[r0:r1].max())
    assert split_rows(NY, 3)[0] == (0, 40)               # bands of 40 rows: not thinner than the ghost width


# ---- the torch transport: real bands over gloo on one GPU ------------------------------------------------------------
def _worker(rank, world, port, tmpdir, static_sigma, single):
    sys.path.insert(0, ROOT)
    from oracle import fp32_criterion as crit
    from oracle.pyoracle import Oracle
    from seabreeze_param_amd import hip
    from seabreeze_param_amd.bands import BandRunner, split_rows
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dt = np.float32 if single else np.float64
        st, p, per, mask, _ = _inputs(dt)
        ref = _oracle_steps(Oracle(8), st, p, per, mask)
        ctx = hip.Context(0)
        runner = BandRunner(ctx, torch, dist, rank, world, NX, NY, NZ, halo=HALO, dtype=dt, static_sigma=static_sigma,
                            table_contrast=True)
        runner.upload_static(st.z, st.sigma, mask)
        r0, r1 = split_rows(NY, world)[rank]
        state = (runner.ws, runner.wd, runner.thc, runner.sb_con)
        prev_ref = [np.zeros((NY, NX)) for _ in range(4)]
        checks = []
        for tn in STEPS:
            th, u, v = per[tn]
            s = runner.upload_step_inputs(p, u, v, th)
            before = [t.cpu().numpy().copy() for t in state]
            runner.step(DT_S, tn, s)
            runner.synchronize()
            got = [t.cpu().numpy().copy() for t in state]
            c, launches = ctx.last_counters(), ctx.last_step_report()["kernel_launches"]
            if single:
                checks.append(crit.check_step(tn, before, got, [a[r0:r1].copy() for a in prev_ref], [a[r0:r1] for a in ref[tn]],
                                              np.ones((r1 - r0, NX), bool), timestep=DT_S))
            else:
                for nm, a, b in zip(NAMES, got, ref[tn]):
                    _close64(a, b[r0:r1], f"rank {rank} step {tn} {nm}")
            assert c["global_path_cells"] == 0 and c["one_class_cells"] == 0 and c["max_radius"] == 40, (rank, tn, c)
            assert c["band_cells"] == (r1 - r0) * NX, (rank, tn, c)
            want = GATHERED_LAUNCHES - (1 if static_sigma and tn > STEPS[0] else 0)      # static sigma: no MERGE from step 2 on
            assert launches == want, (rank, tn, launches, want)
            prev_ref = ref[tn]
        if single:
            res = crit.merge(checks)
            assert res["ok"], (rank, res)
        ctx.close()
        open(os.path.join(tmpdir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,static_sigma", [(2, False), (3, False), (2, True)], ids=["world2", "world3", "world2-static-sigma"])
def test_torch_transport_real_bands(tmp_path, world, static_sigma):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), static_sigma, False), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


def test_torch_transport_single_precision(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), False, True), nprocs=2, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(2))


# ---- the native band step on a one-rank communicator -----------------------------------------------------------------
def _framed(core, h):
    """the whole-grid rule as ghost cells: poles replicate, longitude wraps"""
    ny, nx = core.shape
    return np.ascontiguousarray(core[np.ix_(np.clip(np.arange(-h, ny + h), 0, ny - 1), np.arange(-h, nx + h) % nx)])


def _theta_frame(th, h):
    """theta's interior inside a frame of NaN: the band step fills its ghost cells itself"""
    f = np.full((NY + 2 * h, NX + 2 * h), np.nan)
    f[h:h + NY, h:h + NX] = th
    return f


class _Band:
    """one band that owns the globe, on a one-rank communicator: static frames on the device, fresh state per run"""

    def __init__(self, h):
        from seabreeze_param_amd import hip
        self.h = h
        self.st, self.p, self.per, self.mask, _ = _inputs(np.float64)
        self.ctx = hip.Context(0)
        self.ctx.comm_init(hip.comm_unique_id(), 0, 1)
        self.ctx.set_search_radius_hint(HALO)
        self.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.z, self.sg, self.mk = (self.dev(_framed(a, h)) for a in (self.st.z, self.st.sigma, self.mask))
        self.pd = self.dev(self.p)
        self.uvd = {tn: (self.dev(u), self.dev(v)) for tn, (_, u, v) in self.per.items()}
        torch.cuda.synchronize()

    def run(self):
        """tn = 1, 2, 3 from zero state -> per step (state, counters, step report)"""
        ctx, h = self.ctx, self.h
        state = [torch.zeros((NY, NX), dtype=torch.float64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        out = {}
        for tn in STEPS:
            thf = self.dev(_theta_frame(self.per[tn][0], h))
            torch.cuda.synchronize()
            ud, vd = self.uvd[tn]
            ctx.band_seabreeze_diag_dev(np.float64, DT_S, tn, NX, NY, NZ, h, self.pd.data_ptr(), ud.data_ptr(), vd.data_ptr(),
                                        thf.data_ptr(), self.mk.data_ptr(), self.z.data_ptr(), self.sg.data_ptr(),
                                        *[s.data_ptr() for s in state])
            ctx.synchronize()
            out[tn] = ([s.cpu().numpy().copy() for s in state], ctx.last_counters(), ctx.last_step_report())
        return out

    def run_host(self):
        """the same through the host-pointer form sb_band_seabreeze_diag_f64"""
        ctx, h = self.ctx, self.h
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        z, sg, mk = (_framed(a, h) for a in (self.st.z, self.st.sigma, self.mask))
        state = [np.zeros((NY, NX)) for _ in range(4)]
        out = {}
        for tn in STEPS:
            th, u, v = self.per[tn]
            thf = _theta_frame(th, h)
            rc = ctx.lib.sb_band_seabreeze_diag_f64(ctx.h, C.c_double(DT_S), C.c_int(tn), C.c_int(NX), C.c_int(NY), C.c_int(NZ), C.c_int(h),
                                                    ptr(self.p), ptr(u), ptr(v), ptr(thf), ptr(mk), ptr(z), ptr(sg),
                                                    *[ptr(s) for s in state], None)
            ctx._chk(rc, "sb_band_seabreeze_diag_f64")
            assert np.array_equal(thf, _framed(th, h))           # its ghost cells came back filled
            out[tn] = ([s.copy() for s in state], ctx.last_counters(), ctx.last_step_report())
        return out

    def tables(self, on, bands):
        self.ctx.set_table_contrast(on)
        self.ctx.set_table_contrast_bands(bands)

    def close(self):
        self.ctx.comm_finalize()
        self.ctx.close()


@pytest.fixture(scope="module")
def ref64(oracles):
    """the fp64 oracle on the whole grid, tn = 1, 2, 3: never modified"""
    st, p, per, mask, _ = _inputs(np.float64)
    out = _oracle_steps(oracles[8], st, p, per, mask)
    for states in out.values():
        for a in states:
            a.setflags(write=False)
    return out


@pytest.fixture
def band():
    b = _Band(HALO)
    yield b
    b.close()


def _report(launches):
    return dict(kernel_launches=launches, rccl_ops=0, rccl_groups=0, d2d_copies=0)


def _assert_table_run(run, ref64, what):
    for tn in STEPS:
        state, c, rep = run[tn]
        for nm, a, b in zip(NAMES, state, ref64[tn]):
            _close64(a, b, f"{what} step {tn} {nm}")
        assert c["global_path_cells"] == 0 and c["one_class_cells"] == 0 and c["max_radius"] == 40, (what, tn, c)
        assert c["band_cells"] == NX * NY
        assert rep == _report(BAND_LAUNCHES), (what, tn, rep)


def test_native_band_step_one_rank(band, ref64):
    """Phases 1 and 2 round the join, theta's ghost cells by the whole swap_bounds on the communication stream; twice from
    fresh state: the same bits (the sums are exact); and through the host-pointer form."""
    band.tables(True, True)
    first = band.run()
    _assert_table_run(first, ref64, "device pointers")
    second = band.run()
    host = band.run_host()
    for tn in STEPS:
        for nm, a, b, c in zip(NAMES, first[tn][0], second[tn][0], host[tn][0]):
            assert np.array_equal(a, b, equal_nan=True), (tn, nm)
            assert np.array_equal(a, c, equal_nan=True), ("host pointers", tn, nm)
        assert second[tn][1] == first[tn][1] and host[tn][1] == first[tn][1]
        assert host[tn][2]["kernel_launches"] == BAND_LAUNCHES


def test_native_band_step_static_sigma(band, ref64):
    """static sigma: from the second step on the scalars stand -- no MERGE"""
    band.tables(True, True)
    band.ctx.set_static_sigma(True)
    run = band.run()
    for tn in STEPS:
        state, c, rep = run[tn]
        for nm, a, b in zip(NAMES, state, ref64[tn]):
            _close64(a, b, f"static sigma step {tn} {nm}")
        assert c["global_path_cells"] == 0 and c["max_radius"] == 40, c
        assert rep == _report(BAND_LAUNCHES - (1 if tn > STEPS[0] else 0)), (tn, rep)


def test_switch_discipline_on_one_context(band, ref64):
    """The band switch alone changes nothing; both on: the tables; off again: today's kernels again.  A whole
    single-domain table call in between keeps its six launches; the window cache never serves a band step."""
    ctx = band.ctx
    st, p, per, mask = band.st, band.p, band.per, band.mask

    def whole_call():
        sh = [np.zeros((NY, NX)) for _ in range(4)]
        th, u, v = per[1]
        ctx.seabreeze_diag(DT_S, 1, p, u, v, th, mask, st.z, st.sigma, *sh, halo=0, bnd=1)
        c = ctx.last_counters()
        for nm, a, b in zip(NAMES, sh, ref64[1]):
            _close64(a, b, f"whole table call {nm}")
        assert ctx.last_step_report()["kernel_launches"] == TABLE_LAUNCHES
        assert c["global_path_cells"] == 0 and c["max_radius"] == 40 and c["band_cells"] == NX * NY, c

    def assert_today(run, what):
        for tn in STEPS:
            state, c, rep = run[tn]
            for nm, a, b in zip(NAMES, state, ref64[tn]):
                _close64(a, b, f"{what} step {tn} {nm}")
            assert c["global_path_cells"] > 0 and c["max_radius"] == 40, (what, tn, c)
            assert rep == _report(TILE_BAND_LAUNCHES), (what, tn, rep)

    band.tables(False, True)                             # the new switch without sb_set_table_contrast: ignored
    off0 = band.run()
    assert_today(off0, "band switch alone")
    band.tables(True, True)
    on = band.run()
    _assert_table_run(on, ref64, "both switches")
    whole_call()
    band.tables(True, False)                             # the new switch off again: a band step ignores sb_set_table_contrast
    off1 = band.run()
    assert_today(off1, "band switch off again")
    whole_call()
    for tn in STEPS:
        for nm, a, b, c in zip(NAMES, on[tn][0], off0[tn][0], off1[tn][0]):
            _close64(a, b, f"on against off, step {tn} {nm}")
            assert np.array_equal(b, c, equal_nan=True), (tn, nm)
    # the window cache: a whole call fills, a table band step neither reads nor writes stored windows and drops them
    band.tables(True, True)
    ctx.set_table_window_cache(True)
    whole_call()
    r = ctx.table_cache_report()
    assert r["fills"] == 1 and r["searched_cells"] == NX * NY and r["stored_cells"] == 0, r
    whole_call()
    r = ctx.table_cache_report()
    assert r["fills"] == 1 and r["stored_cells"] == NX * NY, r          # (the cache works on this grid: the next assertion means something)
    again = band.run()
    r = ctx.table_cache_report()
    assert r["stored_cells"] == 0 and r["searched_cells"] == 0 and r["fills"] == 1, r
    _assert_table_run(again, ref64, "band step with the window cache set")
    whole_call()
    r = ctx.table_cache_report()
    assert r["fills"] == 2 and r["searched_cells"] == NX * NY, r
    ctx.set_table_window_cache(False)


def test_ghost_width_below_the_radius(ref64):
    """halo 24 < 40: a cell whose window leaves the frame takes the global-memory path, bounded by the frame reach, and
    its update runs through the query's own epilogue -- as the tile kernel answers it without the tables."""
    b = _Band(24)
    try:
        b.tables(True, True)
        on = b.run()
        b.tables(False, False)
        off = b.run()
        for tn in STEPS:
            (s_on, c_on, rep_on), (s_off, c_off, rep_off) = on[tn], off[tn]
            assert rep_on == _report(BAND_LAUNCHES) and rep_off == _report(TILE_BAND_LAUNCHES), (rep_on, rep_off)
            assert c_on["global_path_cells"] > 0 and c_off["global_path_cells"] > 0, (c_on, c_off)
            assert c_on["one_class_cells"] == c_off["one_class_cells"], (c_on, c_off)
            assert c_on["band_cells"] == c_off["band_cells"] == NX * NY
            for nm, a, r in zip(NAMES, s_on, s_off):
                _close64(a, r, f"halo 24, on against off, step {tn} {nm}")
            # (cells the frame answers are the whole grid's; the others are NaN in thc, where the oracle never is)
            ok = ~np.isnan(s_on[2])
            assert ok.any() and not ok.all()
            d = np.abs(s_on[2][ok] - ref64[tn][2][ok]) / np.maximum(np.abs(ref64[tn][2][ok]), 1e-2)
            assert d.max() < 1e-7, d.max()
    finally:
        b.close()
