"""BandRunner.setup_mask on ONE GPU: three processes share cuda:0 and exchange over gloo, as tests/test_bands_gpu.py
does for the band step.  Every rank derives its mask -- coastline and signed coast distance -- from its own rows of the
land and ice fields alone, then runs two steps on it; no rank computes the globe.  The mask rows must be the whole-grid
oracle's (coast exact, which the distance's 'unreached' cells and signs show; distance to 1e-12 in fp64, 2e-6 in fp32:
the tolerances of tests/test_setup_gpu.py), and the step outputs the single-domain oracle's under the rules of
tests/test_bands_gpu.py: 1e-7 relative in fp64, the shared single-precision criterion in fp32."""
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


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _mask_rows_ok(mine, ref, rel, what):
    assert np.array_equal(mine >= 12000.0, ref >= 12000.0), f"{what}: cells without a coast in reach differ"
    assert np.array_equal(np.sign(mine), np.sign(ref)), f"{what}: signs differ"
    e = np.abs(mine - ref) / np.maximum(np.abs(ref), 1.0)
    assert e.max() <= rel, f"{what}: max rel err {e.max()}"


def _worker64(rank, world, port, nx, ny, nz, tmpdir):
    sys.path.insert(0, ROOT)
    from oracle.pyoracle import Oracle
    from seabreeze_param_amd import hip, synth
    from seabreeze_param_amd.bands import BandRunner, split_rows
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        orc = Oracle(8)
        st = synth.static_fields(nx, ny)
        kwin = 5
        coast = orc.get_edges(st.landfrac, st.icefrac, rule=1, bnd=1)
        cdist = orc.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=180.0, kwin=kwin)
        r0, r1 = split_rows(ny, world)[rank]
        # the case is about the cuts: the oracle's field near this band's cuts is not the field of the band's rows alone
        alone = orc.get_dist(orc.get_edges(st.landfrac[r0:r1], st.icefrac[r0:r1], rule=1, bnd=1), st.landfrac[r0:r1],
                             st.lon, st.lat[r0:r1], maxdist=180.0, kwin=kwin)
        assert world == 1 or not np.array_equal(alone, cdist[r0:r1])
        p = synth.pressure_3d(st, nz)
        ctx = hip.Context(0)
        runner = BandRunner(ctx, torch, dist, rank, world, nx, ny, nz, halo=kwin + 1)
        # this rank's rows only: nothing of the globe but the coordinate vectors reaches the runner
        runner.setup_mask(st.landfrac[r0:r1].copy(), st.icefrac[r0:r1].copy(), st.lon, st.lat, rule=1, kwin=kwin)
        h = runner.h
        mine = runner.mask.cpu().numpy()
        _mask_rows_ok(mine[h:h + r1 - r0, h:h + nx], cdist[r0:r1], 1e-12, f"rank {rank} mask")
        # the ghost cells are filled: rows of the neighbours, the periodic wrap
        lo, hi = max(r0 - h, 0), min(r1 + h, ny)
        _mask_rows_ok(mine[h - (r0 - lo):h + (hi - r0), h:h + nx], cdist[lo:hi], 1e-12, f"rank {rank} mask with ghost rows")
        assert np.array_equal(mine[:, :h], mine[:, nx:nx + h]) and np.array_equal(mine[:, nx + h:], mine[:, h:2 * h])
        runner.upload_static(st.z, st.sigma)
        full = [np.zeros((ny, nx)) for _ in range(4)]
        for tn in (1, 2):
            th = synth.theta_step(st, tn)
            u, v = synth.wind_step(st, nz, tn)
            s = runner.upload_step_inputs(p, u, v, th)
            runner.step(7200.0, tn, s)
            ctx.synchronize()
            torch.cuda.synchronize()
            orc.seabreeze_diag(7200.0, tn, p, u, v, th, cdist, st.z, st.sigma, *full, halo=0, bnd=1)
            for nm, got, ref in zip(("ws", "wd", "thc", "sb_con"), (runner.ws, runner.wd, runner.thc, runner.sb_con), full):
                a, b = got.cpu().numpy(), ref[r0:r1]
                err = np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-2))
                assert err < 1e-7, f"rank {rank} step {tn} {nm}: {err}"
        assert ctx.last_counters()["band_cells"] > 0
        ctx.close()
        open(os.path.join(tmpdir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [3, 1], ids=["three-bands", "one-band-whole-grid-entry-points"])
def test_setup_mask_then_steps_fp64(tmp_path, world):
    port = _free_port()
    mp.spawn(_worker64, args=(world, port, 160, 96, 4, str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


def _worker32(rank, world, port, nx, ny, nz, tmpdir):
    """Single precision, kwin = 31: the widest window of the one-word kernels in a frame of 32 ghost cells; the steps are
    judged by the shared single-precision rule against the fp64 oracle."""
    sys.path.insert(0, ROOT)
    from oracle import fp32_criterion as crit
    from oracle.pyoracle import Oracle
    from seabreeze_param_amd import hip, synth
    from seabreeze_param_amd.bands import BandRunner, split_rows
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dt = np.float32
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        orc, orc4 = Oracle(8), Oracle(4)
        st = synth.static_fields(nx, ny, dt)
        kwin = 31
        coast = orc4.get_edges(st.landfrac, st.icefrac, rule=1, bnd=1)
        cd4 = orc4.get_dist(coast, st.landfrac, st.lon, st.lat, maxdist=180.0, kwin=kwin)
        r0, r1 = split_rows(ny, world)[rank]
        p = synth.pressure_3d(st, nz, dt)
        ctx = hip.Context(0)
        runner = BandRunner(ctx, torch, dist, rank, world, nx, ny, nz, halo=kwin + 1, dtype=dt)
        runner.setup_mask(st.landfrac[r0:r1].copy(), st.icefrac[r0:r1].copy(), st.lon, st.lat, rule=1, kwin=kwin)
        h = runner.h
        mine = runner.mask.cpu().numpy()
        assert mine.dtype == dt
        _mask_rows_ok(mine[h:h + r1 - r0, h:h + nx], cd4[r0:r1], 2e-6, f"rank {rank} mask")
        runner.upload_static(st.z, st.sigma)
        # the steps' reference runs in fp64 on the mask the GPU holds (gathered from every rank: the criterion judges the
        # steps, the mask is judged above)
        parts = [None] * world
        dist.all_gather_object(parts, mine[h:h + r1 - r0, h:h + nx].copy())
        cd = np.concatenate(parts)
        full = [np.zeros((ny, nx)) for _ in range(4)]
        band = (np.abs(f8(cd)) <= 180.0)[r0:r1]
        per = []
        for tn in (1, 2):
            th = synth.theta_step(st, tn, dt)
            u, v = synth.wind_step(st, nz, tn, dt)
            s = runner.upload_step_inputs(p, u, v, th)
            gp = [t.cpu().numpy().copy() for t in (runner.ws, runner.wd, runner.thc, runner.sb_con)]
            op = [a[r0:r1].copy() for a in full]
            runner.step(7200.0, tn, s)
            ctx.synchronize()
            torch.cuda.synchronize()
            orc.seabreeze_diag(7200.0, tn, f8(p), f8(u), f8(v), f8(th), f8(cd), f8(st.z), f8(st.sigma), *full, halo=0, bnd=1)
            gn = [t.cpu().numpy().copy() for t in (runner.ws, runner.wd, runner.thc, runner.sb_con)]
            per.append(crit.check_step(tn, gp, gn, op, [a[r0:r1] for a in full], band, timestep=7200.0))
        res = crit.merge(per)
        assert res["ok"], (rank, res)
        ctx.close()
        open(os.path.join(tmpdir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_setup_mask_then_steps_fp32_window_31(tmp_path):
    port = _free_port()
    mp.spawn(_worker32, args=(3, port, 256, 192, 3, str(tmp_path)), nprocs=3, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(3))
