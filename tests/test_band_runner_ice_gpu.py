"""BandRunner.setup_mask(follow_ice=True) and BandRunner.update_ice on ONE GPU: the ranks share cuda:0 and exchange over
gloo, as tests/test_band_setup_mp_gpu.py does for setup_mask.  The BITS32 grid and planes of tests/band_ice_cases.py: the
first ice call inside setup_mask, then update_ice for planes 2, 4, 5 and 10.  After each, every rank's mask -- interior AND
ghost rows, the periodic wrap in the ghost columns -- must equal, bit for bit, the rows of the library's whole-grid
get_edges(rule, SB_BND_GLOBAL) + get_dist(kwin) for that plane (a context of its own in the same process); one step after
the last update must equal, bit for bit, the step of a runner that called plain setup_mask with that plane.  A world of 1
takes the whole-grid form (south and north both set, no ghost cells)."""
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


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    diff = a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)
    assert not diff.any(), f"{what}: rows {np.flatnonzero(diff.any(1))[:8]} differ"


def _worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import band_ice_cases as bic
    from band_frames import cuts_of
    from seabreeze_param_amd import hip, synth
    from seabreeze_param_amd.bands import BandRunner, split_rows
    from test_band_setup_gpu import coords
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _, nx, k, halo, heights, _ = bic.CASES[0]
        dt, rule, nz = np.float64, 1, 3
        ny = sum(heights)
        lon, lat = coords(nx, ny, 2, dt)
        land, planes = bic.make(nx, k, cuts_of(heights), dt, 2.3)
        r0, r1 = split_rows(ny, world)[rank]
        whole = hip.Context(0)

        def whole_grid(ci):
            return whole.get_dist(whole.get_edges(land, ci, rule=rule, bnd=hip.SB_BND_GLOBAL), land, lon, lat, maxdist=180.0, kwin=k)

        def check(runner, ci, what):
            ref = whole_grid(ci)
            h = runner.h
            mine = runner.mask.cpu().numpy()
            # (a pole side's ghost rows replicate the edge row: torch's transport fills them so)
            rows = np.clip(np.arange(r0 - h, r1 + h), 0, ny - 1)
            _same_bits(mine, ref[np.ix_(rows, np.arange(-h, nx + h) % nx)], f"rank {rank} {what}")
            return ref

        ctx = hip.Context(0)
        if world > 1:                                             # kwin + 1 > halo: refused before anything is exchanged
            thin = BandRunner(ctx, torch, dist, rank, world, nx, ny, nz, halo=k)
            with pytest.raises(ValueError, match="kwin"):
                thin.setup_mask(land, planes[0], lon, lat, rule=rule, kwin=k, follow_ice=True)
            del thin
        runner = BandRunner(ctx, torch, dist, rank, world, nx, ny, nz, halo=halo)
        with pytest.raises(ValueError):
            runner.update_ice(planes[0])                          # nothing to follow yet
        # this rank's rows only: nothing of the globe but the coordinate vectors reaches the runner
        runner.setup_mask(land[r0:r1].copy(), planes[0][r0:r1].copy(), lon, lat, rule=rule, kwin=k, follow_ice=True)
        first = check(runner, planes[0], "setup_mask(follow_ice=True)")
        addr = runner.mask.data_ptr()
        rep = ctx.band_ice_report()
        assert rep["calls"] == 1 and rep["tiles_marked"] == rep["tiles"] == (r1 - r0) * ((nx + 255) // 256)
        last = None
        for n in (1, 3, 4, 9):
            runner.update_ice(planes[n][r0:r1].copy() if n != 4 else planes[n])      # (either form of the argument)
            last = check(runner, planes[n], f"update_ice, plane {bic.PLANES[n]}")
            assert runner.mask.data_ptr() == addr, "update_ice allocated a new mask frame"
            rep = ctx.band_ice_report()
            assert rep["tiles_marked"] < rep["tiles"] and (n != 1 or rep["tiles_marked"] == 0), (n, rep)
        assert rep["calls"] == 5 and not np.array_equal(first, last)

        # one step on the followed mask against a runner whose mask plain setup_mask made for that plane
        st = synth.static_fields(nx, ny, dt)
        p = synth.pressure_3d(st, nz, dt)
        th = synth.theta_step(st, 1, dt)
        u, v = synth.wind_step(st, nz, 1, dt)
        ctx2 = hip.Context(0)
        plain = BandRunner(ctx2, torch, dist, rank, world, nx, ny, nz, halo=halo)
        plain.setup_mask(land, planes[9], lon, lat, rule=rule, kwin=k)
        _same_bits(plain.mask.cpu().numpy(), runner.mask.cpu().numpy(), f"rank {rank}: the two runners' masks")
        outs = []
        for r in (runner, plain):
            r.upload_static(st.z, st.sigma)
            r.step(5400.0, 1, r.upload_step_inputs(p, u, v, th))
            r.synchronize()
            outs.append([t.cpu().numpy() for t in (r.ws, r.wd, r.thc, r.sb_con)])
        for nm, a, b in zip(("ws", "wd", "thc", "sb_con"), *outs):
            _same_bits(a, b, f"rank {rank} step {nm}")
        assert ctx.last_counters()["band_cells"] > 0
        # a plain setup_mask on the following runner closes the coast again
        runner.setup_mask(land, planes[0], lon, lat, rule=rule, kwin=k)
        check(runner, planes[0], "plain setup_mask after following")
        with pytest.raises(ValueError):
            runner.update_ice(planes[1])
        for c in (ctx, ctx2, whole):
            c.close()
        open(os.path.join(tmpdir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 1])
def test_band_runner_follows_the_ice_on_one_gpu(tmp_path, world):
    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))
