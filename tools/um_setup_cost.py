"""Cost of the UM-layout coast distance on a curvilinear grid next to the regular-grid one.

    python tools/um_setup_cost.py [--n 50] [--nx 2560 --ny 1920 --halo 15]

times, with HIP events on one torch stream (warm, median of N enqueues):
  * sb_get_dist_um_f64_dev on an nx x ny rotated-pole grid (tests/um_setup_ref.py's "dateline" grid, ~4 km), window
    +-halo x +-halo, the synthetic land/ice mask of bench.py with its ghost cells;
  * sb_get_dist_f64_dev on the regular nx x ny grid of bench.py with kwin = halo.
Prints one JSON line.  Each interval holds the call's launches (two kernels each) and the gap to the event before.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from seabreeze_param_amd import hip, synth  # noqa: E402
import um_setup_ref as ur  # noqa: E402


def _time(fn, n, stream):
    for _ in range(5):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    stream.synchronize()
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--nx", type=int, default=2560)
    ap.add_argument("--ny", type=int, default=1920)
    ap.add_argument("--halo", type=int, default=15)
    a = ap.parse_args()
    nx, ny, h, dt = a.nx, a.ny, a.halo, np.float64
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")

    # UM layout, rotated grid
    st_l = synth.static_fields(nx + 2 * h, ny + 2 * h, dt)
    lat, lon = ur.grid_named("dateline", nx, ny, dt, dlon=0.036, dlat=0.036)
    coast_l = ctx.get_edges_um(st_l.landfrac, st_l.icefrac, h, h)
    lf = np.ascontiguousarray(st_l.landfrac[h:h + ny, h:h + nx])
    d_co, d_lf, d_la, d_lo = dev(coast_l), dev(lf), dev(lat), dev(lon)
    d_cd = torch.zeros_like(d_co)

    # regular grid, as bench.py's
    st = synth.static_fields(nx, ny, dt)
    coast = ctx.get_edges(st.landfrac, st.icefrac)
    r_co, r_lf, r_cd = dev(coast), dev(st.landfrac), torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    s = torch.cuda.Stream()
    sh = s.cuda_stream
    um = lambda: ctx.get_dist_um_dev(dt, nx, ny, h, h, d_co.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(), d_lo.data_ptr(),
                                     d_cd.data_ptr(), maxdist=180.0, stream=sh)
    reg = lambda: ctx.get_dist_dev(dt, nx, ny, r_co.data_ptr(), r_lf.data_ptr(), st.lon, st.lat, r_cd.data_ptr(),
                                   maxdist=180.0, kwin=h, stream=sh)
    with torch.cuda.stream(s):
        t_um = _time(um, a.n, s)
        t_reg = _time(reg, a.n, s)
    cd = d_cd.cpu().numpy()[h:h + ny, h:h + nx]
    out = dict(tool="um_setup_cost", nx=nx, ny=ny, halo=h, dtype="f64",
               coast_cells=int(np.count_nonzero(coast_l)), reached_frac=float(np.mean(cd < 12000.0)),
               get_dist_um_dev=t_um, get_dist_dev_regular=t_reg, ratio=t_um["median_us"] / t_reg["median_us"])
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
