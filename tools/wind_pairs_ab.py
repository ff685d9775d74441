"""k_wind with its paired column walk (sb_set_wind_pairs, the default) against the one-cell walk, in one process.

    python tools/wind_pairs_ab.py [--nx 2560 --ny 1920 --nz 56] [--blocks 5] [--n 20] [--tag NAME --out FILE]

The benchmark's shape and synthetic inputs (bench.py: the synthetic coast through get_edges / get_dist, synth's pressure,
winds and temperatures, double precision), two input sets at different addresses taken in turn (the second swaps u and v
and takes the next step's theta).  The knob alternates on / off in `blocks` blocks; a block is 3 untimed calls and then
`n` profiled ones (sb_profile_begin / sb_profile_end: HIP events around every kernel, averaged over the block's calls).
Per block: k_wind's average, the other kernels', and last_wind_pairs().  Prints one JSON line and, with --out, merges it
into that file under --tag (the build measured: SEABREEZE_HIP_LIB picks an A/B build of SB_WIND_UN_PAIR, see
seabreeze_param_amd/csrc/Makefile).  Run it under a time limit of its own.
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

from seabreeze_param_amd import hip, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=2560)
    ap.add_argument("--ny", type=int, default=1920)
    ap.add_argument("--nz", type=int, default=56)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--tag", default="default")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    nx, ny, nz, dt = a.nx, a.ny, a.nz, np.float64
    ctx = hip.Context(0)
    stream = torch.cuda.Stream()
    st = synth.static_fields(nx, ny, dt)
    cdist = ctx.get_dist(ctx.get_edges(st.landfrac, st.icefrac), st.landfrac, st.lon, st.lat)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
    p = synth.pressure_3d(st, nz, dt)
    u, v = synth.wind_step(st, nz, 1, dt)
    sets = [dict(p=dev(p), u=dev(u), v=dev(v), th=dev(synth.theta_step(st, 1, dt))),
            dict(p=dev(p), u=dev(v), v=dev(u), th=dev(synth.theta_step(st, 2, dt)))]
    del p, u, v
    z, sg, mask = dev(st.z), dev(st.sigma), dev(cdist)
    state = [torch.zeros((ny, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    tn = [0]

    def call():
        tn[0] += 1
        s = sets[tn[0] % len(sets)]
        ctx.seabreeze_diag_dev(dt, 1440.0, tn[0], nx, ny, nz, 0, hip.SB_BND_GLOBAL, s["p"].data_ptr(), s["u"].data_ptr(),
                               s["v"].data_ptr(), s["th"].data_ptr(), mask.data_ptr(), z.data_ptr(), sg.data_ptr(),
                               *[t.data_ptr() for t in state], stream=stream.cuda_stream)

    for _ in range(5):                                   # the first calls make the contrast kernel's stored plan
        call()
    stream.synchronize()
    blocks = []
    for b in range(a.blocks):
        for on in (True, False):
            ctx.set_wind_pairs(on)
            for _ in range(3):
                call()
            stream.synchronize()
            ctx.profile_begin(a.n)
            for _ in range(a.n):
                call()
            ms, ncalls = ctx.profile_end()
            blocks.append(dict(block=b, pairs_knob=on, ran_pairs=ctx.last_wind_pairs(), calls=ncalls,
                               k_wind_us=round(ms["k_wind"] * 1e3, 3), k_scan_us=round(ms["k_scan"] * 1e3, 3),
                               k_thc_us=round(ms["k_thc"] * 1e3, 3)))
    ctx.set_wind_pairs(True)
    on = np.array([b["k_wind_us"] for b in blocks if b["pairs_knob"]])
    off = np.array([b["k_wind_us"] for b in blocks if not b["pairs_knob"]])
    res = dict(tool="wind_pairs_ab", tag=a.tag, lib=os.path.basename(hip.LIB_PATH), nx=nx, ny=ny, nz=nz, dtype="f64",
               input_sets=len(sets), calls_per_block=a.n, band_cells=ctx.last_counters().get("band_cells"), blocks=blocks,
               k_wind_us=dict(pairs=dict(min=float(on.min()), median=float(np.median(on)), max=float(on.max())),
                              one_cell=dict(min=float(off.min()), median=float(np.median(off)), max=float(off.max()))),
               saved_us=float(np.median(off) - np.median(on)))
    print(json.dumps(res))
    if a.out:
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.tag] = res
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
