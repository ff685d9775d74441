"""Cost of the guard for missing and non-finite temperatures (sb_set_nonfinite_guard).

    python tools/guard_cost.py [--nx 2560 --ny 1920 --nz 56] [--n 50] [--parts off,clean,one,block] [--out FILE --key NAME]

The benchmark's grid and mask (synthetic coast, the library's own get_edges / get_dist), fp64, no ghost cells, SB_BND_GLOBAL:
sb_seabreeze_diag_f64_dev on device-resident inputs, the default contrast kernel (k_strip, three launches).  All parts in one
process, each the median of N warm calls between two HIP events on one torch stream, in us, with the per-kernel averages of
sb_profile_begin / sb_profile_end over the same number of further calls beside it (the guard's launches lie outside every
timed pair: what they cost shows in the whole call alone):

  off     the switch off: what every call enqueued before the guard existed
  clean   the switch on, no bad cell: k_guard_bits reads theta and z, the other three launches leave at once
  one     the switch on, one NaN in theta at a coast cell
  block   the switch on, a 40 x 40 block of 2.0e20 across the coast

`--parts off` alone runs with a library that does not know the switch (SEABREEZE_HIP_LIB: the parent commit's build), so
that `off` can be stated as a ratio to the parent measured in the same session; repeat both to see their spreads.
u and v are uniform random numbers.
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
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--parts", default="off,clean,one,block")
    ap.add_argument("--out", default="")
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    nx, ny, nz, dt = a.nx, a.ny, a.nz, np.float64
    parts = a.parts.split(",")
    ctx = hip.Context(0)
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")

    st = synth.static_fields(nx, ny, dt)
    coast = ctx.get_edges(st.landfrac, st.icefrac)
    cdist = ctx.get_dist(coast, st.landfrac, st.lon, st.lat)
    band = np.abs(cdist) <= 180.0
    p3 = dev(synth.pressure_3d(st, nz, dt))
    u = torch.rand((nz, ny, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
    v = torch.rand((nz, ny, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
    mask, z, sg = dev(cdist), dev(st.z), dev(st.sigma)
    theta = synth.theta_step(st, 2, dt)
    # a land band cell with sea to its east, in mid-latitudes, away from the seam
    land = cdist >= 0
    cand = np.argwhere(band & land & ~np.roll(land, -1, axis=1))
    cand = cand[(cand[:, 0] > ny // 4) & (cand[:, 0] < 3 * ny // 4) & (cand[:, 1] > 64) & (cand[:, 1] < nx - 64)]
    cy, cx = (int(c) for c in cand[len(cand) // 2])
    th = {"off": theta, "clean": theta, "one": theta.copy(), "block": theta.copy()}
    th["one"][cy, cx] = np.nan
    th["block"][cy - 20:cy + 20, cx - 20:cx + 20] = 2.0e20
    th = {k: dev(x) for k, x in th.items() if k in parts}
    state = [torch.zeros((ny, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()

    def call(part, tn=2):
        ctx.seabreeze_diag_dev(dt, 1440.0, tn, nx, ny, nz, 0, hip.SB_BND_GLOBAL, p3.data_ptr(), u.data_ptr(), v.data_ptr(),
                               th[part].data_ptr(), mask.data_ptr(), z.data_ptr(), sg.data_ptr(), *[s.data_ptr() for s in state],
                               stream=sh)

    def one_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def measure(part):
        fn = lambda: call(part)
        first = one_ms(fn)
        n = a.n if first < 20.0 else 10
        for _ in range(2):
            one_ms(fn)
        t = np.array([one_ms(fn) for _ in range(n)]) * 1e3
        ctx.profile_begin(n)
        for _ in range(n):
            fn()
        stream.synchronize()
        ms, ncalls = ctx.profile_end()
        out = dict(us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n, first_call_ms=first,
                   kernels_us={k: 1e3 * val for k, val in ms.items()}, profiled_calls=ncalls,
                   counters=ctx.last_counters(), step_report=ctx.last_step_report())
        if hasattr(ctx.lib, "sb_guard_report"):
            out["guard_report"] = ctx.guard_report()
        return out

    res = dict(tool="guard_cost", nx=nx, ny=ny, nz=nz, dtype="f64", library=os.path.basename(hip.LIB_PATH), band_cells=int(band.sum()),
               bad_cell=[cy, cx])
    for part in parts:
        if part != "off":
            ctx.set_nonfinite_guard(True)
        res[part] = measure(part)
        if part != "off":
            ctx.set_nonfinite_guard(False)
    print(json.dumps(res))
    if a.out:
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.key or "this_build"] = res
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
