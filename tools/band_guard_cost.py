"""Cost of the guard for missing and non-finite temperatures in a band step (sb_set_nonfinite_guard_bands beside
sb_set_nonfinite_guard).

    python tools/band_guard_cost.py [--nx 2560 --ny-band 240 --ny-full 1920 --nz 56 --halo 16] [--n 50] [--parts off,clean,one]
                                    [--out FILE --key NAME]     (parts: off,clean,one,gath_off,gath_clean,gath_one)
    python tools/band_guard_cost.py --check FILE

One band of eight of the benchmark's grid and mask (as tools/band_step_cost.py cuts it: 240 rows with coast in them, real
neighbouring rows in the ghost rows of the static fields), fp64, ghost width 16, the default contrast kernel (k_strip), a
one-rank communicator: sb_band_seabreeze_diag_f64_dev on device-resident inputs -- the launches, streams, events and joins a
multi-rank step issues, without the wire.  All parts in one process, each the median of N warm steps between two HIP events
on one torch stream, in us:

  off     both switches off: what every band step enqueued before the switch existed
  clean   both switches on, no bad cell: theta gets the whole swap_bounds (one fill launch), k_guard_bits reads theta and z,
          the other three launches leave at once
  one     both switches on, one NaN in theta at a coast cell
  gath_*  the same three as ONE-SEQUENCE calls with gathered moments (sb_seabreeze_diag_f64_dev, SB_BND_HALO on the same frame,
          sb_use_gathered_moments with this band's own moments): the geometry is the same with the switch on and off there

The one-rank communicator makes both edges of the band poles.  With the switches off the strip kernel takes theta's rows
beyond them by index arithmetic (the edge row again) and never reads the ghost rows, so band cells whose other class lies in
a neighbour's rows search on and some leave the LDS path (`counters`); with the switches on the frame is read as filled
and those windows end in the ghost rows.  `off` against `clean` therefore compares two geometries in this setup, not the
guard's launches; gath_off against gath_clean does compare those.

`--parts off` alone runs with a library that does not know the switch (SEABREEZE_HIP_LIB: the parent commit's build), so that
`off` can be compared with the parent measured in the same session, the two alternating, one process each, three times.
`--check FILE` holds the bound on that comparison: every this_build_off_run* of FILE lies within the range of its
parent_run* widened by 3 % -- the largest ratio profiles/guard_cost.json shows between two builds whose kernels are identical
(1.029) -- and writes the verdict into FILE; exit status 1 if not.
u and v are uniform random numbers.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDEN = 1.03


def check(path):
    allres = json.load(open(path))
    parent = [v["off"]["us"] for k, v in sorted(allres.items()) if k.startswith("parent_run")]
    mine = [v["off"]["us"] for k, v in sorted(allres.items()) if k.startswith("this_build_off_run")]
    assert len(parent) >= 3 and len(mine) >= 3, "three runs of each library"
    lo, hi = min(parent) / WIDEN, max(parent) * WIDEN
    ok = all(lo <= x <= hi for x in mine)
    allres["off_check"] = dict(parent_us=parent, this_build_us=mine, widen=WIDEN, range_us=[lo, hi], ok=ok)
    with open(path, "w") as f:
        json.dump(allres, f, indent=1)
        f.write("\n")
    print(json.dumps(allres["off_check"]))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=2560)
    ap.add_argument("--ny-band", type=int, default=240)
    ap.add_argument("--ny-full", type=int, default=1920)
    ap.add_argument("--nz", type=int, default=56)
    ap.add_argument("--halo", type=int, default=16)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--parts", default="off,clean,one,gath_off,gath_clean,gath_one")
    ap.add_argument("--out", default="")
    ap.add_argument("--key", default="")
    ap.add_argument("--check", default="")
    a = ap.parse_args()
    if a.check:
        return check(a.check)

    import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)
    sys.path.insert(0, ROOT)
    from seabreeze_param_amd import hip, synth

    nx, nyb, nyf, nz, h, dt = a.nx, a.ny_band, a.ny_full, a.nz, a.halo, np.float64
    parts = a.parts.split(",")
    ctx = hip.Context(0)
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    st = synth.static_fields(nx, nyf, dt)
    coast = ctx.get_edges(st.landfrac, st.icefrac)
    cdist = ctx.get_dist(coast, st.landfrac, st.lon, st.lat)
    r0 = (nyf - nyb) // 2 + (300 * nyf) // 1920      # a band with coast in it (tools/band_step_cost.py)
    ctx.comm_init(hip.comm_unique_id(), 0, 1)
    ctx.set_search_radius_hint(h)

    def frame(x):
        g = np.concatenate([x[r0 - h:r0 + nyb + h, -h:], x[r0 - h:r0 + nyb + h], x[r0 - h:r0 + nyb + h, :h]], axis=1)
        return torch.from_numpy(np.ascontiguousarray(g)).cuda()

    z, sg, mk = frame(st.z), frame(st.sigma), frame(cdist)
    p3 = torch.from_numpy(synth.pressure_3d(st, nz, dt, rows=(r0, r0 + nyb))).cuda()
    u = torch.rand((nz, nyb, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
    v = torch.rand((nz, nyb, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
    theta = synth.theta_step(st, 2, dt)
    # a land band cell with sea to its east in the middle rows of the band, away from the seam
    band = np.abs(cdist) <= 180.0
    land = cdist >= 0
    cand = np.argwhere(band & land & ~np.roll(land, -1, axis=1))
    cand = cand[(cand[:, 0] > r0 + nyb // 4) & (cand[:, 0] < r0 + 3 * nyb // 4) & (cand[:, 1] > 64) & (cand[:, 1] < nx - 64)]
    cy, cx = (int(c) for c in cand[len(cand) // 2])
    bad = theta.copy()
    bad[cy, cx] = np.nan
    th = {"off": frame(theta), "one": frame(bad)}
    th["clean"] = th["off"]
    gath = torch.zeros(5, dtype=torch.float64, device="cuda")
    ctx.sigma_moments_dev(dt, nx, nyb, h, sg.data_ptr(), gath.data_ptr(), sh)
    state = [torch.zeros((nyb, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()

    def call(part):
        if part.startswith("gath_"):
            ctx.use_gathered_moments(gath.data_ptr(), 1)
            try:
                ctx.seabreeze_diag_dev(dt, 1440.0, 2, nx, nyb, nz, h, hip.SB_BND_HALO, p3.data_ptr(), u.data_ptr(), v.data_ptr(),
                                       th[part[5:]].data_ptr(), mk.data_ptr(), z.data_ptr(), sg.data_ptr(), *[s.data_ptr() for s in state], sh)
            finally:
                ctx.use_gathered_moments(None, 0)
            return
        ctx.band_seabreeze_diag_dev(dt, 1440.0, 2, nx, nyb, nz, h, p3.data_ptr(), u.data_ptr(), v.data_ptr(), th[part].data_ptr(),
                                    mk.data_ptr(), z.data_ptr(), sg.data_ptr(), *[s.data_ptr() for s in state], sh)

    def one_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        ctx.synchronize()
        return e0.elapsed_time(e1)

    def measure(part):
        fn = lambda: call(part)
        first = one_ms(fn)
        n = a.n if first < 20.0 else 10
        for _ in range(4):
            one_ms(fn)
        t = np.array([one_ms(fn) for _ in range(n)]) * 1e3
        out = dict(us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n, first_call_ms=first,
                   counters=ctx.last_counters(), step_report=ctx.last_step_report())
        if hasattr(ctx.lib, "sb_guard_report"):
            out["guard_report"] = ctx.guard_report()
        return out

    res = dict(tool="band_guard_cost", nx=nx, ny_band=nyb, ny_full=nyf, nz=nz, halo=h, dtype="f64", library=os.path.basename(hip.LIB_PATH),
               band_cells=int(band[r0:r0 + nyb].sum()), bad_cell=[cy - r0, cx])
    for part in parts:
        on = not part.endswith("off")
        if on:
            ctx.set_nonfinite_guard(True)
            ctx.set_nonfinite_guard_bands(True)
        res[part] = measure(part)
        if on:
            ctx.set_nonfinite_guard(False)
            ctx.set_nonfinite_guard_bands(False)
    print(json.dumps(res))
    if a.out:
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.key or "this_build"] = res
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1)
            f.write("\n")
    ctx.comm_finalize()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
