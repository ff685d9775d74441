"""Cost of a stream's ice call (sb_diag_stream_ice_*): what following a moving coast on the device
costs, beside the whole-grid calls it replaces and beside the driver's close-and-reopen.

    python tools/stream_ice_cost.py [--parent-lib PATH] [--rounds 3] [--out profiles/stream_ice_cost.json]

Three parts, each in fresh child processes of this tool (a library is loaded through SEABREEZE_HIP_LIB; a child that
fails or outlives --limit ends the tool: nothing is started on the GPU after a fault or a hang):
  ice     2560 x 1920, fp32 and fp64, on the bench mask (synth.static_fields, window from maxdist = 180 km: k = 15) and on the
          0.0135-degree regional grid of tools/dist_wide_cost.py (k = 113): the HIP-event time of one ice call
          (sb_diag_stream_ice_time: the plane's upload, the clear, the kernels) for an unchanged plane, one cell crossing
          0.4, an ice edge moved by one row over 200 columns, and a plane that changes every tile -- with incremental = 1
          and 0 -- and sb_get_edges_*_dev + sb_get_dist_*_dev on the same inputs (events on a torch stream; no upload in
          that figure: `upload_us` is the plane's pinned upload alone, measured apart, to put beside it).  A variant plane
          alternates with the base plane; both directions are changes of the same size and both are kept.
  driver  seabreezediag.diag at 1024 x 768 x 8 fp32 over 200 steps, the ice edge moving every step and every fourth step,
          with ice_on_device on and off: seconds per step (wall clock over the call, after a warm call).
  parent  sb_get_dist_f64_dev at kwin = 15 (bench grid) and 113 (regional) on this build and on the parent commit's library,
          the libraries taking turns `--rounds` times: this build must lie inside the range of the parent's runs widened
          by 3 % (the margin of profiles/band_guard_cost.json).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 2560, 1920
WIDEN = 1.03


def _grids(np, synth, dt):
    st = synth.static_fields(NX, NY, dt)
    return {"bench_k15": (st.lon.astype(dt), st.lat.astype(dt), st.landfrac.astype(dt), st.icefrac.astype(dt)),
            "regional_k113": ((10.0 + 0.0135 * np.arange(NX)).astype(dt), (60.0 + 0.0135 * np.arange(NY)).astype(dt),
                              st.landfrac.astype(dt), st.icefrac.astype(dt))}


def _variants(np, land, base):
    """the planes an ice call is timed for, each to alternate with `base`"""
    dt = base.dtype
    sea = land == 0
    ys, xs = np.nonzero(sea[200:-200, 300:-300] & (base[200:-200, 300:-300] == 0))
    one = base.copy()
    one[200 + ys[len(ys) // 2], 300 + xs[len(xs) // 2]] = dt.type(0.5)
    edge = base.copy()
    iced = np.nonzero((base > 0.4).any(axis=1))[0]
    row = (iced[iced > NY // 2].min() - 1) if (iced > NY // 2).any() else NY - 50       # the row south of the northern ice
    edge[row, 1000:1200][sea[row, 1000:1200]] = dt.type(0.6)
    every = base.copy()                                          # one more iced cell in every tile and every sixteenth row
    every[8::16, 128::256][sea[8::16, 128::256] & (base[8::16, 128::256] == 0)] = dt.type(0.5)
    return {"unchanged": base, "one_cell": one, "edge_200": edge, "every_tile": every}


def _child_ice(spec):
    import numpy as np
    import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)
    sys.path.insert(0, ROOT)
    from seabreeze_param_amd import hip, synth

    out = {}
    ctx = hip.Context(0)
    s = torch.cuda.Stream()
    med = lambda v: float(np.median(v))
    for dt in (np.float32, np.float64):
        name = "f32" if dt == np.float32 else "f64"
        for grid, (lon, lat, land, base) in _grids(np, synth, dt).items():
            k = hip.dist_window(lon, lat, 180.0)
            res = dict(k=k)
            var = _variants(np, land, base)
            zero = np.zeros_like(land)
            for inc in (1, 0):
                ctx.stream_begin(zero, zero, zero, zero, zero, zero)
                ctx.stream_coast(land, lon, lat, maxdist=180.0, incremental=bool(inc))
                ctx.stream_ice(base)
                first = ctx.stream_ice_time()
                for case, plane in var.items():
                    there, back, marked = [], [], []
                    for _ in range(5):
                        ctx.stream_ice(plane); there.append(1e3 * ctx.stream_ice_time())
                        marked.append(ctx.stream_ice_report()["tiles_marked"])
                        ctx.stream_ice(base); back.append(1e3 * ctx.stream_ice_time())
                    res[f"{case}_inc{inc}"] = dict(us=med(there), runs_us=there, back_us=med(back), tiles_marked=marked[-1])
                res[f"first_call_inc{inc}_us"] = 1e3 * first
                res["tiles"] = ctx.stream_ice_report()["tiles"]
                ctx.stream_end()
            # the calls an ice call replaces, on the same inputs, device-resident, and the upload an ice call holds
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
            d_land, d_cd, d_co = dev(land), dev(zero), dev(zero)
            d_ci = dev(base)
            for case, plane in var.items():
                pin = torch.from_numpy(plane.copy()).pin_memory()
                d_ci.copy_(pin)
                torch.cuda.synchronize()
                t, up = [], []
                with torch.cuda.stream(s):
                    for i in range(7):
                        a, b, c2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                        a.record(s)
                        ctx.get_edges_dev(dt, NX, NY, d_land.data_ptr(), d_ci.data_ptr(), d_co.data_ptr(), stream=s.cuda_stream)
                        ctx.get_dist_dev(dt, NX, NY, d_co.data_ptr(), d_land.data_ptr(), lon, lat, d_cd.data_ptr(), maxdist=180.0,
                                         stream=s.cuda_stream)
                        b.record(s)
                        d_ci.copy_(pin, non_blocking=True)       # the same plane again: what an ice call's upload costs
                        c2.record(s)
                        s.synchronize()
                        if i >= 2:
                            t.append(1e3 * a.elapsed_time(b))
                            up.append(1e3 * b.elapsed_time(c2))
                res[f"{case}_edges_dist_dev"] = dict(us=med(t), runs_us=t)
                if case == "unchanged":
                    res["upload_us"] = med(up)
            out[f"{grid}_{name}"] = res
            del d_land, d_cd, d_co, d_ci, pin
            torch.cuda.empty_cache()
    ctx.close()
    print("RESULT " + json.dumps(out))


class _MovingIce:
    """ci[ts]: a view of a fresh buffer per read, the edge one row further south on odd turns; a turn lasts `every` steps"""

    def __init__(self, np, planes, nt, every):
        self.np, self.planes, self.every = np, planes, every
        self.shape = (nt,) + planes[0].shape

    def __getitem__(self, ts):
        buf = self.np.empty((1,) + self.planes[0].shape, self.np.float32)
        buf[0] = self.planes[(ts // self.every) & 1]
        return buf[0]


def _child_driver(spec):
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "python_wrapper"))
    import seabreezediag as sbd
    from seabreeze_param_amd import synth

    nlon, nlat, nlev, nt = 1024, 768, 8, 200
    st = synth.static_fields(nlon, nlat, np.float32)
    pres = (synth.pressure_1d(nlev, np.float32) / 100.0).astype(np.float32)
    u1, v1 = synth.wind_step(st, nlev, 1, np.float32)
    bc = lambda a: np.broadcast_to(a, (nt,) + a.shape)
    u, v, t = bc(u1), bc(v1), bc(synth.theta_step(st, 1, np.float32))
    sea = st.landfrac == 0
    base = st.icefrac.astype(np.float32)
    iced = np.nonzero((base > 0.4).any(axis=1))[0]
    row = iced[iced > nlat // 2].min() - 1
    moved = base.copy()
    moved[row, 400:600][sea[row, 400:600]] = 0.6
    args = (st.landfrac, st.z, st.sigma, st.lon, st.lat, pres)
    out = {}
    buf = np.zeros((nt, nlat, nlon))                             # (the result array, reused: its page faults are not the driver's)
    for every in (1, 4):
        for on in (True, False):
            kw = dict(timestep=24.0, out=buf, ice_on_device=True) if on else dict(timestep=24.0, out=buf)
            secs = []
            for rep in range(3):                                 # the first is the warm call
                ci = _MovingIce(np, (base, moved), nt, every)
                sbd._dist_cache["key"] = None
                t0 = time.perf_counter()
                sbd.diag(1, *args, u, v, t, ci, **kw)
                secs.append((time.perf_counter() - t0) / nt)
            out[f"every{every}_{'on' if on else 'off'}"] = dict(s_per_step=min(secs[1:]), runs=secs)
    print("RESULT " + json.dumps(out))


def _child_parent(spec):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from seabreeze_param_amd import hip, synth

    dt = np.float64
    ctx = hip.Context(0)
    g = _grids(np, synth, dt)
    s = torch.cuda.Stream()
    out = {}
    for grid, k in (("bench_k15", 15), ("regional_k113", 113)):
        lon, lat, land, ice = g[grid]
        coast = ctx.get_edges(land, ice)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
        d_co, d_lf, d_cd = dev(coast), dev(land), dev(np.zeros_like(land))
        fn = lambda: ctx.get_dist_dev(dt, NX, NY, d_co.data_ptr(), d_lf.data_ptr(), lon, lat, d_cd.data_ptr(), maxdist=180.0, kwin=k,
                                      stream=s.cuda_stream)
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
            s.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(30)]
            for a, b in ev:
                a.record(s); fn(); b.record(s)
            s.synchronize()
        out[f"get_dist_f64_dev_k{k}"] = dict(us=float(np.median([1e3 * a.elapsed_time(b) for a, b in ev])))
    ctx.close()
    print("RESULT " + json.dumps(out))


def _run(part, lib, limit):
    env = dict(os.environ)
    if lib:
        env["SEABREEZE_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SEABREEZE_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", part], env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"child {part} for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--parts", default="ice,driver,parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_ice_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        {"ice": _child_ice, "driver": _child_driver, "parent": _child_parent}[a.child](a.child)
        return
    res = dict(tool="stream_ice_cost", nx=NX, ny=NY, maxdist_km=180.0, runs="one run on one machine")

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    parts = a.parts.split(",")
    try:
        if "ice" in parts:
            res["ice"] = _run("ice", None, a.limit)
            write()
        if "driver" in parts:
            res["driver_1024x768x8_f32_200_steps"] = _run("driver", None, a.limit)
            write()
        if "parent" in parts and a.parent_lib:
            rounds = []
            for i in range(a.rounds):
                rounds.append(dict(parent=_run("parent", a.parent_lib, a.limit), tree=_run("parent", None, a.limit)))
            chk = {}
            for key in rounds[0]["tree"]:
                par = [r["parent"][key]["us"] for r in rounds]
                mine = [r["tree"][key]["us"] for r in rounds]
                lo, hi = min(par) / WIDEN, max(par) * WIDEN
                chk[key] = dict(parent_us=par, this_build_us=mine, widen=WIDEN, range_us=[lo, hi], ok=all(lo <= m <= hi for m in mine))
            res["existing_calls_did_not_move"] = chk
            write()
    except (SystemExit, subprocess.TimeoutExpired):
        res["incomplete"] = True
        write()
        raise
    print(json.dumps(res))
    bad = [k for k, v in res.get("existing_calls_did_not_move", {}).items() if not v["ok"]]
    if bad:
        raise SystemExit(f"outside the parent's range widened by {WIDEN}: {bad}")


if __name__ == "__main__":
    main()
