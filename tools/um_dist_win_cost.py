"""Cost of the UM-layout coast distance at windows beyond the ghost width (k_dist_um_wide).

    python tools/um_dist_win_cost.py [--nocut-lib PATH] [--rounds 2] [--out profiles/um_dist_win_cost.json]

times, with HIP events on one torch stream (device-resident arguments, warm, median of up to 50 enqueues; an interval
holds the call's two launches and the gap to the event before), in fp64 on the 2560 x 1920 rotated-pole "dateline" grid
of tests/um_setup_ref.py with bench.py's synthetic land/ice mask (15 ghost cells):
  * window = halo = 15 through sb_get_dist_um_f64_dev and through sb_get_dist_um_win_f64_dev (both run k_dist_um: the
    control -- the times must lie within each other's spread and the fields must be the same bits);
  * windows 40 and 60 at 0.036 degrees and window 113 at 0.0135 degrees through sb_get_dist_um_win_f64_dev
    (k_dist_um_wide);
  * next to each, sb_get_dist_f64_dev on a regular grid at the same kwin in the same process (bench.py's grid; for 113
    the regional 0.0135-degree grid of tools/dist_wide_cost.py), and what visiting every hit would cost by scaling the
    measured k_dist_um: 520 us * ((2w+1)/31)^2.
--nocut-lib names this tree built with EXTRA=-DSB_UM_WIN_NO_LAT_CUT (csrc/Makefile: BUILD= / OUT= / EXTRA=): the same wide
cases, whose fields must be the same bits (sha1 of the interior).  A library is loaded through SEABREEZE_HIP_LIB, so each
is measured in fresh child processes of this tool, taking turns `--rounds` times; the JSON keeps every round.  A child
that fails or outlives --limit ends the tool (subprocess.run kills the child when its timeout expires: nothing is
started on the GPU after a fault or a hang); the rounds taken so far are in the JSON.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, HALO = 2560, 1920, 15
K_DIST_UM_US = 520.0                  # k_dist_um at window 15 (README): every hit of 31 x 31 cells visited
CASES = (("um", 0.036, 15), ("win", 0.036, 15), ("win", 0.036, 40), ("win", 0.036, 60), ("win", 0.0135, 113))
WIDE = tuple(c for c in CASES if c[2] > 31)


def _child(cases):
    import numpy as np
    import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from seabreeze_param_amd import hip, synth
    import um_setup_ref as ur

    dt, h = np.float64, HALO
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    st_l = synth.static_fields(NX + 2 * h, NY + 2 * h, dt)
    coast_l = ctx.get_edges_um(st_l.landfrac, st_l.icefrac, h, h)
    lf = np.ascontiguousarray(st_l.landfrac[h:h + NY, h:h + NX])
    d_co, d_lf = dev(coast_l), dev(lf)
    d_cd = torch.zeros_like(d_co)
    st = synth.static_fields(NX, NY, dt)                                   # the regular grid, as bench.py's
    r_co, r_lf = dev(ctx.get_edges(st.landfrac, st.icefrac)), dev(st.landfrac)
    r_cd = torch.zeros((NY, NX), dtype=torch.float64, device="cuda")
    regional = (10.0 + 0.0135 * np.arange(NX), 60.0 + 0.0135 * np.arange(NY))
    s = torch.cuda.Stream()
    sh = s.cuda_stream

    def timed(fn):
        with torch.cuda.stream(s):
            fn()                                                         # workspace, tables
            s.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s); fn(); b.record(s)
            s.synchronize()
            one = a.elapsed_time(b) * 1e-3                               # seconds: how many repeats two seconds hold
            n = int(min(50, max(5, 2.0 / max(one, 1e-6))))
            for _ in range(2):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for a, b in ev:
                a.record(s); fn(); b.record(s)
            s.synchronize()
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n)

    out = {}
    for entry, deg, w in cases:
        lat, lon = ur.grid_named("dateline", NX, NY, dt, dlon=deg, dlat=deg)
        d_la, d_lo = dev(lat), dev(lon)
        torch.cuda.synchronize()
        args = (d_co.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(), d_lo.data_ptr(), d_cd.data_ptr())
        if entry == "um":
            fn = lambda: ctx.get_dist_um_dev(dt, NX, NY, h, h, *args, maxdist=180.0, stream=sh)
        else:
            fn = lambda: ctx.get_dist_um_win_dev(dt, NX, NY, h, h, w, w, *args, maxdist=180.0, stream=sh)
        r = timed(fn)
        cd = np.ascontiguousarray(d_cd.cpu().numpy()[h:h + NY, h:h + NX])
        r.update(reached_frac=float(np.mean(cd < 12000.0)), sha1=hashlib.sha1(cd.tobytes()).hexdigest(),
                 every_hit_scaled_us=K_DIST_UM_US * ((2 * w + 1) / 31.0) ** 2)
        rlon, rlat = regional if w == 113 else (st.lon, st.lat)
        reg = lambda: ctx.get_dist_dev(dt, NX, NY, r_co.data_ptr(), r_lf.data_ptr(), rlon, rlat, r_cd.data_ptr(),
                                       maxdist=180.0, kwin=w, stream=sh)
        r["regular_get_dist_dev"] = timed(reg)
        out[f"{entry}_{deg}_w{w}"] = r
    ctx.close()
    print("RESULT " + json.dumps(out))


def _run(lib, cases, limit):
    env = dict(os.environ)
    if lib:
        env["SEABREEZE_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SEABREEZE_HIP_LIB", None)
    spec = ",".join(f"{e}:{d}:{w}" for e, d, w in cases)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec], env=env, capture_output=True, text=True,
                       timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"child for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--nocut-lib", default=None, help="this tree built with EXTRA=-DSB_UM_WIN_NO_LAT_CUT")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "um_dist_win_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        _child([(e, float(d), int(w)) for e, d, w in (c.split(":") for c in a.child.split(","))])
        return
    plans = [("tree", None, CASES)]
    if a.nocut_lib:
        plans.append(("no_lat_cut", a.nocut_lib, WIDE))
    rounds = []

    def write(**more):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="um_dist_win_cost", nx=NX, ny=NY, halo=HALO, dtype="f64", maxdist_km=180.0, **more,
                           rounds=rounds), f, indent=1)
            f.write("\n")

    for i in range(a.rounds):
        rounds.append({})
        for name, lib, cases in plans:
            try:
                rounds[-1][name] = _run(lib, cases, a.limit)
            except (SystemExit, subprocess.TimeoutExpired):
                write(incomplete=f"round {i}, {name}")
                raise
            print(f"round {i} {name}: " + json.dumps({k: v["median_us"] for k, v in rounds[-1][name].items()}), flush=True)
    summary, same = {}, {}
    for name, _, cases in plans:
        for e, d, w in cases:
            key = f"{e}_{d}_w{w}"
            runs = [r[name][key] for r in rounds]
            summary.setdefault(name, {})[key] = dict(
                median_us=sorted(x["median_us"] for x in runs)[len(runs) // 2], medians_us=[x["median_us"] for x in runs],
                regular_us=sorted(x["regular_get_dist_dev"]["median_us"] for x in runs)[len(runs) // 2],
                every_hit_scaled_us=runs[0]["every_hit_scaled_us"], reached_frac=runs[0]["reached_frac"], sha1=runs[0]["sha1"])
    t = summary["tree"]
    same["w15_both_entries"] = t["um_0.036_w15"]["sha1"] == t["win_0.036_w15"]["sha1"]
    if a.nocut_lib:
        for e, d, w in WIDE:
            key = f"{e}_{d}_w{w}"
            same[f"{key}_cut_vs_no_cut"] = t[key]["sha1"] == summary["no_lat_cut"][key]["sha1"]
    write(summary=summary, same_bits=same)
    print(json.dumps(dict(summary=summary, same_bits=same)))
    if not all(same.values()):
        raise SystemExit(f"fields differ: {same}")


if __name__ == "__main__":
    main()
