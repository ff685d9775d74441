"""Cost of following the sea ice in the UM layout (sb_um_ice_*_dev), and whether the existing
calls and the benchmark moved.

    python tools/um_ice_cost.py --parent-lib PATH [--rounds 3] [--out profiles/um_ice_cost.json]

Ice.  This tree only, fp64 and fp32: 2560 x 1920 on the rotated-pole "dateline" grid of tests/um_setup_ref.py with bench.py's
synthetic land / ice mask in frames of 15 ghost cells -- window 15 at 0.036 degrees (window = halo: k_dist_um) and window 113
at 0.0135 degrees (k_dist_um_wide).  HIP-event time of one sb_um_ice_*_dev call on device-resident frames, median of five,
for four planes, each taken by alternating between the base plane and the changed one (every timed call then sees exactly
that change): unchanged; one cell crossing the threshold; an ice edge moved by a row over 200 columns; one more iced cell in
every 4 x 64 tile.  Beside it `today`, sb_get_edges_um_*_dev + sb_get_dist_um_win_*_dev on the same frames, and `whole`, the
same planes with incremental = 0.  After every plane the interior must equal today's bit for bit.

Existing calls.  sb_get_dist_um_f64_dev (halo 15), sb_get_dist_um_win_f64_dev (113) and bench.py --gpus 1 --steps 20
--warmup 5 under a library built from the parent commit (the Makefile's A/B recipe: BUILD= / OUT=) and under this tree's, in
fresh child processes (SEABREEZE_HIP_LIB), the two taking turns, `--rounds` times.  The criterion is the project's: each of
this tree's runs inside the parent's own range widened by 3 %.

Every GPU step is a child process under its own `timeout -k 10 <limit>`; the first one that fails or outlives its limit
ends the tool (nothing is started on the GPU after a fault or a hang); what was taken so far is in the JSON.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, HALO = 2560, 1920, 15
#        name            window  degrees
GRIDS = (("deg0.036_w15", 15, 0.036), ("deg0.0135_w113", 113, 0.0135))
TILE_ROWS, TILE_COLS = 4, 64


def _imports():
    import numpy as np
    import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from seabreeze_param_amd import hip, synth
    import um_setup_ref as ur
    return np, torch, hip, synth, ur


def _median5(np, torch, s, calls):
    """calls: one callable per timed call (five of them), each run once between two events"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls]
    with torch.cuda.stream(s):
        for (a, b), fn in zip(ev, calls):
            a.record(s); fn(); b.record(s)
        s.synchronize()
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=len(calls))


def _planes(np, land_l, ice_l, dt):
    """the base frame and the three changed ones; changes lie in the interior, over open sea"""
    h = HALO
    sea = (land_l == 0) & (ice_l == 0)
    open5 = sea.copy()                                                   # open sea in the 5 x 5 cells round
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            open5 &= np.roll(np.roll(sea, dy, 0), dx, 1)
    inner = np.zeros_like(open5)
    inner[h + 2:h + NY - 2, h + 2:h + NX - 2] = True
    open5 &= inner
    ys, xs = np.nonzero(open5)
    assert ys.size, "no open sea"
    one = ice_l.copy()
    one[ys[ys.size // 2], xs[ys.size // 2]] = 0.6
    edge = ice_l.copy()
    row = h + NY // 2
    cols = np.flatnonzero(sea[row, h:h + NX])[:200] + h
    edge[row, cols] = 0.6
    every = ice_l.copy()
    n_every = 0
    for g in range(NY // TILE_ROWS):
        for t in range(NX // TILE_COLS):
            blk = open5[h + TILE_ROWS * g:h + TILE_ROWS * (g + 1), h + TILE_COLS * t:h + TILE_COLS * (t + 1)]
            c = np.flatnonzero(blk)
            if c.size:
                y, x = divmod(int(c[c.size // 2]), TILE_COLS)
                every[h + TILE_ROWS * g + y, h + TILE_COLS * t + x] = 0.6
                n_every += 1
    f = lambda a: np.ascontiguousarray(a, dtype=dt)
    return dict(unchanged=f(ice_l), one_cell=f(one), edge_row_200=f(edge), every_tile=f(every)), int(cols.size), n_every


def _child_ice():
    np, torch, hip, synth, ur = _imports()
    out = {}
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    h = HALO
    for dt in (np.float64, np.float32):
        st_l = synth.static_fields(NX + 2 * h, NY + 2 * h, dt)
        land_l, ice_l = np.ascontiguousarray(st_l.landfrac, dt), np.ascontiguousarray(st_l.icefrac, dt)
        planes, n_edge, n_every = _planes(np, land_l, ice_l, dt)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
        d_lf_l = dev(land_l)
        d_lf = dev(land_l[h:h + NY, h:h + NX])
        d_ci = {nm: dev(p) for nm, p in planes.items()}
        for name, w, deg in GRIDS:
            lat, lon = ur.grid_named("dateline", NX, NY, dt, dlon=deg, dlat=deg)
            d_la, d_lo = dev(lat), dev(lon)
            ctx = hip.Context(0)
            d_cd, d_coast, d_ref = (torch.zeros_like(d_lf_l) for _ in range(3))
            torch.cuda.synchronize()
            res = dict(window=w, halo=h, degrees=deg, edge_cells=n_edge, every_tile_cells=n_every)

            def today(ci):
                ctx.get_edges_um_dev(dt, NX, NY, h, h, d_lf_l.data_ptr(), ci.data_ptr(), d_coast.data_ptr(), stream=sh)
                ctx.get_dist_um_win_dev(dt, NX, NY, h, h, w, w, d_coast.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(), d_lo.data_ptr(),
                                        d_ref.data_ptr(), maxdist=180.0, stream=sh)

            refs = {}
            for nm in planes:
                today(d_ci[nm]); s.synchronize()
                refs[nm] = d_ref.cpu().numpy()[h:h + NY, h:h + NX].copy()
            res["today"] = _median5(np, torch, s, [lambda: today(d_ci["unchanged"])] * 5)
            res["reached_frac"] = float(np.mean(np.abs(refs["unchanged"]) < 12000.0))
            for inc in (True, False):
                ctx.um_coast_open(dt, NX, NY, h, h, w, w, lat, lon, maxdist=180.0, incremental=inc)
                call = lambda nm: ctx.um_ice_dev(dt, d_lf_l.data_ptr(), d_ci[nm].data_ptr(), d_cd.data_ptr(), stream=sh)
                call("unchanged"); s.synchronize()
                first = ctx.um_ice_report()
                for nm in planes:
                    # base, changed, base, ...: the calls behind the first each see exactly this change; five are timed
                    call("unchanged"); call(nm); s.synchronize()
                    seq = ["unchanged", nm, "unchanged", nm, nm if nm == "unchanged" else "unchanged"]
                    t = _median5(np, torch, s, [(lambda q=q: call(q)) for q in seq])
                    call(nm); s.synchronize()
                    rep = ctx.um_ice_report()
                    got = d_cd.cpu().numpy()[h:h + NY, h:h + NX]
                    t.update(tiles_marked=rep["tiles_marked"], tiles=rep["tiles"],
                             marked_share=rep["tiles_marked"] / rep["tiles"],
                             equal_bits=bool(np.array_equal(np.ascontiguousarray(got).view(np.uint8), refs[nm].view(np.uint8))))
                    res[("ice_" if inc else "whole_") + nm] = t
                res["first_call_tiles" if inc else "whole_first_call_tiles"] = first["tiles_marked"]
                ctx.um_coast_close()
            ctx.close()
            out[f"{name}_{np.dtype(dt).name}"] = res
            print(f"{name} {np.dtype(dt).name}: " + json.dumps({a: round(b["median_us"], 1) for a, b in res.items() if isinstance(b, dict)}),
                  flush=True)
    print("RESULT " + json.dumps(out))


def _child_ab():
    """the existing calls, under whichever library SEABREEZE_HIP_LIB names"""
    np, torch, hip, synth, ur = _imports()
    dt, h = np.float64, HALO
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    st_l = synth.static_fields(NX + 2 * h, NY + 2 * h, dt)
    coast_l = ctx.get_edges_um(st_l.landfrac, st_l.icefrac, h, h)
    d_co, d_lf = dev(coast_l), dev(st_l.landfrac[h:h + NY, h:h + NX])
    d_cd = torch.zeros_like(d_co)
    out = {}

    def timed(fn, n):
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
            s.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for a, b in ev:
                a.record(s); fn(); b.record(s)
            s.synchronize()
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n)

    for key, w, deg, n in (("get_dist_um_f64_dev_halo15", 15, 0.036, 30), ("get_dist_um_win_f64_dev_w113", 113, 0.0135, 20)):
        lat, lon = ur.grid_named("dateline", NX, NY, dt, dlon=deg, dlat=deg)
        d_la, d_lo = dev(lat), dev(lon)
        torch.cuda.synchronize()
        args = (d_co.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(), d_lo.data_ptr(), d_cd.data_ptr())
        if w == 15:
            out[key] = timed(lambda: ctx.get_dist_um_dev(dt, NX, NY, h, h, *args, maxdist=180.0, stream=sh), n)
        else:
            out[key] = timed(lambda: ctx.get_dist_um_win_dev(dt, NX, NY, h, h, w, w, *args, maxdist=180.0, stream=sh), n)
    ctx.close()
    print("RESULT " + json.dumps(out))


def _env(lib):
    env = dict(os.environ)
    if lib:
        env["SEABREEZE_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SEABREEZE_HIP_LIB", None)
    return env


def _step(cmd, lib, limit, what):
    """one GPU step: a child of its own under `timeout -k 10`; a failure ends the tool"""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=_env(lib), capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"{what} for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def _run(lib, what, limit):
    out = _step([sys.executable, os.path.abspath(__file__), "--child", what], lib, limit, f"{what} child")
    sys.stdout.write("".join(l + "\n" for l in out.splitlines() if not l.startswith("RESULT ")))
    line = [l for l in out.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _bench(lib, limit):
    out = _step([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, limit, "bench.py")
    doc = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    return dict(median_us=1e3 * doc["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child process may take")
    ap.add_argument("--skip-ice", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "um_ice_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        (_child_ice if a.child == "ice" else _child_ab)()
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    doc = dict(tool="um_ice_cost", nx=NX, ny=NY, halo=HALO, grid="dateline", maxdist_km=180.0, rounds=[])

    def write(**more):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(doc, **more), f, indent=1)
            f.write("\n")

    try:
        if not a.skip_ice:
            doc["ice"] = _run(None, "ice", a.limit)
            write(incomplete=True)
        for i in range(a.rounds):
            doc["rounds"].append({})
            for name, lib in (("parent", a.parent_lib), ("tree", None)):
                r = _run(lib, "ab", a.limit)
                r["bench_us_per_step"] = _bench(lib, a.limit)
                doc["rounds"][-1][name] = r
                print(f"round {i} {name}: " + json.dumps({k: round(v["median_us"], 1) for k, v in r.items()}), flush=True)
            write(incomplete=True)
    except SystemExit:
        write(incomplete=True)
        raise
    summary, outside = {}, {}
    for key in doc["rounds"][0]["parent"]:
        par = [r["parent"][key]["median_us"] for r in doc["rounds"]]
        tree = [r["tree"][key]["median_us"] for r in doc["rounds"]]
        summary[key] = dict(parent_us=par, tree_us=tree, band_us=[min(par) * 0.97, max(par) * 1.03])
        bad = [t for t in tree if not min(par) * 0.97 <= t <= max(par) * 1.03]
        if bad:
            outside[key] = dict(runs_us=bad, side="slower" if max(bad) > max(par) * 1.03 else "faster")
    equal = all(v["equal_bits"] for g in doc.get("ice", {}).values() for v in g.values() if isinstance(v, dict) and "equal_bits" in v)
    write(existing_calls=summary, outside_parent_range_widened_3pct=outside, ice_fields_equal_todays=equal)
    print(json.dumps(dict(existing_calls=summary, outside=outside, equal=equal)))
    if not equal:
        raise SystemExit("an ice call's field differs from get_edges_um + get_dist_um_win")


if __name__ == "__main__":
    main()
