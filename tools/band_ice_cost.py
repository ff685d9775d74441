"""Cost of following the sea ice in one latitude band (sb_band_ice_*_dev), and whether the existing
coast calls and the benchmark moved.

    python tools/band_ice_cost.py --parent-lib PATH [--rounds 3] [--out profiles/band_ice_cost.json]

Ice.  This tree only, fp64 and fp32: one band of eight of 2560 x 1920 (rows 720 .. 959, cuts on both sides) -- the benchmark
mask under the N1280 coordinates with kwin = 15 in a frame of 16 ghost cells, and under 0.0135-degree regional coordinates
with kwin = 113 in a frame of 114.  HIP-event time of one sb_band_ice_*_dev call, median of five, for four planes, each
taken by alternating between the base plane and the changed one (every call then sees exactly that change): unchanged; one
cell crossing the threshold; the ice edge moved by a row over 200 columns; one more iced cell in every tile.  Beside it
sb_band_get_edges_*_dev + sb_band_get_dist_*_dev on the same frames (today's path with its exchanges left out) and the same
planes with incremental = 0.  After every plane the interior must equal the band calls' bit for bit.  Then, through
BandRunner on a one-rank world (the band as the globe, no ghost cells), the wall time of update_ice against setup_mask.

Existing calls.  sb_band_get_dist_f64_dev (kwin = 15 and 113), sb_get_dist_f64_dev (2560 x 1920, kwin = 15) and
bench.py --gpus 1 --steps 20 --warmup 5 under a library built from the parent commit (the Makefile's A/B recipe: BUILD= /
OUT=) and under this tree's, in fresh child processes (SEABREEZE_HIP_LIB), the two taking turns, `--rounds` times.  The
criterion is the project's: this tree's median inside the parent's range widened by 3 %.

A child that fails or outlives --limit ends the tool (nothing is started on the GPU after a fault or a hang); what was
taken so far is in the JSON.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, BAND_ROWS, R0 = 2560, 1920, 240, 720
#        name          kwin  coordinates
GRIDS = (("N1280_k15", 15, "global"), ("deg0.0135_k113", 113, "regional"))


def _imports():
    import numpy as np
    import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)
    sys.path.insert(0, ROOT)
    from seabreeze_param_amd import hip, synth
    return np, torch, hip, synth


def _coords(np, synth, kind):
    if kind == "global":
        return synth.grid(NX, NY)
    return 10.0 + 0.0135 * np.arange(NX), 56.0 + 0.0135 * np.arange(NY)      # 56 .. 82 N: 70 N inside


def _median5(np, torch, s, calls):
    """calls: one callable per timed call (five of them), each run once between two events"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls]
    with torch.cuda.stream(s):
        for (a, b), fn in zip(ev, calls):
            a.record(s); fn(); b.record(s)
        s.synchronize()
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=len(calls))


def _planes(np, land, ice, dt):
    """the base plane (whole grid) and the three changed ones; changes lie in the band's own rows, over open sea"""
    r1 = R0 + BAND_ROWS
    sea = (land == 0) & (ice == 0)
    open5 = sea.copy()                                                   # open sea in the 5 x 5 cells round
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            open5 &= np.roll(np.roll(sea, dy, 0), dx, 1)
    ys, xs = np.nonzero(open5[R0 + 60:r1 - 60])
    assert ys.size, "no open sea in the band"
    one = ice.copy()
    one[R0 + 60 + ys[ys.size // 2], xs[ys.size // 2]] = 0.6
    edge = ice.copy()
    row = R0 + 120
    cols = np.flatnonzero(sea[row])[:200]
    edge[row, cols] = 0.6
    every = ice.copy()
    n_every = 0
    for y in range(R0 + 4, r1, 8):
        for t in range(NX // 256):
            c = np.flatnonzero(open5[y, 256 * t:256 * (t + 1)])
            if c.size:
                every[y, 256 * t + c[c.size // 2]] = 0.6
                n_every += 1
    f = lambda a: np.ascontiguousarray(a, dtype=dt)
    return dict(unchanged=f(ice), one_cell=f(one), edge_row_200=f(edge), every_tile=f(every)), int(cols.size), n_every


def _child_ice():
    np, torch, hip, synth = _imports()
    out = {}
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    r0, r1 = R0, R0 + BAND_ROWS
    for dt in (np.float64, np.float32):
        st = synth.static_fields(NX, NY, dt)
        land, ice = np.ascontiguousarray(st.landfrac, dt), np.ascontiguousarray(st.icefrac, dt)
        planes, n_edge, n_every = _planes(np, land, ice, dt)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
        for name, k, kind in GRIDS:
            h = k + 1
            lon, lat = _coords(np, synth, kind)
            fr = lambda a: np.pad(a[r0 - h:r1 + h], ((0, 0), (h, h)), mode="wrap")
            latf = np.ascontiguousarray(lat[r0 - h:r1 + h])
            ctx = hip.Context(0)
            d_lsm = dev(fr(land))
            d_ci = {nm: dev(fr(p)) for nm, p in planes.items()}
            d_cd, d_coast, d_ref = (torch.zeros_like(d_lsm) for _ in range(3))
            torch.cuda.synchronize()
            res = dict(kwin=k, halo=h, edge_cells=n_edge, every_tile_cells=n_every)

            def today(ci):
                ctx.band_get_edges_dev(dt, NX, BAND_ROWS, h, False, False, d_lsm.data_ptr(), ci.data_ptr(), d_coast.data_ptr(), rule=1,
                                       stream=sh)
                ctx.band_get_dist_dev(dt, NX, BAND_ROWS, h, False, False, d_coast.data_ptr(), d_lsm.data_ptr(), lon, latf,
                                      d_ref.data_ptr(), k, maxdist=180.0, stream=sh)

            def reference(nm):
                """the band calls' field for a plane: the coast frame with its ghost rows from the whole-grid call"""
                coast = ctx.get_edges(land, planes[nm], rule=1, bnd=hip.SB_BND_GLOBAL)
                d_coast.copy_(dev(fr(coast)))
                torch.cuda.synchronize()
                ctx.band_get_dist_dev(dt, NX, BAND_ROWS, h, False, False, d_coast.data_ptr(), d_lsm.data_ptr(), lon, latf,
                                      d_ref.data_ptr(), k, maxdist=180.0, stream=sh)
                s.synchronize()
                return d_ref.cpu().numpy()[h:h + BAND_ROWS, h:h + NX].copy()

            refs = {nm: reference(nm) for nm in planes}
            today(d_ci["unchanged"]); s.synchronize()                    # warm
            res["edges_plus_dist"] = _median5(np, torch, s, [lambda: today(d_ci["unchanged"])] * 5)
            for inc in (True, False):
                ctx.band_coast_open(dt, NX, BAND_ROWS, h, False, False, lon, latf, k, rule=1, incremental=inc)
                call = lambda nm: ctx.band_ice_dev(dt, d_lsm.data_ptr(), d_ci[nm].data_ptr(), d_cd.data_ptr(), stream=sh)
                call("unchanged"); s.synchronize()
                first = ctx.band_ice_report()
                for nm in planes:
                    # base, changed, base, ...: the six calls behind the first each see exactly this change; five are timed
                    call("unchanged"); call(nm); s.synchronize()
                    seq = ["unchanged", nm, "unchanged", nm, nm if nm == "unchanged" else "unchanged"]
                    t = _median5(np, torch, s, [(lambda q=q: call(q)) for q in seq])
                    call(nm); s.synchronize()
                    rep = ctx.band_ice_report()
                    got = d_cd.cpu().numpy()[h:h + BAND_ROWS, h:h + NX]
                    t.update(tiles_marked=rep["tiles_marked"], tiles=rep["tiles"],
                             equal_bits=bool(np.array_equal(got.view(np.uint8), refs[nm].view(np.uint8))))
                    res[("ice_" if inc else "ice_whole_") + nm] = t
                res["first_call_tiles" if inc else "whole_first_call_tiles"] = first["tiles_marked"]
                ctx.band_coast_close()
            ctx.close()
            out[f"{name}_{np.dtype(dt).name}"] = res
            print(f"{name} {np.dtype(dt).name}: " + json.dumps({a: round(b["median_us"], 1) for a, b in res.items() if isinstance(b, dict)}),
                  flush=True)
    # BandRunner on a one-rank world: the band as the globe
    from seabreeze_param_amd.bands import BandRunner
    dt = np.float64
    st = synth.static_fields(NX, NY, dt)
    land, ice = np.ascontiguousarray(st.landfrac[R0:r1], dt), np.ascontiguousarray(st.icefrac, dt)
    planes, _, _ = _planes(np, np.ascontiguousarray(st.landfrac, dt), ice, dt)
    for name, k, kind in GRIDS:
        lon, lat = _coords(np, synth, kind)
        lat = lat[R0:r1]
        ctx = hip.Context(0)
        runner = BandRunner(ctx, torch, None, 0, 1, NX, BAND_ROWS, 1, halo=k + 1, dtype=dt)
        res = {}

        def wall(fn):
            ts = []
            for _ in range(5):
                runner.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append(1e6 * (time.perf_counter() - t0))
            return dict(median_us=float(np.median(ts)), min_us=float(min(ts)), max_us=float(max(ts)), n=5)

        runner.setup_mask(land, planes["unchanged"][R0:r1], lon, lat, rule=1, kwin=k)
        res["setup_mask"] = wall(lambda: runner.setup_mask(land, planes["unchanged"][R0:r1], lon, lat, rule=1, kwin=k))
        runner.setup_mask(land, planes["unchanged"][R0:r1], lon, lat, rule=1, kwin=k, follow_ice=True)
        for nm in planes:
            state = {"i": 0}

            def upd():
                state["i"] += 1
                runner.update_ice(planes[nm if state["i"] & 1 else "unchanged"][R0:r1])
            runner.update_ice(planes["unchanged"][R0:r1])
            res["update_ice_" + nm] = wall(upd)
        ctx.close()
        out[f"runner_one_rank_{name}_float64"] = res
        print(f"runner {name}: " + json.dumps({a: round(b["median_us"], 1) for a, b in res.items()}), flush=True)
    print("RESULT " + json.dumps(out))


def _child_ab():
    """the existing calls, under whichever library SEABREEZE_HIP_LIB names"""
    np, torch, hip, synth = _imports()
    dt = np.float64
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    st = synth.static_fields(NX, NY, dt)
    coast = ctx.get_edges(st.landfrac, st.icefrac, rule=1, bnd=hip.SB_BND_GLOBAL)
    out = {}

    def timed(fn):
        with torch.cuda.stream(s):
            for _ in range(3):
                fn()
            s.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(30)]
            for a, b in ev:
                a.record(s); fn(); b.record(s)
            s.synchronize()
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=30)

    d_co, d_lf = dev(coast), dev(st.landfrac)
    d_cd = torch.zeros_like(d_co)
    lon, lat = _coords(np, synth, "global")
    out["get_dist_f64_dev_k15"] = timed(lambda: ctx.get_dist_dev(dt, NX, NY, d_co.data_ptr(), d_lf.data_ptr(), lon, lat, d_cd.data_ptr(),
                                                                 maxdist=180.0, kwin=15, stream=sh))
    r0, r1 = R0, R0 + BAND_ROWS
    for name, k, kind in GRIDS:
        lon, lat = _coords(np, synth, kind)
        fr = lambda a: np.pad(a[r0 - k:r1 + k], ((0, 0), (k, k)), mode="wrap")
        b_co, b_lf = dev(fr(coast)), dev(fr(st.landfrac))
        b_cd = torch.zeros_like(b_co)
        latf = np.ascontiguousarray(lat[r0 - k:r1 + k])
        out[f"band_get_dist_f64_dev_k{k}"] = timed(lambda: ctx.band_get_dist_dev(dt, NX, BAND_ROWS, k, False, False, b_co.data_ptr(),
                                                                                  b_lf.data_ptr(), lon, latf, b_cd.data_ptr(), k,
                                                                                  maxdist=180.0, stream=sh))
    ctx.close()
    print("RESULT " + json.dumps(out))


def _env(lib):
    env = dict(os.environ)
    if lib:
        env["SEABREEZE_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SEABREEZE_HIP_LIB", None)
    return env


def _run(lib, what, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], env=_env(lib), capture_output=True, text=True,
                       timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{what} child for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    sys.stdout.write("".join(l + "\n" for l in r.stdout.splitlines() if not l.startswith("RESULT ")))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _bench(lib, limit):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=_env(lib),
                       capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"bench.py for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    doc = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return dict(median_us=1e3 * doc["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child process may take")
    ap.add_argument("--skip-ice", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_ice_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        (_child_ice if a.child == "ice" else _child_ab)()
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    doc = dict(tool="band_ice_cost", nx=NX, ny=NY, band_rows=BAND_ROWS, band_first_row=R0, rounds=[])

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
    except (SystemExit, subprocess.TimeoutExpired):
        write(incomplete=True)
        raise
    summary, outside = {}, {}
    for key in doc["rounds"][0]["parent"]:
        par = [r["parent"][key]["median_us"] for r in doc["rounds"]]
        tree = [r["tree"][key]["median_us"] for r in doc["rounds"]]
        med = sorted(tree)[len(tree) // 2]
        summary[key] = dict(parent_us=par, tree_us=tree, tree_median_us=med, tree_over_parent=med / sorted(par)[len(par) // 2])
        if not min(par) * 0.97 <= med <= max(par) * 1.03:
            outside[key] = "slower" if med > max(par) else "faster"
    equal = all(v["equal_bits"] for g in doc.get("ice", {}).values() for v in g.values() if isinstance(v, dict) and "equal_bits" in v)
    write(existing_calls=summary, outside_parent_range_widened_3pct=outside, ice_fields_equal_band_calls=equal)
    print(json.dumps(dict(existing_calls=summary, outside=outside, equal=equal)))
    if not equal:
        raise SystemExit("an ice call's field differs from the band calls'")


if __name__ == "__main__":
    main()
