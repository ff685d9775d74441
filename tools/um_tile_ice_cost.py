"""Cost of following the sea ice on one tile of the UM's 2-D decomposition (sb_um_tile_ice_*_dev),
and whether the existing calls and the benchmark moved.

    python tools/um_tile_ice_cost.py --parent-lib PATH [--rounds 3] [--out profiles/um_tile_ice_cost.json]

Ice.  This tree only, fp64 and fp32: tools/um_tile_cost.py's tile -- the 640 x 480 one at (1, 1) of a 4 x 4 cut of the
2560 x 1920 rotated-pole "dateline" grid with bench.py's synthetic land / ice mask, no edge side -- in frames of window + 1
ghost cells, window 15 at 0.036 degrees and window 113 at 0.0135 degrees.  HIP-event time of one sb_um_tile_ice_*_dev call
on device-resident frames, median of five, for five planes, each taken by alternating between the base plane and the changed
one (every timed call then sees exactly that change): unchanged; one interior cell crossing the threshold; one cell in a
neighbour's ghost area inside the window; an ice edge moved by a row over 200 columns; one more iced cell in every 4 x 64
tile.  Beside it `today`, sb_tile_get_edges_um_*_dev (ext = window) + sb_tile_get_dist_um_*_dev on the same frames, and
`whole`, the same planes with incremental = 0.  After every plane the interior must equal today's bit for bit.

Existing calls.  sb_tile_get_dist_um_f64_dev (the tile above, window 113), sb_um_ice_f64_dev (2560 x 1920, halo and window
15, one cell crossing the threshold and back) and bench.py --gpus 1 --steps 20 --warmup 5 under a library built from the
parent commit and under this tree's, in fresh child processes (SEABREEZE_HIP_LIB), the two taking turns, `--rounds` times.
The criterion is the project's: each of this tree's runs inside the parent's own range widened by 3 %.

Every GPU step is a child process under its own `timeout -k 10 <limit>`; the first one that fails or outlives its limit
ends the tool (nothing is started on the GPU after a fault or a hang); what was taken so far is in the JSON.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import um_ice_cost as ab                                                 # its imports, its step runner, its bench call

NX, NY, CUT = 2560, 1920, 4
TILE = (NX // CUT, 2 * NX // CUT, NY // CUT, 2 * NY // CUT)              # x0, x1, y0, y1: no edge side
#        name            window  degrees
GRIDS = (("deg0.036_w15", 15, 0.036), ("deg0.0135_w113", 113, 0.0135))
TILE_ROWS, TILE_COLS = 4, 64


def _planes(np, land_f, ice_f, h, w, nxt, nyt, dt):
    """the base frame and the four changed ones, on the tile's frame with h ghost cells; changes lie over open sea"""
    sea = (land_f == 0) & (ice_f == 0)
    open5 = sea.copy()                                                   # open sea in the 5 x 5 cells round
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            open5 &= np.roll(np.roll(sea, dy, 0), dx, 1)
    inner = np.zeros_like(open5)
    inner[h + 2:h + nyt - 2, h + 2:h + nxt - 2] = True
    ys, xs = np.nonzero(open5 & inner)
    assert ys.size, "no open sea in the interior"
    one = ice_f.copy()
    one[ys[ys.size // 2], xs[ys.size // 2]] = 0.6
    # west of the interior, at least two cells inside the source rectangle (its Sobel neighbours are sources too)
    west = np.zeros_like(open5)
    west[h + 2:h + nyt - 2, h - w + 2:h - 2] = True
    gy, gx = np.nonzero(open5 & west)
    assert gy.size, "no open sea in the west neighbour's ghost cells inside the window"
    ghost = ice_f.copy()
    ghost[gy[gy.size // 2], gx[gy.size // 2]] = 0.6
    edge = ice_f.copy()
    row = h + nyt // 2
    cols = np.flatnonzero(sea[row, h:h + nxt])[:200] + h
    edge[row, cols] = 0.6
    every = ice_f.copy()
    n_every = 0
    for g in range(nyt // TILE_ROWS):
        for t in range(nxt // TILE_COLS):
            blk = (open5 & inner)[h + TILE_ROWS * g:h + TILE_ROWS * (g + 1), h + TILE_COLS * t:h + TILE_COLS * (t + 1)]
            c = np.flatnonzero(blk)
            if c.size:
                y, x = divmod(int(c[c.size // 2]), TILE_COLS)
                every[h + TILE_ROWS * g + y, h + TILE_COLS * t + x] = 0.6
                n_every += 1
    f = lambda a: np.ascontiguousarray(a, dtype=dt)
    return (dict(unchanged=f(ice_f), one_cell=f(one), ghost_cell=f(ghost), edge_row_200=f(edge), every_tile=f(every)),
            int(cols.size), n_every)


def _child_ice():
    np, torch, hip, synth, ur = ab._imports()
    import um_tile_ref as ut
    out = {}
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    x0, x1, y0, y1 = TILE
    nxt, nyt = x1 - x0, y1 - y0
    beyond = (x0, NX - x1, y0, NY - y1)
    for dt in (np.float64, np.float32):
        st = synth.static_fields(NX, NY, dt)
        land, ice = np.ascontiguousarray(st.landfrac, dt), np.ascontiguousarray(st.icefrac, dt)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
        for name, w, deg in GRIDS:
            h = w + 1
            lat, lon = ur.grid_named("dateline", NX, NY, dt, dlon=deg, dlat=deg)
            fr = lambda a: ut.cut(a, x0, x1, y0, y1, h, h, 0.0)
            land_f, lat_f, lon_f = fr(land), fr(lat), fr(lon)
            planes, n_edge, n_every = _planes(np, land_f, fr(ice), h, w, nxt, nyt, dt)
            d_lf, d_la, d_lo = dev(land_f), dev(lat_f), dev(lon_f)
            d_ci = {nm: dev(p) for nm, p in planes.items()}
            ctx = hip.Context(0)
            d_cd, d_coast, d_ref = (torch.zeros_like(d_lf) for _ in range(3))
            torch.cuda.synchronize()
            res = dict(window=w, halo=h, degrees=deg, tile=[nxt, nyt], edge_cells=n_edge, every_tile_cells=n_every)

            def today(ci):
                ctx.tile_get_edges_um_dev(dt, nxt, nyt, h, h, w, w, 0, d_lf.data_ptr(), ci.data_ptr(), d_coast.data_ptr(), stream=sh)
                ctx.tile_get_dist_um_dev(dt, nxt, nyt, h, h, w, w, 0, d_coast.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(),
                                         d_lo.data_ptr(), d_ref.data_ptr(), maxdist=180.0, stream=sh)

            refs = {}
            for nm in planes:
                today(d_ci[nm]); s.synchronize()
                refs[nm] = d_ref.cpu().numpy()[h:h + nyt, h:h + nxt].copy()
            res["today"] = ab._median5(np, torch, s, [lambda: today(d_ci["unchanged"])] * 5)
            res["reached_frac"] = float(np.mean(np.abs(refs["unchanged"]) < 12000.0))
            res["ghost_cell_moves_interior_cells"] = int((refs["ghost_cell"] != refs["unchanged"]).sum())
            for inc in (True, False):
                ctx.um_tile_coast_open(dt, nxt, nyt, h, h, w, w, beyond, lat_f, lon_f, maxdist=180.0, incremental=inc)
                call = lambda nm: ctx.um_tile_ice_dev(dt, d_lf.data_ptr(), d_ci[nm].data_ptr(), d_cd.data_ptr(), stream=sh)
                call("unchanged"); s.synchronize()
                first = ctx.um_tile_ice_report()
                for nm in planes:
                    # base, changed, base, ...: the calls behind the first each see exactly this change; five are timed
                    call("unchanged"); call(nm); s.synchronize()
                    seq = ["unchanged", nm, "unchanged", nm, nm if nm == "unchanged" else "unchanged"]
                    t = ab._median5(np, torch, s, [(lambda q=q: call(q)) for q in seq])
                    call(nm); s.synchronize()
                    rep = ctx.um_tile_ice_report()
                    got = d_cd.cpu().numpy()[h:h + nyt, h:h + nxt]
                    t.update(tiles_marked=rep["tiles_marked"], tiles=rep["tiles"],
                             marked_share=rep["tiles_marked"] / rep["tiles"],
                             equal_bits=bool(np.array_equal(np.ascontiguousarray(got).view(np.uint8), refs[nm].view(np.uint8))))
                    res[("ice_" if inc else "whole_") + nm] = t
                res["first_call_tiles" if inc else "whole_first_call_tiles"] = first["tiles_marked"]
                ctx.um_tile_coast_close()
            ctx.close()
            out[f"{name}_{np.dtype(dt).name}"] = res
            print(f"{name} {np.dtype(dt).name}: " + json.dumps({a: round(b["median_us"], 1) for a, b in res.items() if isinstance(b, dict)}),
                  flush=True)
    print("RESULT " + json.dumps(out))


def _child_ab():
    """the existing calls, under whichever library SEABREEZE_HIP_LIB names"""
    np, torch, hip, synth, ur = ab._imports()
    import um_tile_ref as ut
    dt = np.float64
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    out = {}

    def timed(fns, n):
        """n timed calls, fns taken in turn"""
        with torch.cuda.stream(s):
            for k in range(4):
                fns[k % len(fns)]()
            s.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for k, (a, b) in enumerate(ev):
                a.record(s); fns[k % len(fns)](); b.record(s)
            s.synchronize()
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n)

    # sb_tile_get_dist_um_f64_dev: the 640 x 480 tile, window 113
    st = synth.static_fields(NX, NY, dt)
    land, ice = np.ascontiguousarray(st.landfrac, dt), np.ascontiguousarray(st.icefrac, dt)
    coast = np.ascontiguousarray(ctx.get_edges_um(ur.pad_edge(land, 1, 1), ur.pad_edge(ice, 1, 1), 1, 1)[1:-1, 1:-1])
    x0, x1, y0, y1 = TILE
    nxt, nyt, w = x1 - x0, y1 - y0, 113
    h = w + 1
    lat, lon = ur.grid_named("dateline", NX, NY, dt, dlon=0.0135, dlat=0.0135)
    d_co, d_lf, d_la, d_lo = (dev(ut.cut(a, x0, x1, y0, y1, h, h, 0.0)) for a in (coast, land, lat, lon))
    d_cd = torch.zeros_like(d_co)
    torch.cuda.synchronize()
    out["tile_get_dist_um_f64_dev_w113"] = timed([lambda: ctx.tile_get_dist_um_dev(
        dt, nxt, nyt, h, h, w, w, 0, d_co.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(), d_lo.data_ptr(), d_cd.data_ptr(),
        maxdist=180.0, stream=sh)], 20)
    # sb_um_ice_f64_dev: the whole grid, halo and window 15, one cell crossing the threshold and back
    hh = 15
    st_l = synth.static_fields(NX + 2 * hh, NY + 2 * hh, dt)
    land_l, ice_l = np.ascontiguousarray(st_l.landfrac, dt), np.ascontiguousarray(st_l.icefrac, dt)
    planes, _, _ = ab._planes(np, land_l, ice_l, dt)
    lat, lon = ur.grid_named("dateline", NX, NY, dt, dlon=0.036, dlat=0.036)
    d_lfl, d_a, d_b = dev(land_l), dev(planes["unchanged"]), dev(planes["one_cell"])
    d_cdl = torch.zeros_like(d_lfl)
    ctx.um_coast_open(dt, NX, NY, hh, hh, hh, hh, lat, lon, maxdist=180.0)
    torch.cuda.synchronize()
    out["um_ice_f64_dev_one_cell"] = timed([lambda: ctx.um_ice_dev(dt, d_lfl.data_ptr(), d_b.data_ptr(), d_cdl.data_ptr(), stream=sh),
                                           lambda: ctx.um_ice_dev(dt, d_lfl.data_ptr(), d_a.data_ptr(), d_cdl.data_ptr(), stream=sh)], 40)
    ctx.um_coast_close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def _run(lib, what, limit):
    o = ab._step([sys.executable, os.path.abspath(__file__), "--child", what], lib, limit, f"{what} child")
    sys.stdout.write("".join(l + "\n" for l in o.splitlines() if not l.startswith("RESULT ")))
    return json.loads([l for l in o.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "um_tile_ice_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        (_child_ice if a.child == "ice" else _child_ab)()
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    doc = dict(tool="um_tile_ice_cost", nx=NX, ny=NY, cut=[CUT, CUT], tile_x0_x1_y0_y1=list(TILE), grid="dateline", maxdist_km=180.0,
               rounds=[])

    def write(**more):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(doc, **more), f, indent=1)
            f.write("\n")

    try:
        doc["ice"] = _run(None, "ice", a.limit)
        write(incomplete=True)
        for i in range(a.rounds):
            doc["rounds"].append({})
            for name, lib in (("parent", a.parent_lib), ("tree", None)):
                r = _run(lib, "ab", a.limit)
                r["bench_us_per_step"] = ab._bench(lib, a.limit)
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
    equal = all(v["equal_bits"] for g in doc["ice"].values() for v in g.values() if isinstance(v, dict) and "equal_bits" in v)
    # where the incremental path loses: planes on which it is slower than today's chain or than incremental = 0
    loses = {f"{g}/{k[4:]}": dict(ice_us=v["median_us"], today_us=r["today"]["median_us"], whole_us=r["whole_" + k[4:]]["median_us"])
             for g, r in doc["ice"].items() for k, v in r.items()
             if k.startswith("ice_") and v["median_us"] > min(r["today"]["median_us"], r["whole_" + k[4:]]["median_us"])}
    write(existing_calls=summary, outside_parent_range_widened_3pct=outside, ice_fields_equal_todays=equal,
          incremental_slower_than_today_or_whole=loses)
    print(json.dumps(dict(existing_calls=summary, outside=outside, equal=equal, incremental_loses=loses)))
    if not equal:
        raise SystemExit("an ice call's field differs from tile_get_edges_um + tile_get_dist_um")


if __name__ == "__main__":
    main()
