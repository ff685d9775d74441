"""Cost of the UM-layout coast setup on one tile of a 2-D decomposition (sb_tile_get_edges_um_*_dev,
sb_tile_get_dist_um_*_dev), and whether the existing calls and the benchmark moved.

    python tools/um_tile_cost.py --parent-lib PATH [--rounds 3] [--out profiles/um_tile_cost.json]

Tile.  This tree only, fp64: the 2560 x 1920 rotated-pole "dateline" grid of tests/um_setup_ref.py with bench.py's synthetic
land / ice mask, cut 4 x 4; the timed tile is the 640 x 480 one at (1, 1), which has no edge side, in frames of window + 1
ghost cells -- window 15 at 0.036 degrees and window 113 at 0.0135 degrees (the spacing of tools/um_dist_win_cost.py).
HIP-event time, warm, median of up to 50 enqueues on one torch stream, of
  * sb_tile_get_dist_um_f64_dev (k_coastbits over the extended rectangle + k_dist_um_tile over the interior),
  * sb_tile_get_edges_um_f64_dev with ext = window (k_edges_um_tile over the extended rectangle),
  * the comparison, in the same process: sb_get_dist_um_win_f64_dev on a whole domain the size of the tile's extended
    rectangle, (640 + 2w) x (480 + 2w), cut from the same fields -- the same source staging, for more targets.
Both times and their ratio are written down; nothing is tuned against them.  The tile's interior must equal the tile's cells
of sb_get_dist_um_win_f64_dev on the whole 2560 x 1920 domain, bit for bit.

Existing calls.  tools/um_ice_cost.py's A/B: sb_get_dist_um_f64_dev (halo 15), sb_get_dist_um_win_f64_dev (113) and
bench.py --gpus 1 --steps 20 --warmup 5 under a library built from the parent commit and under this tree's, in fresh child
processes, the two taking turns, `--rounds` times; each of this tree's runs must lie inside the parent's own range widened
by 3 %.

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
import um_ice_cost as ab                                                 # its A/B children and its step runner

NX, NY, CUT = 2560, 1920, 4
TILE = (NX // CUT, 2 * NX // CUT, NY // CUT, 2 * NY // CUT)              # x0, x1, y0, y1: no edge side
#        name            window  degrees
GRIDS = (("deg0.036_w15", 15, 0.036), ("deg0.0135_w113", 113, 0.0135))


def _child_tile():
    np, torch, hip, synth, ur = ab._imports()
    import um_tile_ref as ut
    dt = np.float64
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
    s = torch.cuda.Stream()
    sh = s.cuda_stream

    def timed(fn):
        with torch.cuda.stream(s):
            fn()                                                         # workspace
            s.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s); fn(); b.record(s)
            s.synchronize()
            n = int(min(50, max(5, 2.0 / max(a.elapsed_time(b) * 1e-3, 1e-6))))
            for _ in range(2):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for a, b in ev:
                a.record(s); fn(); b.record(s)
            s.synchronize()
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n)

    st = synth.static_fields(NX, NY, dt)
    land, ice = np.ascontiguousarray(st.landfrac, dt), np.ascontiguousarray(st.icefrac, dt)
    coast = np.ascontiguousarray(ctx.get_edges_um(ur.pad_edge(land, 1, 1), ur.pad_edge(ice, 1, 1), 1, 1)[1:-1, 1:-1])
    x0, x1, y0, y1 = TILE
    nxt, nyt = x1 - x0, y1 - y0
    out = {}
    for name, w, deg in GRIDS:
        h = w + 1
        lat, lon = ur.grid_named("dateline", NX, NY, dt, dlon=deg, dlat=deg)
        fr = lambda a: ut.cut(a, x0, x1, y0, y1, h, h, 0.0)
        d_co, d_lf, d_ci, d_la, d_lo = (dev(fr(a)) for a in (coast, land, ice, lat, lon))
        d_cd, d_ed = torch.zeros_like(d_co), torch.zeros_like(d_co)
        # the comparison domain: the tile's extended rectangle as a whole domain without ghost cells
        ex = lambda a: np.ascontiguousarray(a[y0 - w:y1 + w, x0 - w:x1 + w])
        e_co, e_lf, e_la, e_lo = (dev(ex(a)) for a in (coast, land, lat, lon))
        e_cd = torch.zeros_like(e_co)
        torch.cuda.synchronize()
        res = dict(window=w, halo=h, degrees=deg, tile=[nxt, nyt], extended=[nxt + 2 * w, nyt + 2 * w])
        res["tile_get_dist_um_dev"] = timed(lambda: ctx.tile_get_dist_um_dev(
            dt, nxt, nyt, h, h, w, w, 0, d_co.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(), d_lo.data_ptr(), d_cd.data_ptr(),
            maxdist=180.0, stream=sh))
        res["tile_get_edges_um_dev"] = timed(lambda: ctx.tile_get_edges_um_dev(
            dt, nxt, nyt, h, h, w, w, 0, d_lf.data_ptr(), d_ci.data_ptr(), d_ed.data_ptr(), stream=sh))
        res["get_dist_um_win_dev_on_extended"] = timed(lambda: ctx.get_dist_um_win_dev(
            dt, nxt + 2 * w, nyt + 2 * w, 0, 0, w, w, e_co.data_ptr(), e_lf.data_ptr(), e_la.data_ptr(), e_lo.data_ptr(),
            e_cd.data_ptr(), maxdist=180.0, stream=sh))
        res["tile_over_extended"] = res["tile_get_dist_um_dev"]["median_us"] / res["get_dist_um_win_dev_on_extended"]["median_us"]
        # the tile's cells of the whole-domain field (layout halo 1: the wide kernel at either window)
        whole = ctx.get_dist_um_win(np.ascontiguousarray(np.pad(coast, 1)), land, lat, lon, 1, 1, w, w, maxdist=180.0)[1:-1, 1:-1]
        got = d_cd.cpu().numpy()[h:h + nyt, h:h + nxt]
        ed = d_ed.cpu().numpy()[h - w:h + nyt + w, h - w:h + nxt + w]
        res["equal_bits"] = bool(np.array_equal(got, whole[y0:y1, x0:x1]))
        res["edges_equal"] = bool(np.array_equal(ed, coast[y0 - w:y1 + w, x0 - w:x1 + w]))
        res["reached_frac"] = float(np.mean(np.abs(got) < 12000.0))
        out[name] = res
        print(f"{name}: " + json.dumps({a: round(b["median_us"], 1) for a, b in res.items() if isinstance(b, dict)}), flush=True)
    ctx.close()
    print("RESULT " + json.dumps(out))


def _run_tile(limit):
    o = ab._step([sys.executable, os.path.abspath(__file__), "--child", "tile"], None, limit, "tile child")
    sys.stdout.write("".join(l + "\n" for l in o.splitlines() if not l.startswith("RESULT ")))
    return json.loads([l for l in o.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "um_tile_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        _child_tile()
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    doc = dict(tool="um_tile_cost", nx=NX, ny=NY, cut=[CUT, CUT], tile_x0_x1_y0_y1=list(TILE), grid="dateline", dtype="f64", maxdist_km=180.0,
               rounds=[])

    def write(**more):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(doc, **more), f, indent=1)
            f.write("\n")

    try:
        doc["tile"] = _run_tile(a.limit)
        write(incomplete=True)
        for i in range(a.rounds):
            doc["rounds"].append({})
            for name, lib in (("parent", a.parent_lib), ("tree", None)):
                r = ab._run(lib, "ab", a.limit)
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
    equal = all(v["equal_bits"] and v["edges_equal"] for v in doc["tile"].values())
    slower = {k: v["tile_over_extended"] for k, v in doc["tile"].items() if v["tile_over_extended"] > 1.0}
    write(existing_calls=summary, outside_parent_range_widened_3pct=outside, tile_fields_equal_whole_domain=equal,
          tile_slower_than_extended_call=slower)
    print(json.dumps(dict(existing_calls=summary, outside=outside, equal=equal, tile_slower_than_extended_call=slower)))
    if not equal:
        raise SystemExit("a tile's field differs from the whole-domain get_edges_um + get_dist_um_win")


if __name__ == "__main__":
    main()
