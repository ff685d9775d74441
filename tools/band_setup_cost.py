"""Cost of the band-local coast setup (sb_band_get_dist_*), and whether the whole-grid get_dist
moved when its kernels gained the target policy.

    python tools/band_setup_cost.py --parent-lib PATH [--rounds 2] [--out profiles/band_setup_cost.json]

Whole grid.  sb_get_dist_f64_dev at 2560 x 1920 with kwin = 15 (the N1280 grid and window) and with kwin = 113 on a 0.0135
degree regional grid of the same size, under a library built from the parent commit (the Makefile's A/B recipe: BUILD= /
OUT=) and under this tree's.  A library is loaded through SEABREEZE_HIP_LIB, so each runs in fresh child processes, the two
taking turns, `--rounds` times; the distance fields of both must be equal bit for bit.  The yardstick is the parent in
the same job and the margin the spread between the parent's own rounds: a case whose median over this tree's rounds lies
outside the parent's range is listed under `outside_parent_range`.

Band.  This tree only: one band of eight of the first grid (2560 x 240, kwin = 15) and a 240-row band of the second
(kwin = 113), an inner band with cuts on both sides in a frame of kwin ghost cells, against the whole-grid call on the
same coordinates in the same process.  The expectation derived from the rows a band reads is (ny + 2 kwin) / NY of the
whole-grid time plus the launch floor; the ratio is reported, no threshold is set.  The band's interior must equal the
whole grid's rows bit for bit.

Times are medians of warm, event-timed `_dev` calls on one torch stream with device-resident arguments.  A child that fails
or outlives --limit ends the tool (nothing is started on the GPU after a fault or a hang); what was taken so far is in the
JSON.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 2560, 1920
BAND_ROWS = 240
#        name          kwin  lon, lat of the grid
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


def _timer(np, torch, s):
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
    return timed


def _child(band, path):
    np, torch, hip, synth = _imports()
    dt = np.float64
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    timed = _timer(np, torch, s)
    st = synth.static_fields(NX, NY, dt)
    coast = ctx.get_edges(st.landfrac, st.icefrac, rule=1, bnd=hip.SB_BND_GLOBAL)
    d_co, d_lf = dev(coast), dev(st.landfrac)
    d_cd = torch.zeros_like(d_co)
    out, fields = {}, {}
    for name, k, kind in GRIDS:
        lon, lat = _coords(np, synth, kind)
        whole = lambda: ctx.get_dist_dev(dt, NX, NY, d_co.data_ptr(), d_lf.data_ptr(), lon, lat, d_cd.data_ptr(), maxdist=180.0,
                                         kwin=k, stream=sh)
        out[f"whole_{name}"] = timed(whole)
        s.synchronize()
        fields[name] = d_cd.cpu().numpy().copy()
        if not band:
            continue
        r0 = 3 * BAND_ROWS                                               # band 3 of 8: cuts on both sides
        r1, h = r0 + BAND_ROWS, k
        fr = lambda a: np.pad(a[r0 - h:r1 + h], ((0, 0), (h, h)), mode="wrap")
        b_co, b_lf = dev(fr(coast)), dev(fr(st.landfrac))
        b_cd = torch.zeros_like(b_co)
        latf = np.ascontiguousarray(lat[r0 - h:r1 + h])
        bandcall = lambda: ctx.band_get_dist_dev(dt, NX, BAND_ROWS, h, False, False, b_co.data_ptr(), b_lf.data_ptr(), lon, latf,
                                                 b_cd.data_ptr(), k, maxdist=180.0, stream=sh)
        t = timed(bandcall)
        s.synchronize()
        got = b_cd.cpu().numpy()[h:h + BAND_ROWS, h:h + NX]
        w = out[f"whole_{name}"]["median_us"]
        t.update(equal_bits=bool(np.array_equal(got.view(np.uint8), fields[name][r0:r1].view(np.uint8))),
                 reached_cells=int(np.count_nonzero(np.abs(got) < 12000.0)),
                 over_whole=t["median_us"] / w, rows_read_over_rows=(BAND_ROWS + 2 * k) / NY)
        out[f"band_{name}"] = t
    ctx.close()
    if path:
        np.savez(path, **fields)
    print("RESULT " + json.dumps(out))


def _run(lib, what, arg, limit):
    env = dict(os.environ)
    if lib:
        env["SEABREEZE_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SEABREEZE_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, arg], env=env, capture_output=True, text=True,
                       timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{what} child for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_setup_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        _child(a.child[0] == "band", a.child[1])
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    import numpy as np
    doc = dict(tool="band_setup_cost", nx=NX, ny=NY, band_rows=BAND_ROWS, dtype="f64", rounds=[])

    def write(**more):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(doc, **more), f, indent=1)
            f.write("\n")

    try:
        with tempfile.TemporaryDirectory() as tmp:
            for i in range(a.rounds):
                doc["rounds"].append({})
                for name, lib in (("parent", a.parent_lib), ("tree", None)):
                    doc["rounds"][-1][name] = _run(lib, "band" if lib is None else "whole", os.path.join(tmp, name + ".npz"), a.limit)
                    print(f"round {i} {name}: " + json.dumps({k: round(v["median_us"], 1) for k, v in doc["rounds"][-1][name].items()}),
                          flush=True)
            fa, fb = np.load(os.path.join(tmp, "parent.npz")), np.load(os.path.join(tmp, "tree.npz"))
            doc["whole_grid_fields_equal_parent"] = {k: bool(np.array_equal(fa[k].view(np.uint8), fb[k].view(np.uint8))) for k in fa.files}
    except (SystemExit, subprocess.TimeoutExpired):
        write(incomplete=True)
        raise
    summary, outside = {}, {}
    for key in doc["rounds"][0]["parent"]:
        par = [r["parent"][key]["median_us"] for r in doc["rounds"]]
        tree = [r["tree"][key]["median_us"] for r in doc["rounds"]]
        med = sorted(tree)[len(tree) // 2]
        summary[key] = dict(parent_medians_us=par, tree_medians_us=tree, tree_median_us=med,
                            tree_over_parent=med / sorted(par)[len(par) // 2])
        if not min(par) <= med <= max(par):
            outside[key] = "slower" if med > max(par) else "faster"
    for key in (k for k in doc["rounds"][0]["tree"] if k.startswith("band_")):
        rs = [r["tree"][key] for r in doc["rounds"]]
        summary[key] = dict(medians_us=[r["median_us"] for r in rs], over_whole=[r["over_whole"] for r in rs],
                            rows_read_over_rows=rs[0]["rows_read_over_rows"], equal_bits=all(r["equal_bits"] for r in rs))
    write(summary=summary, outside_parent_range=outside)
    print(json.dumps(dict(summary=summary, outside_parent_range=outside, equal=doc["whole_grid_fields_equal_parent"])))
    if not all(doc["whole_grid_fields_equal_parent"].values()) or not all(summary[k]["equal_bits"] for k in summary if k.startswith("band_")):
        raise SystemExit("fields differ")


if __name__ == "__main__":
    main()
