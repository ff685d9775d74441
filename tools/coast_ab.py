"""The coast setup against a library built from the parent commit: the same bits, and the same time.

    python tools/coast_ab.py --parent-lib PATH [--rounds 2] [--out profiles/coast_common_ab.json]

The parent library is an A/B build from a checkout of the parent commit by the Makefile's recipe (csrc/Makefile, BUILD= /
OUT=).  A library is loaded through SEABREEZE_HIP_LIB, so each one runs in fresh child processes of this tool, the libraries
taking turns; a child that fails or outlives --limit ends the tool (subprocess.run kills the child when its timeout
expires: nothing is started on the GPU after a fault or a hang); what was taken so far is in the JSON.

Identity.  One child per library writes the output fields of a fixed list of small cases, in both precisions, to an .npz:
one case per kernel and path of get_edges, get_dist (the shapes of tests/test_setup_gpu.py and tests/test_dist_wide_gpu.py;
every kernel with coordinates that allow the cuts and with shuffled ones that forbid them), get_edges_um, get_dist_um and
get_dist_um_win (the grids of tests/test_um_dist_win_gpu.py).  This process asserts np.array_equal field by field: edges as
masks, distances bit for bit -- the same library routines in the same order, so nothing less is accepted.

Time.  Median of warm, event-timed `_dev` calls on one torch stream (device-resident arguments, up to 50 enqueues; an
interval holds the call's launches and the gap to the event before), at the sizes the project quotes: 2560 x 1920 fp64 and
5120 x 3840 fp32 get_edges and get_dist with the automatic window; 2560 x 1920 fp64 get_dist at kwin = 40 and 100;
get_dist_um with 15 ghost cells and get_dist_um_win at 113 on the grid of tools/um_dist_win_cost.py.  The yardstick is the
parent library in the same job and the margin the spread between the parent's own rounds: a case whose median over this
tree's rounds lies outside the parent's range is listed under `outside_parent_range`.  The JSON keeps every round.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# get_dist: (nx, ny, kwin) -- k_dist_bits_small, k_dist_bits<32>, <64>, k_dist (bytes), k_dist_wide
DIST_SHAPES = ((200, 90, 5), (130, 64, 15), (64, 33, 31), (512, 40, 15), (330, 70, 31), (40, 30, 31),
               (330, 70, 32), (300, 64, 255), (192, 48, 112))
EVERY_HIT = ((420, 40, 9), (420, 40, 40))                        # regional longitudes, shuffled latitudes
EDGE_SHAPES = ((258, 7), (5, 5))
UM_HALOS = ((0, 0), (31, 7))
# get_dist_um_win: (window, halo, grid, nx, ny, mask seed) as tests/test_um_dist_win_gpu.py builds them
UM_WIN = (((32, 0), (3, 2), 2, 100, 72, 11), ((40, 33), (1, 1), 1, 100, 72, 11), ((255, 3), (0, 0), 2, 70, 50, 21))


def _noise_mask(synth, np, nx, ny, seed, dt, frac=False):
    """tests/test_setup_gpu.py's mask: coast cells everywhere, also across the seam and at the poles"""
    r = synth.hash_uniform((ny, nx), 3, seed)
    s = r + np.roll(r, 1, 1) + np.roll(r, 1, 0) + np.roll(r, -1, 1)
    land = np.round(np.clip((s - 1.6) / 1.2, 0, 1) * 8) / 8 if frac else (s > 2.2).astype(np.float64)
    ice = np.where(synth.hash_uniform((ny, nx), 4, seed) > 0.9, 0.35, 0.0)
    return np.ascontiguousarray(land, dt), np.ascontiguousarray(ice, dt)


def _imports():
    import numpy as np
    import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from seabreeze_param_amd import hip, synth
    import um_setup_ref as ur
    return np, torch, hip, synth, ur


def _child_identity(path):
    np, torch, hip, synth, ur = _imports()
    ctx = hip.Context(0)
    out = {}
    for p, dt in (("f64", np.float64), ("f32", np.float32)):
        for nx, ny in EDGE_SHAPES:
            land, ice = _noise_mask(synth, np, nx, ny, 41, dt, frac=True)
            for rule, bnd in ((0, hip.SB_BND_WRAPPER), (1, hip.SB_BND_GLOBAL), (0, hip.SB_BND_GLOBAL), (1, hip.SB_BND_WRAPPER)):
                out[f"{p}/edges/{nx}x{ny}/rule{rule}/bnd{bnd}"] = ctx.get_edges(land, ice, rule=rule, bnd=bnd) > 0
        for nx, ny, k in DIST_SHAPES:
            lon, lat = synth.grid(nx, ny)
            land, ice = _noise_mask(synth, np, nx, ny, 11, dt)
            coast = ctx.get_edges(land, ice)
            coords = {"cuts": (lon, lat), "nocuts": (np.random.default_rng(5).permutation(lon), np.random.default_rng(6).permutation(lat))}
            for name, (lo, la) in coords.items():
                for maxdist in (180.0, 900.0):                   # the sweep-time reset at two thresholds
                    out[f"{p}/dist/{nx}x{ny}/k{k}/{name}/maxdist{maxdist:g}"] = ctx.get_dist(
                        coast, land, lo.astype(dt), la.astype(dt), maxdist=maxdist, kwin=k)
        for nx, ny, k in EVERY_HIT:
            lon, lat = synth.grid(nx, ny)
            land, ice = _noise_mask(synth, np, nx, ny, 21, dt)
            coast = ctx.get_edges(land, ice)
            coords = {"regional": (np.linspace(100.0, 160.0, nx), lat), "lat-shuffled": (lon, np.random.default_rng(6).permutation(lat))}
            for name, (lo, la) in coords.items():
                out[f"{p}/dist/{nx}x{ny}/k{k}/{name}"] = ctx.get_dist(coast, land, lo.astype(dt), la.astype(dt), maxdist=400.0, kwin=k)
        land, ice = ur.noise_mask(258, 7, 41, dt, frac=True)
        lf_l, ice_l, _ = ur.coast_of(land, ice, 2, 5)
        out[f"{p}/edges_um/258x7/halo2x5"] = ctx.get_edges_um(lf_l, ice_l, 2, 5) > 0
        grids = sorted(ur.GRIDS)
        for hi, hj in UM_HALOS:
            lat, lon = ur.grid_named("dateline", 100, 72, dt)
            land, ice = ur.noise_mask(100, 72, 11, dt)
            _, _, coast_l = ur.coast_of(land, ice, hi, hj)
            out[f"{p}/dist_um/halo{hi}x{hj}"] = ctx.get_dist_um(coast_l, land, lat, lon, hi, hj, maxdist=180.0)
        for (wi, wj), (hi, hj), g, nx, ny, seed in UM_WIN:
            lat, lon = ur.grid_named(grids[g], nx, ny, dt)
            for maker in (ur.noise_mask, ur.sparse_mask):
                land, ice = maker(nx, ny, seed if maker is ur.noise_mask else seed + 1, dt)
                _, _, coast_l = ur.coast_of(land, ice, hi, hj)
                out[f"{p}/dist_um_win/{wi}x{wj}/halo{hi}x{hj}/{maker.__name__}"] = ctx.get_dist_um_win(
                    coast_l, land, lat, lon, hi, hj, wi, wj, maxdist=180.0)
    ctx.close()
    np.savez(path, **out)
    print("RESULT " + json.dumps(dict(fields=len(out))))


def _child_time():
    np, torch, hip, synth, ur = _imports()
    ctx = hip.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
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
    for p, dt, nx, ny, windows in (("f64", np.float64, 2560, 1920, (-1, 40, 100)), ("f32", np.float32, 5120, 3840, (-1,))):
        st = synth.static_fields(nx, ny, dt)
        d_lf, d_ice = dev(st.landfrac), dev(st.icefrac)
        d_co, d_cd = torch.zeros_like(d_lf), torch.zeros_like(d_lf)
        torch.cuda.synchronize()
        out[f"get_edges_{p}_{nx}x{ny}"] = timed(lambda: ctx.get_edges_dev(dt, nx, ny, d_lf.data_ptr(), d_ice.data_ptr(), d_co.data_ptr(), stream=sh))
        for k in windows:
            out[f"get_dist_{p}_{nx}x{ny}_k{'auto' if k < 0 else k}"] = timed(
                lambda: ctx.get_dist_dev(dt, nx, ny, d_co.data_ptr(), d_lf.data_ptr(), st.lon, st.lat, d_cd.data_ptr(), maxdist=180.0,
                                         kwin=k, stream=sh))
        del d_lf, d_ice, d_co, d_cd
    nx, ny, h, dt = 2560, 1920, 15, np.float64                           # tools/um_dist_win_cost.py's grid
    st_l = synth.static_fields(nx + 2 * h, ny + 2 * h, dt)
    d_co = dev(ctx.get_edges_um(st_l.landfrac, st_l.icefrac, h, h))
    d_lf = dev(st_l.landfrac[h:h + ny, h:h + nx])
    d_cd = torch.zeros_like(d_co)
    for name, deg, w in (("get_dist_um_f64_halo15", 0.036, 15), ("get_dist_um_win_f64_w113", 0.0135, 113)):
        lat, lon = ur.grid_named("dateline", nx, ny, dt, dlon=deg, dlat=deg)
        d_la, d_lo = dev(lat), dev(lon)
        torch.cuda.synchronize()
        args = (d_co.data_ptr(), d_lf.data_ptr(), d_la.data_ptr(), d_lo.data_ptr(), d_cd.data_ptr())
        if w == h:
            out[name] = timed(lambda: ctx.get_dist_um_dev(dt, nx, ny, h, h, *args, maxdist=180.0, stream=sh))
        else:
            out[name] = timed(lambda: ctx.get_dist_um_win_dev(dt, nx, ny, h, h, w, w, *args, maxdist=180.0, stream=sh))
    ctx.close()
    print("RESULT " + json.dumps(out))


def _run(lib, what, arg, limit):
    env = dict(os.environ)
    if lib:
        env["SEABREEZE_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SEABREEZE_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what] + ([arg] if arg else []), env=env,
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{what} child for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coast_common_ab.json"))
    a = ap.parse_args()
    if a.child is not None:
        _child_identity(a.child[1]) if a.child[0] == "identity" else _child_time()
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    import numpy as np
    libs = (("parent", a.parent_lib), ("tree", None))
    doc = dict(tool="coast_ab", identity={}, rounds=[])

    def write(**more):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(doc, **more), f, indent=1)
            f.write("\n")

    try:
        with tempfile.TemporaryDirectory() as tmp:
            for name, lib in libs:
                _run(lib, "identity", os.path.join(tmp, name + ".npz"), a.limit)
            fa, fb = (np.load(os.path.join(tmp, name + ".npz")) for name, _ in libs)
            assert sorted(fa.files) == sorted(fb.files)
            differ = [k for k in fa.files if fa[k].dtype != fb[k].dtype or not np.array_equal(fa[k], fb[k])]
            doc["identity"] = dict(fields=len(fa.files), cells=int(sum(fa[k].size for k in fa.files)), differ=differ)
        print(f"identity: {len(fa.files)} fields, {len(differ)} differ", flush=True)
        if differ:
            raise SystemExit(f"fields differ from the parent's: {differ}")
        for i in range(a.rounds):
            doc["rounds"].append({})
            for name, lib in libs:
                doc["rounds"][-1][name] = _run(lib, "time", None, a.limit)
                print(f"round {i} {name}: " + json.dumps({k: round(v["median_us"], 1) for k, v in doc["rounds"][-1][name].items()}), flush=True)
    except (SystemExit, subprocess.TimeoutExpired):
        write(incomplete=True)
        raise
    summary, outside = {}, {}
    for key in doc["rounds"][0]["tree"]:
        par = [r["parent"][key]["median_us"] for r in doc["rounds"]]
        tree = [r["tree"][key]["median_us"] for r in doc["rounds"]]
        med = sorted(tree)[len(tree) // 2]
        summary[key] = dict(parent_medians_us=par, tree_medians_us=tree, tree_median_us=med, tree_over_parent=med / sorted(par)[len(par) // 2])
        if not min(par) <= med <= max(par):
            outside[key] = "slower" if med > max(par) else "faster"
    write(summary=summary, outside_parent_range=outside)
    print(json.dumps(dict(identity=doc["identity"], summary=summary, outside_parent_range=outside)))


if __name__ == "__main__":
    main()
