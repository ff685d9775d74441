"""Cost of get_dist at search windows beyond 31 cells (k_dist_wide).

    python tools/dist_wide_cost.py [--parent-lib PATH] [--nocut-lib PATH] [--rounds 2] [--out profiles/dist_wide_cost.json]

times sb_get_dist_f64_dev with HIP events on one torch stream (device-resident arguments, warm, median of repeated
enqueues; an interval holds the call's two launches and the gap to the event before):
  * the bench grid (2560 x 1920, synth.static_fields' coast and coordinates), kwin = 15 (k_dist_bits, the control),
    40, 100 (k_dist_wide; k_dist in a library built from the parent commit), 120, 200 (k_dist_wide only);
  * a regional grid of the same size and coast at 0.0135 degrees (lon 10 + 0.0135 j, lat 60 + 0.0135 i), kwin = 113, with the
    per-target column cut and, in a library built with -DSB_DIST_NO_INNER_CUT, without it.
The other libraries are A/B builds by the Makefile's recipe (csrc/Makefile, BUILD= / OUT= / EXTRA=), the parent's from a
checkout of the parent commit.  A library is loaded through SEABREEZE_HIP_LIB, so each one is measured in fresh child
processes of this tool, the libraries taking turns `--rounds` times; the JSON keeps every round.  A window a library
refuses is recorded as refused.  A child that fails or outlives --limit ends the tool (subprocess.run kills the child when
its timeout expires: nothing is started on the GPU after a fault or a hang); the rounds taken so far are in the JSON.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 2560, 1920
GLOBAL_K = (15, 40, 100, 120, 200)
REGIONAL_K = 113


def _child(cases):
    import numpy as np
    import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)
    sys.path.insert(0, ROOT)
    from seabreeze_param_amd import hip, synth

    dt = np.float64
    ctx = hip.Context(0)
    st = synth.static_fields(NX, NY, dt)
    coast = ctx.get_edges(st.landfrac, st.icefrac)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    d_co, d_lf = dev(coast), dev(st.landfrac)
    d_cd = torch.zeros((NY, NX), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    coords = {"global": (st.lon, st.lat),
              "regional": (10.0 + 0.0135 * np.arange(NX), 60.0 + 0.0135 * np.arange(NY))}
    s = torch.cuda.Stream()
    out = {}
    for grid, k in cases:
        lon, lat = coords[grid]
        fn = lambda: ctx.get_dist_dev(dt, NX, NY, d_co.data_ptr(), d_lf.data_ptr(), lon, lat, d_cd.data_ptr(),
                                      maxdist=180.0, kwin=k, stream=s.cuda_stream)
        key = f"{grid}_k{k}"
        try:
            with torch.cuda.stream(s):
                fn()                                             # the tables' upload, the workspace
                s.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s); fn(); b.record(s)
                s.synchronize()
                one = a.elapsed_time(b) * 1e-3                   # seconds: how many repeats two seconds hold
                n = int(min(50, max(5, 2.0 / max(one, 1e-6))))
                for _ in range(2):
                    fn()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
                for a, b in ev:
                    a.record(s); fn(); b.record(s)
                s.synchronize()
            t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
            cd = d_cd.cpu().numpy()
            out[key] = dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n,
                            reached_frac=float(np.mean(cd < 12000.0)), checksum=float(np.abs(cd[cd < 12000.0]).sum()))
        except hip.SeabreezeHipError as e:
            out[key] = dict(refused=str(e))
    ctx.close()
    print("RESULT " + json.dumps(out))


def _run(lib, cases, limit):
    env = dict(os.environ)
    if lib:
        env["SEABREEZE_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SEABREEZE_HIP_LIB", None)
    spec = ",".join(f"{g}:{k}" for g, k in cases)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec], env=env, capture_output=True, text=True,
                       timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"child for {lib or 'this tree'} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default=None, help="libseabreeze_hip.so built from the parent commit")
    ap.add_argument("--nocut-lib", default=None, help="this tree built with EXTRA=-DSB_DIST_NO_INNER_CUT")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take (k_dist at kwin = 100: of the order of a second per call)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_wide_cost.json"))
    a = ap.parse_args()
    if a.child is not None:
        _child([(g, int(k)) for g, k in (c.split(":") for c in a.child.split(","))])
        return
    plans = [("tree", None, [("global", k) for k in GLOBAL_K] + [("regional", REGIONAL_K)])]
    if a.parent_lib:
        plans.append(("parent", a.parent_lib, [("global", 15), ("global", 40), ("global", 100), ("global", 120)]))
    if a.nocut_lib:
        plans.append(("no_inner_cut", a.nocut_lib, [("regional", REGIONAL_K)]))
    rounds = []

    def write(**more):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="dist_wide_cost", nx=NX, ny=NY, dtype="f64", maxdist_km=180.0, **more, rounds=rounds), f, indent=1)
            f.write("\n")

    for i in range(a.rounds):
        rounds.append({})
        for name, lib, cases in plans:
            try:
                rounds[-1][name] = _run(lib, cases, a.limit)
            except (SystemExit, subprocess.TimeoutExpired):
                write(incomplete=f"round {i}, {name}")
                raise
            print(f"round {i} {name}: " + json.dumps({k: v.get("median_us", "refused") for k, v in rounds[-1][name].items()}), flush=True)
    best = {}
    for name, _, cases in plans:
        for g, k in cases:
            key = f"{g}_k{k}"
            runs = [r[name][key] for r in rounds]
            best.setdefault(name, {})[key] = (runs[0] if "refused" in runs[0] else
                                              dict(median_us=sorted(x["median_us"] for x in runs)[len(runs) // 2],
                                                   medians_us=[x["median_us"] for x in runs]))
    ratios = {}
    if a.parent_lib:
        for k in (15, 40, 100):
            ratios[f"global_k{k}_parent_over_tree"] = best["parent"][f"global_k{k}"]["median_us"] / best["tree"][f"global_k{k}"]["median_us"]
    if a.nocut_lib:
        ratios["regional_nocut_over_cut"] = best["no_inner_cut"][f"regional_k{REGIONAL_K}"]["median_us"] / best["tree"][f"regional_k{REGIONAL_K}"]["median_us"]
    write(summary=best, ratios=ratios)
    print(json.dumps(dict(summary=best, ratios=ratios)))


if __name__ == "__main__":
    main()
