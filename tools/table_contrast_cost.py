"""Cost of the contrast from device-wide summed-area tables (sb_set_table_contrast).

    python tools/table_contrast_cost.py --part fixed|board|board160|cache [--nx 2560 --ny 1920] [--n 50] [--out FILE]

Every part times whole sb_seabreeze_diag_f64_dev calls with HIP events on one torch stream (warm, median of N) and the
kernels of a call with sb_profile_begin / sb_profile_end, one profiled call at a time (median of N).  In a table call the
profile reports the row pass under k_t0 and the column pass and the query together under k_thc; the column pass alone is
the k_thc of a call on the same grid with an empty band (the query then finds no segment), the query the difference.

  fixed     the benchmark grid and mask (bench.py's: the synthetic coast, get_edges / get_dist, radii <= 16), nz levels, the
            switch off and on in one process; the table passes against their byte floor, 20 B per frame cell read and
            written once per pass, as a fraction of the measured 2-in/1-out stream rate (4.65 TB/s)
  board     a periodic checkerboard of 80 x 80 land and sea blocks, every cell in the band (radii up to 40): the path of
            the parent commit -- switch off, radius hint 32 -- against the tables
  board160  the same with 160-cell blocks (radii up to 80), the tables only
  cache     sb_set_table_window_cache off and on in turn within one process (five blocks of N / 5 warm calls each way, the
            first calls after every switch -- among them the call that searches and stores -- not timed): the whole call,
            the row pass, the column pass and the query, on the checkerboard of 80-cell blocks at 640 x 480 and at
            2560 x 1920 (4 levels) and on the grid and mask of `fixed` (56 levels); the report of the last timed call
            shows that it was answered from stored windows
u and v are uniform random numbers (the level k_wind picks depends on p alone).  Each part prints one JSON line and,
with --out, merges it into that file under its name.  Run every part under a time limit of its own.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch  # before the library: one HIP runtime (seabreeze_param_amd/hip.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seabreeze_param_amd import hip, synth  # noqa: E402

STREAM_RATE = 4.65e12       # B/s, 2-in/1-out stream on this chip
PROF = ("k_scan", "k_prep", "k_t0", "k_thc", "k_wind")


class Case:
    def __init__(self, ctx, nx, ny, nz, mask, stream):
        dt = np.float64
        self.ctx, self.nx, self.ny, self.nz, self.stream = ctx, nx, ny, nz, stream
        st = synth.static_fields(nx, ny, dt)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda")
        self.p = dev(synth.pressure_3d(st, nz, dt))
        self.u = torch.rand((nz, ny, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
        self.v = torch.rand((nz, ny, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
        self.th, self.z, self.sg = dev(synth.theta_step(st, 1, dt)), dev(st.z), dev(st.sigma)
        self.mask, self.none = dev(mask), torch.full((ny, nx), 12000.0, dtype=torch.float64, device="cuda")
        self.state = [torch.zeros((ny, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()

    def call(self, mask=None, tn=2):
        m = self.mask if mask is None else mask
        self.ctx.seabreeze_diag_dev(np.float64, 5400.0, tn, self.nx, self.ny, self.nz, 0, hip.SB_BND_GLOBAL, self.p.data_ptr(),
                                    self.u.data_ptr(), self.v.data_ptr(), self.th.data_ptr(), m.data_ptr(), self.z.data_ptr(),
                                    self.sg.data_ptr(), *[s.data_ptr() for s in self.state], stream=self.stream.cuda_stream)

    def one_call_ms(self, mask=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            a.record(self.stream)
            self.call(mask)
            b.record(self.stream)
        self.stream.synchronize()
        return a.elapsed_time(b)

    def samples(self, n, mask=None):
        """-> n warm whole-call times and n times per kernel, in us"""
        for _ in range(3):
            self.one_call_ms(mask)
        whole = np.array([self.one_call_ms(mask) for _ in range(n)]) * 1e3
        ker = {k: [] for k in PROF}
        for _ in range(n):
            self.ctx.profile_begin(1)
            with torch.cuda.stream(self.stream):
                self.call(mask)
            ms, _ = self.ctx.profile_end()
            for k in PROF:
                ker[k].append(ms[k] * 1e3)
        return whole, ker

    def measure(self, n, mask=None):
        """-> whole-call and per-kernel medians in us, the counters and the launches of the last call"""
        whole, ker = self.samples(n, mask)
        out = dict(call_us=float(np.median(whole)), call_min_us=float(whole.min()), n=n,
                   kernels_us={k: float(np.median(v)) for k, v in ker.items()})
        out["counters"] = self.ctx.last_counters()
        out["launches"] = self.ctx.last_step_report()["kernel_launches"]
        return out


def table_parts(case, n):
    """the table call, and its kernels apart"""
    on = case.measure(n)
    empty = case.measure(n, case.none)
    rows, cols = on["kernels_us"]["k_t0"], empty["kernels_us"]["k_thc"]
    cells = case.nx * case.ny
    floor_us = 2 * 20.0 * cells / STREAM_RATE * 1e6      # 20 B per frame cell read and written once
    on["table_kernels_us"] = dict(rows=rows, cols=cols, query=on["kernels_us"]["k_thc"] - cols)
    on["pass_floor_us"] = floor_us
    on["fraction_of_stream_rate"] = dict(rows=floor_us / rows, cols=floor_us / cols)
    on["empty_band_call_us"] = empty["call_us"]
    return on


def cache_parts(case, n, blocks=5):
    """the table call with the window cache off and on, in alternating blocks: medians over all blocks"""
    per = max(1, n // blocks)
    acc = {m: dict(call=[], rows=[], thc=[], cols=[], empty_call=[]) for m in ("off", "on")}
    out = {}
    for _ in range(blocks):
        for m in ("off", "on"):
            case.ctx.set_table_window_cache(m == "on")
            whole, ker = case.samples(per)
            acc[m]["call"] += list(whole); acc[m]["rows"] += ker["k_t0"]; acc[m]["thc"] += ker["k_thc"]
            out[m] = dict(report=case.ctx.table_cache_report(), counters=case.ctx.last_counters(),
                          launches=case.ctx.last_step_report()["kernel_launches"])
            whole, ker = case.samples(per, case.none)
            acc[m]["empty_call"] += list(whole); acc[m]["cols"] += ker["k_thc"]
    case.ctx.set_table_window_cache(False)
    for m in ("off", "on"):
        med = {k: float(np.median(v)) for k, v in acc[m].items()}
        out[m].update(call_us=med["call"], call_min_us=float(np.min(acc[m]["call"])), n=len(acc[m]["call"]),
                      empty_band_call_us=med["empty_call"],
                      table_kernels_us=dict(rows=med["rows"], cols=med["cols"], query=med["thc"] - med["cols"]))
    out["saved_us"] = out["off"]["call_us"] - out["on"]["call_us"]
    return out


def board(nx, ny, w):
    x, y = np.arange(nx)[None, :], np.arange(ny)[:, None]
    return np.where(((x // w) + (y // w)) % 2 == 0, 100.0, -100.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=("fixed", "board", "board160", "cache"))
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--nx", type=int, default=2560)
    ap.add_argument("--ny", type=int, default=1920)
    ap.add_argument("--nz", type=int, default=0, help="levels (default: 56 for fixed, 4 for the checkerboards)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    nx, ny = a.nx, a.ny
    ctx = hip.Context(0)
    stream = torch.cuda.Stream()
    res = dict(tool="table_contrast_cost", part=a.part, nx=nx, ny=ny, dtype="f64")
    if a.part == "cache":
        ctx.set_table_contrast(True)
        for name, cnx, cny in (("board", 640, 480), ("board", nx, ny), ("fixed", nx, ny)):
            if name == "fixed":
                st = synth.static_fields(cnx, cny, np.float64)
                mask, nz = ctx.get_dist(ctx.get_edges(st.landfrac, st.icefrac), st.landfrac, st.lon, st.lat), a.nz or 56
            else:
                mask, nz = board(cnx, cny, 80), a.nz or 4
            res[f"{name}_{cnx}x{cny}"] = dict(nz=nz, **cache_parts(Case(ctx, cnx, cny, nz, mask, stream), a.n))
    elif a.part == "fixed":
        nz = a.nz or 56
        st = synth.static_fields(nx, ny, np.float64)
        cdist = ctx.get_dist(ctx.get_edges(st.landfrac, st.icefrac), st.landfrac, st.lon, st.lat)
        case = Case(ctx, nx, ny, nz, cdist, stream)
        res["nz"] = nz
        res["off"] = case.measure(a.n)
        ctx.set_table_contrast(True)
        res["on"] = table_parts(case, a.n)
        res["added_us"] = res["on"]["call_us"] - res["off"]["call_us"]
    else:
        nz = a.nz or 4
        w = 80 if a.part == "board" else 160
        case = Case(ctx, nx, ny, nz, board(nx, ny, w), stream)
        res["nz"], res["block"] = nz, w
        if a.part == "board":
            # the parent commit's behaviour first: switch off, radius hint 32 (fp64: the tile kernel, beyond 32 the global path)
            ctx.set_search_radius_hint(32)
            first_ms = case.one_call_ms()
            res["off_hint32_first_call_ms"] = first_ms
            n_off = a.n if first_ms < 20.0 else (10 if first_ms < 1000.0 else 0)
            if n_off:
                res["off_hint32"] = case.measure(n_off)
            ctx.set_search_radius_hint(16)
        ctx.set_table_contrast(True)
        res["on"] = table_parts(case, a.n)
        if "off_hint32" in res:
            res["ratio_call"] = res["off_hint32"]["call_us"] / res["on"]["call_us"]
            res["ratio_contrast"] = res["off_hint32"]["kernels_us"]["k_thc"] / (res["on"]["kernels_us"]["k_t0"] + res["on"]["kernels_us"]["k_thc"])
    print(json.dumps(res))
    if a.out:
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres["cache" if a.part == "cache" else f"{a.part}_{nx}x{ny}"] = res
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
