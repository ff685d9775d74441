"""Cost of search_radius next to get_dist, the setup call it follows.

    python tools/search_radius_cost.py [--n 20] [--out profiles/search_radius_cost.json]

One process, fp64, device-resident arguments, HIP events on one torch stream, warm, the median of N enqueues in us (an
interval holds the call's launches, its two small memsets and the gap to the event before):

  bench      the benchmark grid and mask: 2560 x 1920, synth.static_fields' coast and coordinates, get_dist with kwin = 15;
             sb_get_dist_f64_dev and sb_search_radius_f64_dev (SB_BND_GLOBAL) on it
  regional   the 0.0135-degree regional case (tools/dist_wide_cost.py: the same coast at lon 10 + 0.0135 j,
             lat 60 + 0.0135 i), the mask from get_dist with kwin = 113: the whole grid (SB_BND_GLOBAL), and one band of
             eight (rows 720 .. 959, a frame of 113 ghost cells, both sides cut) with sb_band_search_radius_f64_dev

and for each search_radius case the summary, the band cells per contrast regime (hip.contrast_regimes) and the bytes the
three passes move by the count of DESIGN 2.6b: 8 B (fp64 mask) + 2 B (row distance) per cell of the rows read, the two bit
planes, and the column walk's loads (one 16-bit distance and one plane word per row folded, summed over the band cells
from the histogram).
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

NX, NY, NHIST = 2560, 1920, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_radius_cost.json"))
    a = ap.parse_args()
    dt = np.float64
    ctx = hip.Context(0)
    s = torch.cuda.Stream()
    sh = s.cuda_stream
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")

    def measure(fn):
        with torch.cuda.stream(s):
            fn()                                                 # workspace, coordinate tables, code
            s.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); fn(); e1.record(s)
            s.synchronize()
            one = e0.elapsed_time(e1) * 1e-3                     # seconds: a slow call is repeated less often
            n = int(min(a.n, max(5, 2.0 / max(one, 1e-6))))
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for e0, e1 in ev:
                e0.record(s); fn(); e1.record(s)
            s.synchronize()
        t = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])
        return dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n)

    st = synth.static_fields(NX, NY, dt)
    coast = ctx.get_edges(st.landfrac, st.icefrac)
    d_co, d_lf = dev(coast), dev(st.landfrac)
    d_rad = torch.zeros((NY, NX), dtype=torch.int32, device="cuda")
    d_sum = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_hist = torch.zeros(NHIST, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def radius_case(call, rows_read, nx_read, ny_int):
        r = measure(call)
        summ, hist = d_sum.cpu().tolist(), d_hist.cpu().numpy()
        steps = int(sum(k * int(c) for k, c in enumerate(hist) if k >= 1))      # (the last bin counted at its lower edge)
        planes = 2 * rows_read * ((nx_read + 63) // 64) * 8
        r.update(summary=dict(band_cells=summ[0], with_radius=summ[1], without_window=summ[2], max_radius=summ[3]),
                 regimes=hip.contrast_regimes(hist),
                 bytes=dict(bits_pass=8 * rows_read * nx_read + planes, rows_pass=planes // 2 + 2 * rows_read * nx_read,
                            cols_walk=2 * steps * (2 + 8) + summ[0] * (2 + 8), radius_plane=4 * nx_read * ny_int))
        return r

    res = dict(tool="search_radius_cost", dtype="f64", nx=NX, ny=NY, nhist=NHIST)
    coords = {"bench": (st.lon, st.lat, 15), "regional": (10.0 + 0.0135 * np.arange(NX), 60.0 + 0.0135 * np.arange(NY), 113)}
    for name, (lon, lat, k) in coords.items():
        d_cd = torch.zeros((NY, NX), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        out = dict(kwin=k)
        out["get_dist"] = measure(lambda: ctx.get_dist_dev(dt, NX, NY, d_co.data_ptr(), d_lf.data_ptr(), lon, lat, d_cd.data_ptr(),
                                                           maxdist=180.0, kwin=k, stream=sh))
        out["search_radius"] = radius_case(
            lambda: ctx.search_radius_dev(dt, NX, NY, 0, hip.SB_BND_GLOBAL, d_cd.data_ptr(), d_rad.data_ptr(), d_sum.data_ptr(),
                                          d_hist.data_ptr(), NHIST, maxdist=180.0, stream=sh), NY, NX, NY)
        if name == "regional":
            h, r0, r1 = 113, 720, 960
            frame = torch.zeros((r1 - r0 + 2 * h, NX + 2 * h), dtype=torch.float64, device="cuda")
            frame[:, h:h + NX] = d_cd[r0 - h:r1 + h]             # (the east-west ghost columns are never read)
            d_rb = torch.zeros((r1 - r0, NX), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            out["band_of_eight"] = dict(halo=h, rows=[r0, r1])
            out["band_of_eight"]["band_search_radius"] = radius_case(
                lambda: ctx.band_search_radius_dev(dt, NX, r1 - r0, h, False, False, frame.data_ptr(), d_rb.data_ptr(),
                                                   d_sum.data_ptr(), d_hist.data_ptr(), NHIST, maxdist=180.0, stream=sh),
                r1 - r0 + 2 * h, NX, r1 - r0)
            # the band against its rows of the whole grid: equal wherever the whole grid's radius is within reach of the
            # band's ghost rows (halo + rows to the nearer cut), -1 where it is not -- no other difference is expected
            whole, band = d_rad.cpu().numpy()[r0:r1], d_rb.cpu().numpy()
            y = np.arange(r1 - r0)[:, None]
            beyond = whole > np.minimum(y, r1 - r0 - 1 - y) + h
            differ = band != whole
            out["band_of_eight"]["against_whole_grid_rows"] = dict(
                cells_that_differ=int(differ.sum()), cells_beyond_the_reach=int(beyond.sum()),
                all_of_them_minus_one_in_the_band=bool((band[beyond] == -1).all()),
                differ_only_beyond_the_reach=bool(np.array_equal(differ, beyond)),
                whole_grid_radii_beyond_the_reach=sorted(set(int(v) for v in whole[beyond])))
        res[name] = out
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
