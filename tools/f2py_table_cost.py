"""Cost of the table contrast for the f2py flavour (sb_set_table_contrast_f2py).

    python tools/f2py_table_cost.py [--nx 2560 --ny 1920 --nps 8] [--n 50] [--out FILE --key NAME]

2560 x 1920, fp32, no ghost cells; the mask a periodic checkerboard of 80-cell land and sea blocks, every cell in the band:
radii up to 40 (the case of tools/table_contrast_cost.py --part board and profiles/table_contrast_cost.json).  All parts in
one process, each the median of N warm calls between two HIP events on one torch stream, in us, with the per-kernel
averages of sb_profile_begin / sb_profile_end over the same number of further calls beside it:

  f2py_off      sb_diag_f32_dev with both switches off, radius hint 32: the flavour's five launches, cells beyond the LDS
                reach on the global-memory path
  f2py_on       the same call with sb_set_table_contrast and sb_set_table_contrast_f2py on: six launches
  f2py_on_kept  ... and sb_set_table_window_cache beside them (the first call fills; the timed calls read W)
  host_table    sb_seabreeze_diag_f32_dev, SB_BND_GLOBAL, on the same 2-D fields with the table switch on: the host-model
                table call (its k_wind walks a 3-D pressure field of nps levels; the f2py flavour's p is one column, so
                compare k_scan, k_prep, the row pass [k_t0] and column pass + query [k_thc], not the whole call)

Expectation, stated before measuring: the row pass of f2py_on moves the bytes of host_table's plus one t0 plane written
(the workspace plane; rows 1 .. nlats - 1 of `output` a second time) and saves f2py_off's k_t0, which reads three planes
and writes those two; column pass and query as host_table's.  u and v are uniform random numbers.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=2560)
    ap.add_argument("--ny", type=int, default=1920)
    ap.add_argument("--nps", type=int, default=8)
    ap.add_argument("--block", type=int, default=80)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    nx, ny, nps, dt = a.nx, a.ny, a.nps, np.float32
    ctx = hip.Context(0)
    ctx.set_search_radius_hint(32)                       # the largest an LDS kernel is instantiated for
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")

    st = synth.static_fields(nx, ny, dt)
    p1, p3 = dev(synth.pressure_1d(nps, dt)), dev(synth.pressure_3d(st, nps, dt))
    u = torch.rand((nps, ny, nx), dtype=torch.float32, device="cuda") * 16.0 - 8.0
    v = torch.rand((nps, ny, nx), dtype=torch.float32, device="cuda") * 16.0 - 8.0
    x, y = np.arange(nx)[None, :], np.arange(ny)[:, None]
    mask = dev(np.where(((x // a.block) + (y // a.block)) % 2 == 0, 100.0, -100.0))
    th, z, sg = dev(synth.theta_step(st, 1, dt)), dev(st.z), dev(st.sigma)
    state = [torch.zeros((ny, nx), dtype=torch.float32, device="cuda") for _ in range(4)]
    out4 = torch.zeros((4, ny, nx), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def f2py_call(tn=2):
        ctx.diag_dev(dt, tn, nps, nx, ny, p1.data_ptr(), z.data_ptr(), sg.data_ptr(), th.data_ptr(), v.data_ptr(), u.data_ptr(),
                     mask.data_ptr(), *[s.data_ptr() for s in state[:3]], out4.data_ptr(), stream=sh)

    def host_call(tn=2):
        ctx.seabreeze_diag_dev(dt, 1440.0, tn, nx, ny, nps, 0, hip.SB_BND_GLOBAL, p3.data_ptr(), u.data_ptr(), v.data_ptr(),
                               th.data_ptr(), mask.data_ptr(), z.data_ptr(), sg.data_ptr(), *[s.data_ptr() for s in state], stream=sh)

    def one_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def measure(fn):
        first = one_ms(fn)
        n = a.n if first < 20.0 else 10                  # (a call of tens of milliseconds: ten warm ones tell enough)
        for _ in range(2):
            one_ms(fn)
        t = np.array([one_ms(fn) for _ in range(n)]) * 1e3
        ctx.profile_begin(n)
        for _ in range(n):
            fn()
        stream.synchronize()
        ms, ncalls = ctx.profile_end()
        return dict(us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n, first_call_ms=first,
                    kernels_us={k: 1e3 * val for k, val in ms.items()}, profiled_calls=ncalls,
                    counters=ctx.last_counters(), step_report=ctx.last_step_report(), cache=ctx.table_cache_report())

    res = dict(tool="f2py_table_cost", nx=nx, ny=ny, nps=nps, block=a.block, dtype="f32")
    res["f2py_off"] = measure(f2py_call)
    ctx.set_table_contrast(True)
    ctx.set_table_contrast_f2py(True)
    res["f2py_on"] = measure(f2py_call)
    ctx.set_table_window_cache(True)
    res["f2py_on_kept"] = measure(f2py_call)
    ctx.set_table_window_cache(False)
    ctx.set_table_contrast_f2py(False)
    res["host_table"] = measure(host_call)
    res["ratio_off_over_on"] = res["f2py_off"]["us"] / res["f2py_on"]["us"]
    print(json.dumps(res))
    if a.out:
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.key or "this_build"] = res
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
