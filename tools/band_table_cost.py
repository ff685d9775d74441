"""Cost of the table contrast in a band step (sb_set_table_contrast_bands; DESIGN.md sections 2.4d and 5.1).

    python tools/band_table_cost.py [--parent] [--nx 2560 --ny 240 --nz 56 --halo 113] [--n 50] [--out FILE --key NAME]

One band of eight of the 0.0135-degree regional case: 2560 x 240 interior cells, 56 levels, fp64, a ghost width of 113, on
a one-rank communicator (RCCL loaded, no neighbour: the exchange is the local ghost fill, the all-gather a note in the
gathered set) -- the launches, streams, events and joins of a multi-rank step without the wire.  The mask is a periodic
checkerboard of 80-cell land and sea blocks over the frame, every cell in the band: radii up to 40, as
tools/table_contrast_cost.py --part board.  All parts in one process, each the median of N warm calls between two HIP
events on one torch stream, in us:

  band_on     (a) sb_band_seabreeze_diag_f64_dev with sb_set_table_contrast and sb_set_table_contrast_bands on
  band_off    (b) the same band step with the new switch off: the tile kernel, cells beyond radius 32 on the global path
  whole_table (c) the plain whole-call table path (sb_seabreeze_diag_f64_dev, SB_BND_HALO, no gathered moments) on the same
              ghost-celled frame
  ghost_fill  (d) sb_swap_bounds_f64_dev of theta alone: what the table band step puts on the communication stream

--parent: parts (b) and (c) only and no call of the new switch -- for a library built from the parent commit
(SEABREEZE_HIP_LIB=...), run twice in the same job: its run-to-run spread is the margin within which (b) and (c) of this
build count as unchanged.  u and v are uniform random numbers (the level k_wind picks depends on p alone).
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
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--nx", type=int, default=2560)
    ap.add_argument("--ny", type=int, default=240)
    ap.add_argument("--nz", type=int, default=56)
    ap.add_argument("--halo", type=int, default=113)
    ap.add_argument("--block", type=int, default=80)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--key", default="")
    a = ap.parse_args()
    nx, ny, nz, h, dt = a.nx, a.ny, a.nz, a.halo, np.float64
    ctx = hip.Context(0)
    ctx.comm_init(hip.comm_unique_id(), 0, 1)
    ctx.set_search_radius_hint(32)                       # the largest an LDS kernel is instantiated for
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to("cuda")

    st = synth.static_fields(nx + 2 * h, ny + 2 * h, dt)             # the fields on the frame; p, u, v on its interior
    core = (slice(None), slice(h, h + ny), slice(h, h + nx))
    p = dev(synth.pressure_3d(st, nz, dt)[core])
    u = torch.rand((nz, ny, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
    v = torch.rand((nz, ny, nx), dtype=torch.float64, device="cuda") * 16.0 - 8.0
    x, y = np.arange(-h, nx + h)[None, :], np.arange(-h, ny + h)[:, None]
    mask = dev(np.where(((x // a.block) + (y // a.block)) % 2 == 0, 100.0, -100.0))
    th, z, sg = dev(synth.theta_step(st, 1, dt)), dev(st.z), dev(st.sigma)
    state = [torch.zeros((ny, nx), dtype=torch.float64, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    fields = (p.data_ptr(), u.data_ptr(), v.data_ptr(), th.data_ptr(), mask.data_ptr(), z.data_ptr(), sg.data_ptr(),
              *[s.data_ptr() for s in state])

    def band_step(tn=2):
        ctx.band_seabreeze_diag_dev(dt, 5400.0, tn, nx, ny, nz, h, *fields, sh)

    def whole_call(tn=2):
        ctx.seabreeze_diag_dev(dt, 5400.0, tn, nx, ny, nz, h, hip.SB_BND_HALO, *fields, stream=sh)

    def ghost_fill():
        ctx.swap_bounds_dev(dt, th.data_ptr(), nx, ny, h, sh)

    def one_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def measure(fn, report=True):
        first = one_ms(fn)
        n = a.n if first < 20.0 else 10                  # (a call of tens of milliseconds: ten warm ones tell enough)
        for _ in range(2):
            one_ms(fn)
        t = np.array([one_ms(fn) for _ in range(n)]) * 1e3
        out = dict(us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), n=n, first_call_ms=first)
        if report:
            out["counters"] = ctx.last_counters()
            out["step_report"] = ctx.last_step_report()
        return out

    res = dict(tool="band_table_cost", parent=bool(a.parent), nx=nx, ny=ny, nz=nz, halo=h, block=a.block, dtype="f64",
               frame=[nx + 2 * h, ny + 2 * h])
    ghost_fill()                                         # theta's ghost cells as every band step leaves them
    ctx.synchronize()
    ctx.set_table_contrast(True)
    if not a.parent:
        ctx.set_table_contrast_bands(True)
        res["band_on"] = measure(band_step)
        ctx.set_table_contrast_bands(False)
    res["band_off"] = measure(band_step)                 # (sb_set_table_contrast alone: a band step ignores it)
    res["whole_table"] = measure(whole_call)
    if not a.parent:
        res["ghost_fill"] = measure(ghost_fill, report=False)
        res["ratio_band_off_over_on"] = res["band_off"]["us"] / res["band_on"]["us"]
    print(json.dumps(res))
    if a.out:
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.key or ("parent" if a.parent else "this_build")] = res
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1)
            f.write("\n")
    ctx.comm_finalize()
    ctx.close()


if __name__ == "__main__":
    main()
