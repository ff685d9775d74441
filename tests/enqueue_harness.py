"""Enqueue-only runs of the `_dev` entry points (include/seabreeze_hip.h: they "enqueue on `stream` ... without
synchronising"): a whole sequence of calls goes behind device work that keeps the caller's stream busy, with no host
synchronisation between the first enqueue and the end.  TEST INFRASTRUCTURE ONLY.

One step, everything on the same side stream s:
  1  a filler (a chain of torch.mm on fixed tensors) that keeps s busy far longer than the host needs to enqueue the step;
  2  the step's theta, u, v are copied IN PLACE into the buffers the library is given;
  3  the library call with stream = s;
  4  every output / state array is copied into the step's snapshot; the state is carried in place.
After the last step s is synchronised once, then the snapshots are read.

Why that sees a mis-ordered operation: whatever the library does that is not ordered behind 2 on s reads the theta of the
step before -- valid data, another thc --, and whatever has not finished by 4 leaves a wrong snapshot.  Nothing is ever
poisoned with NaN or garbage: stale step inputs are the detector (before the first step the buffers hold the inputs of a
step beyond the sequence).

The filler's length is measured, not assumed: its duration once with events, the host's wall time per step with
perf_counter; a run whose filler is not at least RATIO times the enqueue time raises VacuousRun -- it does not pass.  For
steady-state calls (`steady[k]`) an event recorded right behind the filler must still be pending immediately before the
library call (else VacuousRun) and immediately after it returned (else the call blocked: BlockedCall).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np
import torch

from seabreeze_param_amd import hip

RATIO = 20.0            # filler duration / host enqueue time of one step, at least
FILLER_MS = 25.0        # what the filler is sized for
FILLER_N = 4096


class VacuousRun(RuntimeError):
    """the stream was not busy while the calls were enqueued: the run shows nothing"""


class BlockedCall(AssertionError):
    """a steady-state call returned only after work enqueued ahead of it had finished"""


class Filler:
    """reps x torch.mm on fixed finite tensors (rows of b sum to 1: the values stay bounded), sized to FILLER_MS"""

    def __init__(self, n=FILLER_N, target_ms=FILLER_MS):
        self.a = torch.rand((n, n), dtype=torch.float32, device="cuda")
        self.b = torch.full((n, n), 1.0 / n, dtype=torch.float32, device="cuda")
        self.out = [torch.empty_like(self.a), torch.empty_like(self.a)]
        self.reps = 1
        for _ in range(2):                               # (the first torch.mm loads its kernels)
            self.enqueue()
        torch.cuda.synchronize()
        one = self.measure()
        self.reps = int(min(256, max(1, np.ceil(target_ms / max(one, 1e-3)))))
        self.ms = self.measure()

    def enqueue(self):
        """on torch's current stream"""
        x = self.a
        for r in range(self.reps):
            torch.mm(x, self.b, out=self.out[r & 1])
            x = self.out[r & 1]

    def measure(self):
        """the filler's duration in ms on an idle device, once, with events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.enqueue()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


@dataclass
class Case:
    """One sequence's inputs, host side.  kind: "generic" (sb_seabreeze_diag_*_dev, SB_BND_GLOBAL), "f2py" (sb_diag_*_dev) or
    "band" (sb_band_seabreeze_diag_*_dev: mask, z, sigma and theta are (ny + 2 halo, nx + 2 halo) frames with zero ghost
    cells; the statics' are filled once by swap_bounds on the sequence's stream, theta's by every call).  theta, u, v:
    one array per step; p: (nz, ny, nx), or (nz,) for "f2py"."""
    kind: str
    dt: type
    nx: int
    ny: int
    nz: int
    p: np.ndarray
    mask: np.ndarray
    z: np.ndarray
    sigma: np.ndarray
    theta: list
    u: list
    v: list
    tns: list
    stale: tuple                        # (theta, u, v) of a step beyond the sequence: what the in-place buffers hold at first
    halo: int = 0
    timestep: float = 5400.0            # seconds; the f2py flavour is handed timestep / 60 minutes
    setup: object = None                # setup(ctx), once, ahead of the sequence's first enqueue: the switches of this case
    hint: object = None                 # sb_set_search_radius_hint ahead of EVERY call (several cases may share a context)
    extra: dict = field(default_factory=dict)

    @property
    def nsteps(self):
        return len(self.tns)


def frame(a, halo, dt):
    """interior -> (ny + 2 halo, nx + 2 halo) with zero ghost cells"""
    a = np.asarray(a, dtype=dt)
    f = np.zeros((a.shape[0] + 2 * halo, a.shape[1] + 2 * halo), dt)
    f[halo:halo + a.shape[0], halo:halo + a.shape[1]] = a
    return f


class Sequence:
    """The device side of one case on one context and one stream.  upload() before anything is enqueued; enqueue_step(k)
    per step, in order; collect() after the caller's final synchronisation."""

    def __init__(self, ctx, case, stream, filler=None, call_stream=None, sync_each=False, steady=None):
        self.ctx, self.case, self.stream, self.filler = ctx, case, stream, filler
        self.call_stream = call_stream if call_stream is not None else stream     # (the self-check hands the call another one)
        self.sync_each = sync_each
        n = case.nsteps
        self.steady = list(steady) if steady is not None else [k >= 1 for k in range(n)]
        self.t_enqueue = [0.0] * n
        self.pending_before = [None] * n
        self.pending_after = [None] * n
        self.uploaded = False

    def upload(self):
        c = self.case
        tdt = torch.float64 if np.dtype(c.dt) == np.float64 else torch.float32
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=c.dt)).cuda()
        self.p, self.mask, self.z, self.sigma = up(c.p), up(c.mask), up(c.z), up(c.sigma)
        self.theta_all, self.u_all, self.v_all = (torch.stack([up(a) for a in xs]) for xs in (c.theta, c.u, c.v))
        # the buffers the library is given: until step 2 of the first step rewrites them they hold valid inputs of a step
        # that is NOT in the sequence (the last step's would let a call that ran ahead of everything get step n right)
        self.theta, self.u, self.v = (up(a) for a in c.stale)
        nstate = 3 if c.kind == "f2py" else 4
        self.state = [torch.zeros((c.ny, c.nx), dtype=tdt, device="cuda") for _ in range(nstate)]
        if c.kind == "f2py":
            self.state.append(torch.zeros((4, c.ny, c.nx), dtype=tdt, device="cuda"))      # `output`
        self.hist = [[torch.zeros_like(s) for s in self.state] for _ in range(c.nsteps)]
        self.ev = [torch.cuda.Event() for _ in range(c.nsteps)]
        self.statics_filled = c.kind != "band"
        if c.setup is not None:
            c.setup(self.ctx)
        self.uploaded = True

    def _call(self, k):
        c, h = self.case, self.call_stream.cuda_stream
        ptr = lambda t: t.data_ptr()
        if c.hint is not None:
            self.ctx.set_search_radius_hint(c.hint)      # (host state only)
        if c.kind == "generic":
            self.ctx.seabreeze_diag_dev(c.dt, c.timestep, c.tns[k], c.nx, c.ny, c.nz, 0, hip.SB_BND_GLOBAL, ptr(self.p), ptr(self.u),
                                        ptr(self.v), ptr(self.theta), ptr(self.mask), ptr(self.z), ptr(self.sigma),
                                        *[ptr(s) for s in self.state], stream=h)
        elif c.kind == "band":
            self.ctx.band_seabreeze_diag_dev(c.dt, c.timestep, c.tns[k], c.nx, c.ny, c.nz, c.halo, ptr(self.p), ptr(self.u),
                                             ptr(self.v), ptr(self.theta), ptr(self.mask), ptr(self.z), ptr(self.sigma),
                                             *[ptr(s) for s in self.state], stream=h)
        elif c.kind == "f2py":
            self.ctx.diag_dev(c.dt, c.tns[k], c.nz, c.nx, c.ny, ptr(self.p), ptr(self.z), ptr(self.sigma), ptr(self.theta),
                              ptr(self.v), ptr(self.u), ptr(self.mask), *[ptr(s) for s in self.state], stream=h,
                              timestep=c.timestep / 60.0)
        else:
            raise ValueError(c.kind)

    def enqueue_step(self, k):
        assert self.uploaded
        c, s = self.case, self.stream
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            if not self.statics_filled:                  # a band's static ghost cells: once, on s, nothing waited for
                for f in (self.z, self.sigma, self.mask):
                    self.ctx.swap_bounds_dev(c.dt, f.data_ptr(), c.nx, c.ny, c.halo, stream=self.call_stream.cuda_stream)
                self.statics_filled = True
            if self.filler is not None:
                self.filler.enqueue()                    # 1
                self.ev[k].record(s)
            self.theta.copy_(self.theta_all[k])          # 2
            self.u.copy_(self.u_all[k])
            self.v.copy_(self.v_all[k])
            if self.filler is not None:
                self.pending_before[k] = not self.ev[k].query()
            self._call(k)                                # 3
            if self.filler is not None:
                self.pending_after[k] = not self.ev[k].query()
            for dst, src in zip(self.hist[k], self.state):     # 4
                dst.copy_(src)
        self.t_enqueue[k] = time.perf_counter() - t0
        if self.sync_each:                               # the synchronised twin
            self.call_stream.synchronize()
            s.synchronize()
            self.ctx.synchronize()

    def collect(self):
        """-> per step the list of arrays [ws, wd, thc, sb_con] (f2py: [ws, wd, thc, output])"""
        return [[t.cpu().numpy() for t in step] for step in self.hist]

    # ---- what the run itself showed
    def enqueue_seconds(self):
        """host wall time of enqueueing one step: the median over the steps behind the first"""
        ts = self.t_enqueue[1:] or self.t_enqueue
        return float(np.median(ts))

    def report(self, what):
        """prints the filler's duration and the host's enqueue time per step"""
        f_ms, e_ms = self.filler.ms, 1e3 * self.enqueue_seconds()
        print(f"[enqueue-only] {what}: filler {f_ms:.2f} ms per step ({self.filler.reps} x mm), host enqueue {e_ms:.3f} ms per "
              f"step, ratio {f_ms / max(e_ms, 1e-9):.0f}; the whole sequence enqueued in {1e3 * sum(self.t_enqueue):.2f} ms")

    def check_busy(self, what, assert_no_sync=True):
        """VacuousRun unless the filler outlasts the enqueueing RATIO times and the stream was busy ahead of every call;
        BlockedCall if a steady-state call returned with the filler ahead of it finished"""
        n = self.case.nsteps
        idle = [k for k in range(n) if not self.pending_before[k] and (self.steady[k] or not assert_no_sync)]
        if idle:
            raise VacuousRun(f"{what}: the filler had finished before the call of step(s) {[k + 1 for k in idle]} was made")
        if assert_no_sync:
            blocked = [k for k in range(n) if self.steady[k] and not self.pending_after[k]]
            if blocked:
                raise BlockedCall(f"{what}: the call of step(s) {[k + 1 for k in blocked]} returned only after the filler enqueued "
                                  f"ahead of it had finished -- a hidden synchronisation (enqueue times, ms: "
                                  f"{[round(1e3 * t, 3) for t in self.t_enqueue]})")
        check_ratio(self.filler, self.enqueue_seconds(), what)


def check_ratio(filler, enqueue_s, what):
    if filler.ms < RATIO * 1e3 * enqueue_s:
        raise VacuousRun(f"{what}: filler {filler.ms:.2f} ms < {RATIO:.0f} x enqueue time {1e3 * enqueue_s:.3f} ms")


def run_interleaved(seqs, order):
    """enqueue step k of seqs[i] for every (i, k) of `order`, no synchronisation in between; then every stream once"""
    for q in seqs:
        if not q.uploaded:
            q.upload()
    torch.cuda.synchronize()
    for i, k in order:
        seqs[i].enqueue_step(k)
    for q in seqs:
        q.call_stream.synchronize()
        q.stream.synchronize()
    return [q.collect() for q in seqs]


def run_enqueued(ctx, case, steps, stream, filler, call_stream=None, steady=None, what="", assert_no_sync=True, check=True):
    """The whole sequence of `case` (its first `steps` steps) enqueued on `stream` behind `filler`, one synchronisation at
    the end.  -> (per-step arrays, the Sequence)"""
    assert steps == case.nsteps
    q = Sequence(ctx, case, stream, filler=filler, call_stream=call_stream, steady=steady)
    out = run_interleaved([q], [(0, k) for k in range(steps)])[0]
    q.report(what or case.kind)
    if check:
        q.check_busy(what or case.kind, assert_no_sync=assert_no_sync)
    return out, q


def run_synchronised(ctx, case, stream):
    """the same sequence, no filler, everything synchronised after every call: the twin an enqueue-only run must equal"""
    q = Sequence(ctx, case, stream, sync_each=True)
    return run_interleaved([q], [(0, k) for k in range(case.nsteps)])[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    v = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(v) == b.view(v)).all())
