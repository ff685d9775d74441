"""The three LDS contrast kernels' window search at every seam (fields: tests/window_cases.py; the fields themselves are
held to the numpy model, the oracle and numpy window means in tests/test_window_cases.py).

Kernels, by the knobs that select them, and L, the largest radius each answers from its LDS tables:

    k_strip             fp64, fp32   radius hint 16                           L = 16
    k_strip32           fp32         radius hint 30                           L = 31
    k_thc3, halo 24     fp64         radius hint 24                           L = 24
    k_thc3, halo 32     fp64         radius hint 30                           L = 32
    k_thc3, halo 32     fp32         radius hint 30, set_wide_strip(False)    L = 32

Every case runs three calls on one distance field (tn = 1, 2, 3, fresh temperatures, state carried): the first plans, the
later ones march by the stored plan and must reproduce radius and land-side count from the stored word.  Per call:

* ws, wd, thc, sb_con (f2py flavour: the four output planes and the state) against the fp64 oracle -- fp64 at the suite's
  1e-7 relative with its 1e-9 floor, fp32 by the shared single-precision rule (oracle/fp32_criterion.py) on the same
  fp32-representable inputs; the trigger pattern equals the oracle's; cells off the band keep their markers;
* sb_last_counters: band cells and largest radius are the model's, no cell with one class, and the cells handed to the
  global-memory search are EXACTLY the band cells whose radius exceeds L -- the hand-off sits one cell beyond the tables
  (16 -> 17, 24 -> 25, 31 -> 32, 32 -> 33) -- the same number on all three calls.  No kernel documents a more conservative
  rule, and none showed one.

The oracle sequences of a kernel's cases are computed once, by a pool of threads, and shared by every test of the kernel."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import window_cases as wc
from conftest import relerr
from oracle import fp32_criterion as crit

pytestmark = pytest.mark.gpu

KERNELS = {                     # name: (L, dtype, radius hint, set_wide_strip, a strip kernel)
    "strip-f64": (16, np.float64, 16, True, True),
    "strip-f32": (16, np.float32, 16, True, True),
    "strip32-f32": (31, np.float32, 30, True, True),
    "tiles24-f64": (24, np.float64, 24, True, False),
    "tiles32-f64": (32, np.float64, 30, True, False),
    "tiles32-f32": (32, np.float32, 30, False, False),
}
NWORK = max(1, min(16, len(os.sched_getaffinity(0))))


def _flavours(spec):
    return ("generic", "f2py") if spec[3] == "wrapper" else ("generic",)


def _runs(L):
    return [(s, fl) for s in wc.all_specs(L) for fl in _flavours(s)]


@functools.lru_cache(maxsize=1)
def _oracle_sequences(L, dtype):
    """{(spec, flavour): calls} for every case of limit L on inputs of `dtype`, in the oracle's double precision."""
    from oracle.pyoracle import Oracle
    keys = _runs(L)
    # (a fresh oracle object per sequence: it keeps the largest radius of its last call in an attribute)
    with ThreadPoolExecutor(NWORK) as pool:
        seqs = list(pool.map(lambda k: wc.run_sequence(Oracle(8), wc.build(k[0]), k[1], dtype, sdtype=np.float64), keys))
    return dict(zip(keys, seqs))


@pytest.fixture
def kernel(request, hipctx, oracles):
    L, dtype, hint, wide, _ = KERNELS[request.param]
    hipctx.set_search_radius_hint(hint)
    hipctx.set_wide_strip(wide)
    yield hipctx, L, dtype
    hipctx.set_search_radius_hint(16)
    hipctx.set_wide_strip(True)
    hipctx.set_plan_cache(True)
    hipctx.set_fold(True)


def _assert_close64(a, b, what):
    e = relerr(a, b, floor=1e-2)      # (test_parity_gpu.py: |err| <= 1e-7 |b|, or 1e-9 absolute)
    assert e < 1e-7, f"{what}: rel err {e}"


def _check(ctx, L, dtype, spec, flavour):
    """One case under one flavour: the three calls against the oracle's, and the counters against the model's."""
    case = wc.build(spec)
    band, radius = case.view(flavour)
    want = dict(band_cells=int(band.sum()), global_path_cells=int((radius > L).sum()), one_class_cells=0,
                max_radius=int(radius.max()))
    ora = _oracle_sequences(L, dtype)[(spec, flavour)]
    hip = wc.run_sequence(ctx, case, flavour, dtype)
    names = ("ws", "wd", "thc", "sb_con")
    per, prev_g, prev_o = [], None, None
    for tn, g, o in zip(wc.STEPS, hip, ora):
        what = f"{spec.name} {flavour} tn={tn}"
        # print before asserting: a run with -s shows every figure
        print(what, g["counters"], "model", want, "oracle nn_max", o["nn_max"])
        assert o["nn_max"] == want["max_radius"], what
        assert g["counters"] == want, (what, g["counters"], want)
        if case.W == L:
            # nothing beyond the tables: the largest radius they answer, at every border offset, and nothing handed on
            assert g["counters"]["global_path_cells"] == 0 and g["counters"]["max_radius"] == L, what
        if flavour == "f2py":
            gs, os_ = g["state"] + [g["out"][0]], o["state"] + [o["out"][0]]
            gs, os_, b = [a[:-1] for a in gs], [a[:-1] for a in os_], band[:-1]
            assert np.all(g["out"][0, :-1][~b] > 1e19), what                      # the fill value off the band
            assert not g["out"][:, -1].any() and all(np.all(a[-1] == wc.MARKER) for a in g["state"]), what    # row ny - 1 untouched
        else:
            gs, os_, b = g["state"], o["state"], band
            assert np.all(gs[3][~b] == 0.0), what
        assert all(np.all(a[~b] == wc.MARKER) for a in gs[:3]), what             # the state off the band keeps its markers
        assert not np.isnan(gs[2]).any(), what
        if dtype == np.float64:
            for a, r, nm in zip(gs, os_, names):
                _assert_close64(a, r, f"{what} {nm}")
            if flavour == "f2py":
                for k, nm in enumerate(("sb_con", "t0", "windspeed", "winddir")):
                    _assert_close64(g["out"][k, :-1], o["out"][k, :-1], f"{what} output {nm}")
            assert np.array_equal(gs[3] != 0, os_[3] != 0), what
        else:
            first = [np.full_like(a, wc.MARKER) for a in gs]
            first_o = [np.full_like(a, wc.MARKER) for a in os_]
            ts = wc.TIMESTEP_MIN * 60.0 if flavour == "f2py" else wc.TIMESTEP_S
            res = crit.check_step(tn, prev_g or first, gs, prev_o or first_o, os_, b, timestep=ts)
            print(what, {k: res[k] for k in ("thc_abs_K", "windspeed_rel", "winddir_abs_deg", "sb_con_bound_ratio", "trigger_flips", "unexplained_flips")})
            per.append(res)
            if flavour == "f2py":
                assert relerr(g["out"][1, :-1], o["out"][1, :-1], floor=1.0) < 2e-6, what      # t0 (test_strip32_gpu.py)
        prev_g, prev_o = gs, os_
    if per:
        res = crit.merge(per)
        assert res["ok"], (spec.name, flavour, res)


_SUBSET = lambda s: s[0] == "A" and s[3] == "global" and s[2] in wc.SEAM_PLACEMENTS
MODES = ("stored-plan", "replan", "kprep")


def pytest_generate_tests(metafunc):
    """The cases depend on the kernel's L: (kernel, mode, case) triples, the kernel outermost so that its oracle sequences
    are computed once and dropped when the next kernel's are."""
    if "spec" not in metafunc.fixturenames:
        return
    triples, ids = [], []
    for kn, (L, _, _, _, strip) in KERNELS.items():
        for mode in MODES:
            if mode == "kprep" and not strip:
                continue                                      # (the tile kernel never does k_prep's work)
            for s, fl in _runs(L):
                if mode == "stored-plan" or _SUBSET(s):
                    triples.append((kn, mode, s, fl))
                    ids.append(f"{kn}-{mode}-{s.name}-{fl}")
    metafunc.parametrize("kernel,mode,spec,flavour", triples, ids=ids, indirect=["kernel"])


def test_window_search(kernel, mode, spec, flavour):
    """Every case with the defaults (the first call plans, two calls march by the stored plan); the interior and the
    two double-seam placements (W = L + 2 and W = L) again with set_plan_cache(False) -- every call plans -- and, for the
    strip kernels, with set_fold(False): k_prep as a kernel of its own ahead of them."""
    ctx, L, dtype = kernel
    ctx.set_plan_cache(mode != "replan")
    ctx.set_fold(mode != "kprep")
    _check(ctx, L, dtype, spec, flavour)
