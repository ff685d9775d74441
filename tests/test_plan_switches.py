"""Which of a context's six opt-in switches serve a diag call (sb_apply_switches, sb_diag_plan.hpp), and the frame a band step
gives theta (sb_band_folds_frame), on the CPU: the `switches` command of tests/plan_dump.cpp, built host-only
(tests/plan_dump.py).

Every condition below is written out by hand from what INTEGRATION.md ("Regional grids of a few km" to "Inputs with
missing values") and the table of launch sequences in DESIGN.md section 2.3 say about the calls each switch serves:

  sb_set_table_contrast         whole single-domain calls of the host-model flavour, SB_BND_GLOBAL / SB_BND_HALO, Geo::band == 0
  sb_set_table_contrast_f2py    beside it: whole calls of the f2py flavour, SB_BND_WRAPPER (which has no ghost cells), no gathered moments
  sb_set_table_contrast_bands   beside it: band phases and calls with gathered moments of the host-model flavour, SB_BND_HALO
  sb_set_table_window_cache     beside it: a whole table call; ignored for band steps and calls with gathered moments
  sb_set_nonfinite_guard        every whole call, with or without the table switches, on plain geometry (Geo::band == 0)
  sb_set_nonfinite_guard_bands  beside it: phase 2 of a band step and calls with gathered moments, host-model flavour

A band step (host-model flavour, SB_BND_HALO, gathered moments, phase 1 then phase 2) decides its frame first and runs both
phases with Geo::band != 0 exactly if it `folds`: the band tables and the band guard must then find Geo::band == 0.
"""
import itertools

import pytest

import plan_dump as pd
from plan_dump import BND_GLOBAL, BND_HALO, BND_WRAPPER

CLASSES = ((6, 8), (24, 4), (24, 8), (31, 8))       # (hint, esize): k_strip, k_strip32, the tile kernel twice
STRIP = {(6, 8): 1, (24, 4): 2, (24, 8): 0, (31, 8): 0}
STATES = [dict(zip(pd.SWITCHES, bits)) for bits in itertools.product((0, 1), repeat=6)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pd.build(tmp_path_factory)


def _ask(exe, cases):
    out = pd.run(exe, [pd.switches_line(str(i), **k) for i, k in enumerate(cases)])
    assert len(out) == len(cases)
    got = [pd.parse_switches(ln) for ln in out]
    assert [lab for lab, _ in got] == [str(i) for i in range(len(cases))]
    return [g for _, g in got]


def test_eligibility_over_every_switch_state_and_call(exe):
    cases = []
    for sw in STATES:
        for host, bnd, ghost, band, phases, gathered, (hint, esize) in itertools.product(
                (0, 1), (BND_WRAPPER, BND_GLOBAL, BND_HALO), (0, 1), (0, 1), (1, 2, 3), (0, 1), CLASSES):
            cases.append(dict(sw, host_model=host, t0_fly=host, bnd=bnd, ghost=ghost, band_geo=band, phases=phases,
                              gathered=gathered, hint=hint, esize=esize))
    assert len(cases) == 64 * 2 * 3 * 2 * 2 * 3 * 2 * 4
    for k, g in zip(cases, _ask(exe, cases)):
        on = lambda name: bool(k["sw_" + name])
        host, bnd, plain = bool(k["host_model"]), k["bnd"], not k["band_geo"]
        whole = k["phases"] == 3 and not k["gathered"]
        f2py = on("table") and on("table_f2py") and not host and bnd == BND_WRAPPER and not k["ghost"]
        host_table = on("table") and host and bnd in (BND_GLOBAL, BND_HALO) and plain
        band_table = host_table and on("table_bands") and bnd == BND_HALO and not whole
        want = dict(table=host_table or f2py, band_table=band_table, f2py_table=f2py, guard=on("guard") and plain,
                    guard_bands=on("guard") and on("guard_bands") and plain,
                    cache=on("table_cache") and whole and (host_table or f2py))
        # ... and what the two plans make of the filled input: the rows of the design table
        want["plan_table"] = (host_table and whole) or band_table or (f2py and whole)
        want["guard_on"] = on("guard") and plain and k["phases"] != 1 and (whole or (on("guard_bands") and host))
        for name, w in want.items():
            assert g[name] == int(w), (name, k, g)


def _band_step(sw, hint, esize, nx, **kw):
    return dict(sw, host_model=1, t0_fly=1, bnd=BND_HALO, ghost=1, gathered=1, mout=1, hint=hint, esize=esize, nx=nx, **kw)


def test_band_step_frame_and_the_switches_it_carries(exe):
    """A band step never folds its frame where the band tables or the band guard may be served, and then phase 2 is served
    (Geo::band == 0); where it folds, neither is."""
    first = [_band_step(sw, hint, esize, nx, phases=1) for sw in STATES for hint, esize in CLASSES for nx in (200, 99, 98)]
    folds = [g["folds"] for g in _ask(exe, first)]
    # both phases run with the Geo::band the frame decision gives them
    ph1 = _ask(exe, [dict(k, band_geo=f) for k, f in zip(first, folds)])
    ph2 = _ask(exe, [dict(k, band_geo=f, phases=2, mout=0) for k, f in zip(first, folds)])
    assert any(folds) and not all(folds)
    for k, f, g1, g2 in zip(first, folds, ph1, ph2):
        assert g1["folds"] == g2["folds"] == f, k                  # (the decision reads neither the phase nor Geo::band)
        tables = k["sw_table"] and k["sw_table_bands"]
        guard = k["sw_guard"] and k["sw_guard_bands"]
        if tables or guard:
            assert f == 0, k
        if tables:
            assert g1["band_table"] == g2["band_table"] == 1 and g1["plan_table"] == g2["plan_table"] == 1, (k, g1, g2)
        if guard:
            assert g2["guard"] == g2["guard_bands"] == 1 and g2["guard_on"] == 1 and g1["guard_on"] == 0, (k, g1, g2)
        if f:
            for g in (g1, g2):
                assert not any(g[n] for n in ("table", "band_table", "f2py_table", "guard", "guard_bands", "cache",
                                              "plan_table", "guard_on")), (k, g)


def test_every_switch_off(exe):
    """Nothing is filled, and a band step folds its frame exactly on a strip kernel with rows longer than 98 cells."""
    off = dict.fromkeys(pd.SWITCHES, 0)
    cases = [_band_step(off, hint, esize, nx, phases=ph, band_geo=band)
             for hint, esize in CLASSES for nx in (200, 99, 98) for ph in (1, 2) for band in (0, 1)]
    contrast = pd.plans(exe, [pd.line(f"{h}/{e}", hint=h, esize=e) for h, e in CLASSES])
    for (h, e), strip in STRIP.items():
        assert contrast[f"{h}/{e}"].contrast.startswith(f"strip={strip} "), (h, e)
    for k, g in zip(cases, _ask(exe, cases)):
        assert not any(g[n] for n in ("table", "band_table", "f2py_table", "guard", "guard_bands", "cache", "plan_table", "guard_on")), (k, g)
        assert g["folds"] == int(STRIP[(k["hint"], k["esize"])] != 0 and k["nx"] > 98), (k, g)
