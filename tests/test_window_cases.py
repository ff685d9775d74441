"""The directed window-search fields (tests/window_cases.py) against the numpy model of the radius, the oracle and numpy
window means -- on the CPU.  Three independent statements of the window rule are held to each other here, so that
tests/test_contrast_window_gpu.py can hold the kernels to them:

* the closed form (radius = max(1, Chebyshev distance to the lone cell)) equals radius_ref.search_radius wherever it applies;
* the oracle's largest radius is the closed form's W, its thc is the numpy window mean at the closed form's radius;
* coverage: the global-rule cases of a kernel visit every (owned column of a strip, radius) and every (row of a block,
  radius) pair, radii 1 .. L -- and with them every radius of k_strip32 at which a window straddles column 64 of its
  staged row;
* sensitivity: in at least 90 % of a Family A case's band cells with radius r < L the contrast at r + 1 differs from the
  contrast at r by more than 1e-3 K -- a radius off by one cannot hide inside any tolerance the GPU module uses.

Recorded (interior placement): L = 31 -> 4489 band cells, largest radius 33, 520 beyond L; L = 32 -> 4761 / 34 / 536.  The
lattices reach beyond (p - 1) / 2 near the north pole row, where the last lattice row lies up to p - 1 rows away (p = 25:
19, p = 33: 28): with L = 16 those cells are ones the strip kernel hands to the global-memory search."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import radius_ref
import window_cases as wc

NWORK = max(1, min(16, len(os.sched_getaffinity(0))))


@pytest.mark.parametrize("L", wc.LIMITS)
def test_closed_form_is_the_models_radius(L):
    specs = wc.all_specs(L)
    assert len({s.name for s in specs}) == len(specs)
    for s in specs:
        c = wc.build(s)
        model = wc.model_radius(c.mask, c.halo, c.rule)
        assert np.array_equal(model, c.radius), s.name
        if c.rule == "wrapper":                                # ... and as the f2py flavour sees the field
            assert np.array_equal(wc.model_radius(c.mask, 0, c.rule, f2py=True), c.view("f2py")[1]), s.name
        assert np.array_equal(model != 0, c.band), s.name
        assert not (model == -1).any(), s.name                 # no cell without a window
        if c.family == "A":
            assert c.max_radius == c.W, s.name
            # every radius up to W occurs
            # (a lone cell in the rim of a frame lies a few cells from the nearest band cell)
            first = 1 if c.rule != "halo" else int(c.radius[c.band].min())
            assert first <= 5 and set(np.unique(c.radius[c.band])) == set(range(first, c.W + 1)), s.name
        # under the global rule and in frames the expectation IS the closed form; under the wrapper rule it is unless the
        # lone cell sits in column 0 (read twice)
        assert c.closed == (c.family == "A" and not (c.rule == "wrapper" and c.lone[1] == 0)), s.name
    c = wc.build(wc.all_specs(L)[0])                           # interior, a land cell in the sea
    W = L + 2
    assert c.lone == wc.INTERIOR and int(c.band.sum()) == (2 * W + 1) ** 2 and c.beyond() == (2 * W + 1) ** 2 - (2 * L + 1) ** 2
    for r in range(1, W + 1):
        assert int((c.radius == r).sum()) == 8 * r + (r == 1), r
    if L == 31:
        assert (int(c.band.sum()), c.max_radius, c.beyond()) == (4489, 33, 520)
    if L == 32:
        assert (int(c.band.sum()), c.max_radius, c.beyond()) == (4761, 34, 536)


def test_a_lone_cell_in_the_column_the_wrapper_rule_never_reads():
    """Why the wrapper placements replace (16, 159): every band cell of that patch is without a window."""
    for L in wc.LIMITS:
        c = wc.lone_cell(L, (16, 159), "global", True)
        model = radius_ref.search_radius(c.mask, wc.MAXDIST, 0, radius_ref.BND_WRAPPER)
        assert np.array_equal(model != 0, c.band) and (model[c.band] == -1).all(), L


@pytest.mark.parametrize("L", wc.LIMITS)
def test_coverage_of_columns_rows_and_radii(L):
    cases = [wc.build(s) for s in wc.global_specs(L)]
    cols, rows = wc.coverage(cases, L)
    assert cols[:, 1:].all(), np.argwhere(~cols[:, 1:])
    assert rows[:, 1:].all(), np.argwhere(~rows[:, 1:])
    if L == 31:
        # k_strip32's six-entry branch: the window of owned column c with radius r crosses into the third segment of the
        # staged row where c + 32 + r >= 64
        c, r = np.meshgrid(np.arange(32), np.arange(L + 1), indexing="ij")
        six = (c + 32 + r >= 64) & (r >= 1)
        assert six.sum() > 0 and cols[six].all()


def _oracle_check(spec):
    from oracle.pyoracle import Oracle
    orc = Oracle(8)                   # (one per thread: it keeps the largest radius of its last call in an attribute)
    c = wc.build(spec)
    flavours = ("generic", "f2py") if c.rule == "wrapper" else ("generic",)
    bad = []
    for fl in flavours:
        st, p, u, v, th = wc.inputs(c, 1, np.float64, fl)
        state = [np.full((wc.NY, wc.NX), wc.MARKER) for _ in range(3 if fl == "f2py" else 4)]
        if fl == "f2py":
            orc.diag(1, p, st.z, st.sigma, th, v, u, c.mask, *state, timestep=wc.TIMESTEP_MIN)
        else:
            orc.seabreeze_diag(wc.TIMESTEP_S, 1, p, u, v, th, c.mask, st.z, st.sigma, *state, halo=c.halo, bnd=c.bnd)
        nn = orc.last_nn_max
        thc = state[2]
        band, radius = c.view(fl)
        num = wc.window_contrast(c, wc.t0_of(c, th, st), radius)
        if nn != int(radius.max()):
            bad.append((spec.name, fl, "nn_max", nn, int(radius.max())))
        if np.isnan(thc).any() or np.isnan(num[band]).any():
            bad.append((spec.name, fl, "NaN"))
        err = float(np.max(np.abs(thc[band] - num[band])))
        if not err < 1e-9:
            bad.append((spec.name, fl, "thc against the numpy window mean", err))
        if not np.all(thc[~band] == wc.MARKER):
            bad.append((spec.name, fl, "state touched off the band"))
    return bad


@pytest.mark.parametrize("L", wc.LIMITS)
def test_oracle_against_closed_form_and_numpy_means(L, oracles):
    """The oracle itself, pinned to statements that do not come from it: its largest radius is W (the model's maximum for
    the lattices), its thc is the fp64 window mean at the expected radius (1e-9 K: the summation orders differ), no NaN."""
    with ThreadPoolExecutor(NWORK) as pool:
        bad = [b for res in pool.map(_oracle_check, wc.all_specs(L)) for b in res]
    assert not bad, bad


@pytest.mark.parametrize("L", wc.LIMITS)
def test_a_radius_off_by_one_moves_thc(L):
    """The sensitivity condition, for every Family A case and each of the three calls' temperatures."""
    for s in wc.all_specs(L):
        c = wc.build(s)
        if c.family != "A":
            continue
        sel = c.band & (c.radius >= 1) & (c.radius < L)
        if c.rule == "halo":
            sel &= c.radius + 1 <= wc.frame_reach(c.halo)      # the next window must exist
        assert sel.sum() > 50, s.name
        st = wc.statics(c)
        for tn in wc.STEPS:
            t0 = wc.t0_of(c, wc.theta(c, tn), st)
            at_r = wc.window_contrast(c, t0, c.radius)
            at_r1 = wc.window_contrast(c, t0, np.where(sel, c.radius + 1, 0).astype(np.int32))
            assert np.isfinite(at_r[sel]).all() and np.isfinite(at_r1[sel]).all(), (s.name, tn)
            share = float((np.abs(at_r1[sel] - at_r[sel]) > 1e-3).mean())
            assert share >= 0.90, (s.name, tn, share)
