"""The coast-distance kernels on the directed fields of tests/dist_cases.py (what the fields are and what they reach:
tests/test_dist_cases.py, on the CPU): every case in fp64 and fp32 against the oracle of that precision under the rule of
tests/test_setup_gpu.py (_check_dist: the same unreached cells, the same signs, 1e-12 | 2e-6 of max(|d|, 1 km)), in fp64
also against the numpy model (tests/dist_ref.py); every source cell's own distance exactly 0.5 km; the Family A and B fields
of k = 15, 31 and 40 -- every kernel under the band policy -- cut into three bands of unequal height with a source exactly k
and k + 1 rows beyond each cut on both sides of it, bit for bit against the whole-grid call; and the value cases (coast and mask with negative numbers, both zeros and fractions).

A failure names the case and the first differing cell with the sources in its window (row offset, window bit).

What the noise and island masks of the older modules cannot show and this module does: coast != 0 or mask != 0 in place
of > 0 (the value cases: no earlier input is negative), and a source counted as swept after its own cell (the k = 0 field
with 2 maxdist below 0.5 km: the only distance there is the source's own)."""
import numpy as np
import pytest

import dist_cases as dc
from band_frames import band_dist, cuts_of
from test_setup_gpu import _check_dist

pytestmark = pytest.mark.gpu

TOL = {8: 1e-12, 4: 2e-6}
BIG = dc.BIG
SHAPE_IDS = [dc.shape_id(s) for s in dc.SHAPES]
BAND_SHAPES = [s for s in dc.SHAPES if (s.k in (15, 31) and s.nx in (600, 286, 318, 63, 62)) or (s.k, s.nx) == (40, 600)]


def _run(ctx, orc, c, dt):
    a = [np.ascontiguousarray(v, dt) for v in (c.coast, c.mask, c.lon, c.lat)]
    o = orc.get_dist(*a, maxdist=c.maxdist, kwin=c.k)
    h = ctx.get_dist(*a, maxdist=c.maxdist, kwin=c.k)
    return h, o


def _hold(ctx, orc, c, prec):
    dt = np.float64 if prec == 8 else np.float32
    h, o = _run(ctx, orc, c, dt)
    what = f"{c.name} fp{8 * prec}"
    msg = dc.first_difference(c, h.astype(np.float64), o.astype(np.float64), TOL[prec])
    assert msg is None, f"fp{8 * prec} against the oracle: {msg}"
    _check_dist(h, o, what, TOL[prec])
    if prec == 8:
        msg = dc.first_difference(c, h, dc.expected(c), TOL[8])
        assert msg is None, f"fp64 against the model: {msg}"
        _check_dist(h, dc.expected(c), what + " (model)", TOL[8])
    # the 0.5 km anchor: a source's own distance is R 2 atan2(0, 1) + 0.5 (thrown away only where 0.5 > 2 maxdist)
    own = np.abs(h[c.coast > 0])
    assert np.all(own == (0.5 if 0.5 <= 2 * c.maxdist else BIG)), f"{what}: a source cell's own distance is not 0.5"
    return h


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("shape", dc.SHAPES, ids=SHAPE_IDS)
def test_directed_cases(hipctx, oracles, shape, prec):
    for c in dc.cases_of(shape):
        _hold(hipctx, oracles[prec], c, prec)


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("shape", dc.VALUE_SHAPES, ids=[dc.shape_id(s) for s in dc.VALUE_SHAPES])
def test_value_case(hipctx, oracles, shape, prec):
    """The reference's tests are coast > 0 and mask > 0: -1, -0.0 and 0 are no coast, -0.5, -0.0 and 0 give the negative sign."""
    c = dc.value_case(shape)
    h = _hold(hipctx, oracles[prec], c, prec)
    reached = np.abs(h) < BIG
    assert reached.any() and np.all((h[reached] > 0) == (c.mask[reached] > 0))
    plain = c._replace(coast=(c.coast > 0).astype(np.float64), mask=(c.mask > 0).astype(np.float64))
    dt = np.float64 if prec == 8 else np.float32
    assert np.array_equal(_run(hipctx, oracles[prec], plain, dt)[0], h)


def _band_field(c, bands):
    """The case's coast with a source exactly k rows and k + 1 rows beyond each cut, on both sides of it: the first lies in
    the last row a band's window reaches (and in its frame's outermost ghost row), the second in no window of the band."""
    coast = c.coast.copy()
    marks = []
    for n, cut in enumerate(b[0] for b in bands[1:]):
        col = (17 + 291 * n) % c.nx
        for row in (cut - 1 + c.k, cut + c.k, cut - c.k, cut - c.k - 1):
            if 0 <= row < c.ny:
                coast[row, col] = 1.0
                marks.append((row, col))
    return coast, marks


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("shape", BAND_SHAPES, ids=[dc.shape_id(s) for s in BAND_SHAPES])
def test_bands_equal_whole_grid(hipctx, oracles, shape, prec):
    dt = np.float64 if prec == 8 else np.float32
    k, ny = shape.k, dc.ny_of(shape.k)
    # cuts at rows k + 1 and 2k + 1: the rows k and k + 1 beyond either cut lie in the grid on both sides of it
    heights = (k + 1, k, ny - 2 * k - 1)
    bands = cuts_of(heights)
    assert sum(heights) == ny and len(set(heights)) == 3 and any(h % 2 for h in heights)
    assert all(cut - k - 1 >= 0 and cut + k <= ny - 1 for cut in (b[0] for b in bands[1:]))
    ran = 0
    for c in dc.cases_of(shape):
        if c.family not in "AB" or c.maxdist >= dc.FAR:
            continue
        coast, marks = _band_field(c, bands)
        assert len(set(marks)) == 8                              # (either cut has its four sources)
        c = c._replace(coast=coast, name=c.name + "-bands")
        whole, o = _run(hipctx, oracles[prec], c, dt)
        msg = dc.first_difference(c, whole.astype(np.float64), o.astype(np.float64), TOL[prec])
        assert msg is None, f"fp{8 * prec} against the oracle: {msg}"
        _check_dist(whole, o, c.name, TOL[prec])
        a = [np.ascontiguousarray(v, dt) for v in (c.coast, c.mask, c.lon, c.lat)]
        got = band_dist(hipctx, *a, bands, k, k, maxdist=c.maxdist)       # (asserts that nothing outside the interior is written)
        diff = got.view(np.uint8).reshape(ny, -1) != whole.view(np.uint8).reshape(ny, -1)
        assert not diff.any(), f"{c.name}: rows {np.flatnonzero(diff.any(1))[:8]} differ from the whole-grid call in their bits"
        # the sources k rows beyond a cut are seen across it: the last row of the band below lies in the late class of the
        # source k rows above it, which is never thrown away
        for n, cut in enumerate(b[0] for b in bands[1:]):
            assert (cut - 1 + k, (17 + 291 * n) % c.nx) in marks and abs(got[cut - 1, (17 + 291 * n) % c.nx]) < BIG, c.name
        ran += 1
    assert ran >= 8
    assert {s.kernel for s in BAND_SHAPES} == set(dc.KERNELS)
