"""The directed coast-distance fields (tests/dist_cases.py) against the numpy model (tests/dist_ref.py), the oracle and the
launch plan -- on the CPU, so that tests/test_dist_directed_gpu.py can hold the kernels to them:

* model against oracle: every case under the rule of tests/test_setup_gpu.py (_check_dist) at 1e-12;
* every case reaches the kernel and the cut bits it claims (tests/dist_plan_dump.cpp, as tests/test_dist_plan.py runs it);
* coverage, counted from the expected fields: over Family A of a shape every (target column mod 64, window bit 0 .. 2k) and
  every (target-row parity, row offset -k .. k) is reached, and no reached cell lies outside the window of a source;
* sensitivity: per kernel, each deliberate error of the model moves at least 20 cells in at least one case; the own-row
  class error must do so in Family C;
* no early-class minimum within 1e-4 relative of 2 maxdist: the fp32 run cannot flip a reset by rounding.

The index-nearest error (per sweep class, source row and side only the hit nearest by index) is exact wherever the
haversine term grows with the index distance inside a window.  That holds under set 1 and under sets 3 and 4 as well: a longitude that occurs twice is a tie, not a disorder, and permuted
latitudes leave every single row in order (the host's test of the order is strict, so it switches the cut off there, which
costs time and never a value).  It is wrong where a window crosses the seam of a frame that does not close: set 2, which is
why CIRCLE is off there and INNER is decided per target.  test_each_mutant_moves_cells asserts exactly that: no cell under
sets 1, 3 and 4, at least 20 under set 2 -- and the disorder along the rows, which set 4 is, is "rowstop"'s to show.

Recorded: 2256 cases, 8712 sources, 24 070 091 reached cells; model against oracle at most 4.5e-16 relative.  Per shape
(cases / sources / reached cells):
  BITS32 k15 nx600 52 / 508 / 304478, nx287 72 / 476 / 273527, k1 nx600 28 / 480 / 3183, k0 nx600 8 / 340 / 170;
  BITS64 k16 nx600 48 / 504 / 337451, k31 nx600 68 / 504 / 1100662, nx319 104 / 476 / 1016818;
  BITS_SMALL k31 nx318 108 / 484 / 1037245, nx63 240 / 424 / 854282, k15 nx286 76 / 480 / 276586;
  BYTES k31 nx62 236 / 416 / 829154, k20 nx30 152 / 292 / 173450;
  WIDE k32 68 / 532 / 1221191, k40 88 / 536 / 1871023, k62 112 / 532 / 4326937, k63 128 / 528 / 4412790 (nx600),
  k40 nx100 332 / 600 / 2089531, k63 nx100 336 / 600 / 3941613.
Cells moved per mutant, over a kernel's Family B and C cases and its first Family A field (side_class: Family C alone), as
"most in one case / cases that move of cases":
              k-1            k+1            noreset         reset_after_min  side_class   rowstop
  BYTES       278 / 118:120  124 / 75:120   3330 / 116:120  3952 / 116:120   60 / 16:16   1696 / 55:120
  BITS_SMALL  1123 / 116:116 1050 / 94:116  7743 / 110:116  9454 / 110:116   62 / 20:24   2469 / 56:116
  BITS32      1698 / 60:64   1630 / 64:64   4720 / 56:64    4614 / 54:64     30 / 18:24   973 / 16:64
  BITS64      1871 / 76:76   1778 / 76:76   12987 / 70:76   14405 / 70:76    62 / 18:24   2473 / 39:76
  WIDE        2524 / 260:268 2270 / 233:268 39341 / 256:268 37167 / 256:268  126 / 38:48  9608 / 140:268
index_nearest, most in one Family B case (k <= 40): set 2 BYTES 864, BITS_SMALL 896, BITS32 192, BITS64 896, WIDE 1517;
sets 1, 3 and 4: 0 in every case."""
import numpy as np
import pytest

import dist_cases as dc
import dist_ref
from test_dist_plan import dump          # noqa: F401  (the fixture that builds and runs tests/dist_plan_dump.cpp)
from test_setup_gpu import _check_dist

BIG = dist_ref.BIG
SHAPE_IDS = [dc.shape_id(s) for s in dc.SHAPES]


def test_shapes_stand_on_the_bounds_of_the_kernel_choice():
    have = {(s.nx, s.k): s.kernel for s in dc.SHAPES}
    assert set(have.values()) == set(dc.KERNELS)
    # nx = 2k + 256 | 2k + 257, nx = 2k | 2k + 1, k = 15 | 16, k = 31 | 32
    assert (have[(286, 15)], have[(287, 15)]) == ("BITS_SMALL", "BITS32")
    assert (have[(318, 31)], have[(319, 31)]) == ("BITS_SMALL", "BITS64")
    assert (have[(62, 31)], have[(63, 31)]) == ("BYTES", "BITS_SMALL")
    assert (have[(600, 15)], have[(600, 16)], have[(600, 31)], have[(600, 32)]) == ("BITS32", "BITS64", "BITS64", "WIDE")
    assert {s.k for s in dc.SHAPES if s.kernel == "WIDE"} == {32, 40, 62, 63}          # two, two, two and three passes of 31 rows
    # k_dist_wide on a grid narrower than its window (every column once, some window bits twice), and on one narrower than
    # a workgroup's reach only
    assert any(s.kernel == "WIDE" and 2 * s.k + 1 > s.nx for s in dc.SHAPES)
    assert any(s.kernel == "WIDE" and 2 * s.k + 1 <= s.nx < 256 + 2 * s.k for s in dc.SHAPES)
    for s in dc.SHAPES:
        ny = dc.ny_of(s.k)
        assert ny % 2 == 1 and ny >= 2 * s.k + 3 and s.nx * ny < 200_000


def test_cases_reach_the_kernel_and_cuts_they_claim(dump):
    lines, want = [], {}
    for s in dc.SHAPES:
        lines.append(f"K K/{dc.shape_id(s)} {s.nx} {s.k}")
        want[f"K/{dc.shape_id(s)}"] = [s.kernel]
        ny = dc.ny_of(s.k)
        for cset in (1, 2, 3, 4):
            lon, lat = dc.coords(cset, s.nx, ny)
            label = f"C/{dc.shape_id(s)}/{cset}"
            lines.append(" ".join(["C", label, str(s.k), str(s.nx), str(ny)] + [repr(float(v)) for v in lon] + [repr(float(v)) for v in lat]))
            want[label] = [str(dc.cuts_claim(cset, s.nx, s.k))] * 2                      # fp64 and fp32 coordinates
    got = dump(lines)
    for label, w in want.items():
        assert got[label][:len(w)] == w, (label, got[label], w)
    for c in dc.all_cases() + [dc.value_case(s) for s in dc.VALUE_SHAPES]:
        assert (c.kernel, c.cuts) == (c.shape.kernel, dc.cuts_claim(c.cset, c.nx, c.k)), c.name
    # the sets are what the issue of each family needs: all four cuts, no circle, rows only, no rows
    wide = dc.Shape("WIDE", 40, 600)
    assert [dc.cuts_claim(n, wide.nx, wide.k) for n in (1, 2, 3, 4)] == [15, dc.INNER | dc.ROWS, dc.ROWS, dc.CIRCLE | dc.INNER]
    lat4 = dc.coords(4, 600, 125)[1]
    assert np.any(np.diff(lat4) > 0) and np.any(np.diff(lat4) < 0) and np.all(np.diff(dc.coords(3, 600, 125)[1]) < 0)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=SHAPE_IDS)
def test_model_against_oracle(shape, oracles):
    cases = dc.cases_of(shape)
    assert len({c.name for c in cases}) == len(cases)
    nsrc = nreach = 0
    for c in cases:
        o = oracles[8].get_dist(c.coast, c.mask, c.lon, c.lat, maxdist=c.maxdist, kwin=c.k)
        m = dc.expected(c)
        _check_dist(m, o, c.name, 1e-12)
        nsrc += int((c.coast > 0).sum())
        nreach += int((np.abs(m) < BIG).sum())
    print(f"{dc.shape_id(shape)}: {len(cases)} cases, {nsrc} sources, {nreach} reached cells")
    for vs in dc.VALUE_SHAPES:
        if vs == shape:
            v = dc.value_case(vs)
            o = oracles[8].get_dist(v.coast, v.mask, v.lon, v.lat, maxdist=v.maxdist, kwin=v.k)
            _check_dist(dc.expected(v), o, v.name, 1e-12)
            plain = dist_ref.dist_model((v.coast > 0).astype(float), (v.mask > 0).astype(float), v.lon, v.lat, v.maxdist, v.k)
            assert np.array_equal(dc.expected(v), plain)
            assert {-1.0, 0.25, 2.0} <= set(np.unique(v.coast)) and np.signbit(v.coast[v.coast == 0]).all()
            assert set(np.unique(v.mask)) == {-0.5, 0.0, 0.3, 1.0} and np.signbit(v.mask[v.mask == 0]).any()
            # reached cells under each of the five mask values, sources of both values
            reached = np.abs(o) < BIG
            assert all((reached & (v.mask == x) & (np.signbit(v.mask) == sb)).any()
                       for x, sb in ((-0.5, True), (0.0, True), (0.0, False), (0.3, False), (1.0, False)))


def test_every_case_is_met_by_a_shape():
    """Families per shape: A and C under sets 1 and 2, B under all four; A with the reset inside the reach and out of it."""
    for s in dc.SHAPES:
        cs = dc.cases_of(s)
        fam = lambda f: {(c.cset, c.maxdist >= dc.FAR) for c in cs if c.family == f}
        assert fam("A") == {(1, False), (1, True), (2, False), (2, True)}, s
        if s.k >= 1:
            assert {n for n, _ in fam("B")} == {1, 2, 3, 4} and {n for n, _ in fam("C")} == {1, 2}, s
        for c in cs:
            if c.family == "A":                                  # lone cells: more than 2k + 1 apart in rows or in columns
                src = np.argwhere(c.coast > 0)
                dy = np.abs(src[:, None, 0] - src[None, :, 0])
                dx = np.abs(src[:, None, 1] - src[None, :, 1])
                dx = np.minimum(dx, c.nx - dx)
                near = (dy <= 2 * c.k + 1) & (dx <= 2 * c.k + 1)
                assert near.sum() == len(src), c.name
            if c.family == "C":
                cols = set(np.argwhere(c.coast > 0)[:, 1])
                assert cols in ({c.nx - 3, 0, 7}, {c.nx - 1}, {c.k + 2}), c.name


def _coverage(cases):
    """From the expected fields of lone-cell cases: which (target column mod 64, window bit) and (target-row parity, row offset
    + k) pairs are reached, and how many reached cells lie in no source's window."""
    k, nx = cases[0].k, cases[0].nx
    cols = np.zeros((min(64, nx), 2 * k + 1), bool)
    rows = np.zeros((2, 2 * k + 1), bool)
    outside = 0
    off = np.arange(-k, k + 1)
    for c in cases:
        reached = np.abs(dc.expected(c)) < BIG
        inwin = np.zeros_like(reached)
        for i, j in np.argwhere(c.coast > 0):
            ys = i + off
            ys = ys[(ys >= 0) & (ys < c.ny)]
            xs = (j + off) % nx                                  # target j + off sees the source at window bit k - off
            Y, X = np.meshgrid(ys, xs, indexing="ij")
            B = np.broadcast_to((k - off)[None, :], Y.shape)
            hit = reached[Y, X]
            inwin[Y, X] = True
            cols[(X % 64)[hit], B[hit]] = True
            rows[(Y % 2)[hit], (i - Y + k)[hit]] = True
        outside += int((reached & ~inwin).sum())
    return cols, rows, outside


@pytest.mark.parametrize("shape", dc.SHAPES, ids=SHAPE_IDS)
def test_coverage_of_columns_bits_rows_and_offsets(shape):
    cases = [c for c in dc.cases_of(shape) if c.family == "A"]
    cols, rows, outside = _coverage(cases)
    assert cols.all(), np.argwhere(~cols)[:8]
    assert rows.all(), np.argwhere(~rows)[:8]
    assert outside == 0
    # the seams by name hold a source in some field, in rows of both parities; so do the named rows
    k, nx, ny = shape.k, shape.nx, dc.ny_of(shape.k)
    src = np.concatenate([np.argwhere(c.coast > 0) for c in cases if c.cset == 1 and c.maxdist < dc.FAR])
    named = [0, 1, k - 1, k, k + 1, nx - 1, nx - 2, nx - k - 1, nx - k, 63, 64, 255, 256, 64 * (nx // 64)] + list(range(32, nx, 64))
    assert {c for c in named if 0 <= c < nx} <= set(src[:, 1]) and set(range(min(64, nx))) <= set(src[:, 1] % 64)
    assert {0, 1, k, ny - 1, ny - 2, ny - 1 - k} <= set(src[:, 0]) and set(src[:, 0] % 2) == {0, 1}
    # with the reset inside the reach alone, part of the early class is out of reach: that is what maxdist is chosen for
    near = [c for c in cases if c.maxdist < dc.FAR]
    if k >= 15:
        assert not _coverage(near)[1].all()
    if shape.kernel == "WIDE":                                   # k_dist_wide's pass boundaries, both target-row parities
        for d in (30, 31, 32, 61, 62, 63):
            if d <= k:
                assert rows[:, k - d].all() and rows[:, k + d].all(), d


def _mutant_counts(kernel):
    """{mutant: [(case name, family, set, cells moved)]} over a kernel's Family B and C cases and its first Family A field."""
    out = {m: [] for m in dist_ref.MUTANTS}
    for s in dc.SHAPES:
        if s.kernel != kernel:
            continue
        for c in dc.cases_of(s):
            if c.family == "A" and "-A0-" not in c.name:
                continue
            for m in dist_ref.MUTANTS:
                if m == "index_nearest" and (c.family != "B" or c.k > 40):     # (its table grows with k cubed)
                    continue
                if m == "side_class" and c.family != "C":
                    continue
                got = dist_ref.dist_model(c.coast, c.mask, c.lon, c.lat, c.maxdist, c.k, mutate=m)
                out[m].append((c.name, c.family, c.cset, dist_ref.moved(got, dc.expected(c))))
    return out


@pytest.mark.parametrize("kernel", dc.KERNELS)
def test_each_mutant_moves_cells(kernel):
    counts = _mutant_counts(kernel)
    for m in ("k-1", "k+1", "noreset", "reset_after_min", "side_class", "rowstop"):
        best = max(n for _, _, _, n in counts[m])
        print(f"{kernel} {m}: {best} / {sum(n > 0 for _, _, _, n in counts[m])} of {len(counts[m])}")
        assert best >= 20, (kernel, m, best)
    assert all(f == "C" for _, f, _, _ in counts["side_class"])
    # index-nearest (module docstring): exact under sets 1, 3 and 4, wrong where a regional frame's window crosses the seam
    per_set = {n: [(name, v) for name, _, cs, v in counts["index_nearest"] if cs == n] for n in (1, 2, 3, 4)}
    print(f"{kernel} index_nearest: " + ", ".join(f"set {n}: {max(v for _, v in per_set[n])} / "
                                                 f"{sum(v > 0 for _, v in per_set[n])} of {len(per_set[n])}" for n in per_set))
    for n in (1, 3, 4):
        assert per_set[n] and all(v == 0 for _, v in per_set[n]), (n, [x for x in per_set[n] if x[1]])
    assert max(v for _, v in per_set[2]) >= 20, per_set[2]


@pytest.mark.parametrize("shape", dc.SHAPES, ids=SHAPE_IDS)
def test_no_reset_on_a_knife_edge(shape):
    beyond = 0
    for c in list(dc.cases_of(shape)) + [dc.value_case(s) for s in dc.VALUE_SHAPES if s == shape]:
        early, _ = dist_ref.dist_planes(c.coast, c.lon, c.lat, c.k)
        e = early[np.isfinite(early)]
        assert e.size and not np.any(np.abs(e / (2 * c.maxdist) - 1.0) < 1e-4), c.name
        # 2 maxdist inside the reach: early minima on both sides of it (a lone cell in the last row has none beyond it)
        if c.k >= 1 and c.family in "BC":
            assert np.any(e > 2 * c.maxdist) and np.any(e < 2 * c.maxdist), c.name
        if c.k >= 1 and c.family == "A" and c.maxdist < dc.FAR:
            assert np.any(e < 2 * c.maxdist), c.name
            beyond += int(np.any(e > 2 * c.maxdist))
    assert shape.k == 0 or beyond >= 4
