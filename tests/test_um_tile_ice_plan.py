"""What an ice call of one UM tile decides on the host (seabreeze_param_amd/csrc/sb_ice_plan.hpp: sb_um_tile_ice_plan,
sb_um_tile_ice_reach): the refusals, the source rectangle, the sizes of the planes, and which workgroups of the tile distance
kernel (4 rows x 64 columns of the interior) a changed word of the rectangle's coast bit plane marks -- the same function
k_edge_bits_delta's tile instance marks with on the device.

tests/um_tile_ice_plan_dump.cpp is built host-only.  Every word of every case's source rectangle is walked.  Lower bound: a
brute force over targets (tests/um_tile_ice_ref.py, tests/um_ice_ref.py) -- every target whose window holds a cell of the word
lies in a marked workgroup.  Upper bound: no marked workgroup lies wholly outside rows y-wj-3 .. y+wj+3 and columns
x-wi-63 .. x+63+wi+63 of the word's first cell (x, y) (whole words, whole row groups, whole tiles: a condition of the design).
Copies of the rule narrowed on purpose -- the origin forgotten among them -- are caught by the lower bound.  Then, in numpy,
the argument the whole feature rests on: the whole-domain restatement run on a tile's source rectangle alone gives the
whole-domain field, on every one of the twelve ice planes.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import um_ice_cases as uic
import um_ice_ref as uir
import um_setup_ref as ur
import um_tile_ice_ref as uti
import um_tile_ref as ut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#         nx   ny   window      beyond (W, E, S, N)
CASES = [(124, 23, (15, 15), (10, 66, 0, 47)),       # case a's tile (10, 134, 0, 23): eW = 10, a word straddles the west edge
         (10, 23, (15, 15), (0, 190, 23, 24)),       # nx < 64, an edge side, sides beyond the window
         (13, 6, (40, 9), (70, 117, 9, 15)),         # the 13 x 6 tile of um_tile_ref.SPARSE_CUTS' unequal cut
         (13, 9, (40, 9), (70, 117, 6, 55)),         # case b's: 6 < 9 rows to the domain's edge
         (117, 55, (40, 9), (83, 0, 15, 0)),
         (67, 23, (0, 0), (67, 66, 23, 24)),
         (65, 19, (255, 255), (0, 65, 0, 18)),       # every e* clipped by beyond
         (65, 18, (255, 255), (65, 0, 19, 0)),
         (200, 70, (15, 15), (0, 0, 0, 0))]          # the whole domain: sb_um_ice_reach itself
IDS = ["%dx%d-%s-%s" % (c[0], c[1], "x".join(map(str, c[2])), "/".join(map(str, c[3]))) for c in CASES]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("um_tile_ice_plan_dump") / "dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-x", "c++", os.path.join(ROOT, "tests", "um_tile_ice_plan_dump.cpp"), "-o", exe],
                   check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        res = {ln.split()[0]: ln.split()[1:] for ln in out}
        assert len(res) == len(lines)
        return res
    return run


def _marks(f, nx, ny):
    assert (int(f[0]), int(f[1])) == (uir.groups(ny), uir.tiles(nx))
    return np.array(f[2:], int).reshape(uir.groups(ny), uir.tiles(nx)).astype(bool)


def _marks_of_words(dump, nx, ny, win, beyond):
    """{(x0, s): marks} of every word of the source rectangle, each marked alone"""
    e = uti.sources(win, beyond)
    words = [(x0, s) for s in range(ny + e[2] + e[3]) for x0 in range(0, nx + e[0] + e[1], 64)]
    got = dump([f"M w{x0}s{s} {nx} {ny} {win[0]} {win[1]} {' '.join(map(str, beyond))} 1 {x0} {s}" for x0, s in words])
    return {(x0, s): _marks(got[f"w{x0}s{s}"], nx, ny) for x0, s in words}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_word(dump, case):
    nx, ny, win, beyond = case
    e = uti.sources(win, beyond)
    narrowed = {"origin": 0, "wj-1": 0, "no +63": 0}
    for (x0, s), marks in _marks_of_words(dump, nx, ny, win, beyond).items():
        cells = uti.word_cells(nx, e, x0, s)
        assert cells and all(-e[0] <= x < nx + e[1] and -e[2] <= y < ny + e[3] for x, y in cells)
        need = uti.brute_marks(nx, ny, win, cells)
        assert need.any(), (x0, s)                                # e* <= the window: every source cell has a target
        assert not (need & ~marks).any(), (x0, s, np.argwhere(need & ~marks)[:5])
        cap = uti.cap_marks(nx, ny, win, e, cells)
        assert not (marks & ~cap).any(), (x0, s, np.argwhere(marks & ~cap)[:5])
        # the Python restatement the other tests model the marks with is the header's rule
        assert np.array_equal(uti.word_marks(nx, ny, win, e, cells), marks), (x0, s)
        if beyond == (0, 0, 0, 0):
            assert np.array_equal(uir.word_marks(nx, ny, *win, [(x0, s)]), marks)
        if win == (255, 255):
            assert marks.all()
        for nm, kw in (("origin", dict(shift=(0, 0))), ("wj-1", dict(dwj=-1)), ("no +63", dict(tail=0))):
            narrowed[nm] += int((need & ~uti.word_marks(nx, ny, win, e, cells, **kw)).any())
    # the origin forgotten shows where the shift by (eW, eS) carries a reach's first column or row across a tile's or a
    # row group's edge (eW = 40, eS = 9 below; eW = 10 alone moves no reach of the first case across one); the other two as
    # in tests/test_um_ice_plan.py
    if (nx, ny, win) == (124, 23, (15, 15)):
        assert narrowed["wj-1"] > 0 and narrowed["no +63"] > 0, narrowed
    if (nx, ny, win) == (117, 55, (40, 9)):
        assert narrowed["origin"] > 0 and narrowed["wj-1"] > 0, narrowed
    if beyond == (0, 0, 0, 0):
        assert narrowed["origin"] == 0


def test_a_word_straddles_the_interiors_west_edge(dump):
    """eW = 10: the rectangle's first word holds ghost columns -10 .. -1 and interior columns 0 .. 53; a flip in ghost column
    -10 alone (brute force: columns 0 .. 5) is marked as the whole word (columns 0 .. 68: two tiles)"""
    nx, ny, win, beyond = CASES[0]
    e = uti.sources(win, beyond)
    assert e == (10, 15, 0, 15) and uti.words_of([(-10, 4)], e) == [(0, 4)] == uti.words_of([(53, 4)], e)
    marks = _marks_of_words(dump, nx, ny, win, beyond)[(0, 4)]
    assert marks[:, :2].any(axis=0).all() and uti.brute_marks(nx, ny, win, [(-10, 4)])[:, 1:].sum() == 0


def test_many_words_mark_the_union(dump):
    nx, ny, win, beyond = CASES[4]
    e = uti.sources(win, beyond)
    rng = np.random.default_rng(7)
    cells = [(int(rng.integers(-e[0], nx + e[1])), int(rng.integers(-e[2], ny + e[3]))) for _ in range(12)]
    words = uti.words_of(cells, e)
    got = dump([" ".join(["M u", str(nx), str(ny), str(win[0]), str(win[1])] + [str(b) for b in beyond] + [str(len(words))] +
                         [f"{x0} {s}" for x0, s in words])])["u"]
    marks = _marks(got, nx, ny)
    assert not (uti.brute_marks(nx, ny, win, cells) & ~marks).any()
    assert not (marks & ~uti.cap_marks(nx, ny, win, e, cells)).any()
    assert np.array_equal(marks, uti.word_marks(nx, ny, win, e, cells))


def test_path_sizes_and_refusals(dump):
    # (nx, ny, hi, hj, wi, wj, bW, bE, bS, bN, incremental) -> PATH eW eE eS eN nw rows tiles
    want = {(124, 23, 17, 17, 15, 15, 10, 66, 0, 47, 1): "DELTA 10 15 0 15 3 6 2",
            (124, 23, 16, 16, 15, 15, 10, 66, 0, 47, 0): "WHOLE 10 15 0 15 3 6 2",
            (13, 6, 41, 10, 40, 9, 70, 117, 9, 15, 1): "DELTA 40 40 9 9 2 2 1",
            (65, 19, 66, 19, 255, 255, 0, 65, 0, 18, 1): "DELTA 0 65 0 18 3 5 2",
            (200, 70, 1, 1, 15, 15, 0, 0, 0, 0, 1): "DELTA 0 0 0 0 4 18 4",      # the whole domain: sb_um_ice_plan's sizes
            (67, 23, 1, 1, 0, 0, 67, 66, 23, 24, 1): "DELTA 0 0 0 0 2 6 2",        # no window: the ring alone
            # a halo below e* + 1 on one side each, and below 1 on an edge side
            (124, 23, 15, 17, 15, 15, 10, 66, 0, 47, 1): "NONE", (124, 23, 17, 15, 15, 15, 10, 66, 0, 47, 1): "NONE",
            (124, 23, 10, 17, 15, 15, 10, 0, 0, 47, 1): "NONE", (124, 23, 17, 0, 15, 15, 10, 66, 0, 0, 1): "NONE",
            (124, 23, 11, 1, 15, 15, 10, 0, 0, 0, 1): "DELTA 10 0 0 0 3 6 2",
            # sizes, windows, a negative beyond
            (0, 23, 17, 17, 15, 15, 10, 66, 0, 47, 1): "NONE", (124, 0, 17, 17, 15, 15, 10, 66, 0, 47, 1): "NONE",
            (124, 23, 300, 300, 256, 15, 0, 0, 0, 0, 1): "NONE", (124, 23, 300, 300, 15, 256, 0, 0, 0, 0, 1): "NONE",
            (124, 23, 17, 17, -1, 15, 10, 66, 0, 47, 1): "NONE", (124, 23, 17, 17, 15, -1, 10, 66, 0, 47, 0): "NONE",
            (124, 23, 17, 17, 15, 15, -1, 66, 0, 47, 1): "NONE", (124, 23, 17, 17, 15, 15, 10, 66, 0, -2, 1): "NONE"}
    got = dump([f"P {'/'.join(map(str, key))} " + " ".join(map(str, key)) for key in want])
    for key, w in want.items():
        assert " ".join(got["/".join(map(str, key))]) == w, key


def test_report_bounds_of_the_written_test(dump):
    """The inputs of tests/test_um_tile_ice_gpu.py::test_only_marked_workgroups_are_written: for every tile the brute-force
    count lies at or below what the rule marks, that at or below the cap, and the cap leaves cells outside it in the tile
    that holds the flip -- so the sentinel of that test has somewhere to stand."""
    case, before, plane = uti.WRITTEN
    c = uti.CASES[case]
    H, land, lf_L, planes, co = uti.whole_inputs(case, 8)
    seen_ghost_only = seen_partial = False
    for t in ut.tiles(c["cuts"]):
        nx, ny = t[1] - t[0], t[3] - t[2]
        beyond = uti.beyond_of(t, c["nx"], c["ny"])
        e = uti.sources(c["win"], beyond)
        cells = uti.changed_cells(co[before], co[plane], t, e)
        lo, cap = uti.brute_marks(nx, ny, c["win"], cells), uti.cap_marks(nx, ny, c["win"], e, cells)
        words = uti.words_of(cells, e)
        if not words:
            assert not lo.any() and not cap.any()
            continue
        got = dump([" ".join(["M u", str(nx), str(ny), str(c["win"][0]), str(c["win"][1])] + [str(b) for b in beyond] +
                             [str(len(words))] + [f"{x0} {s}" for x0, s in words])])["u"]
        marks = _marks(got, nx, ny)
        assert lo.any() and not (lo & ~marks).any() and not (marks & ~cap).any(), t
        assert lo.sum() <= marks.sum() <= cap.sum()
        seen_ghost_only |= all(not (0 <= x < nx and 0 <= y < ny) for x, y in cells)
        seen_partial |= not cap.all()
    assert seen_ghost_only and seen_partial


# ---- the cut itself, in numpy ------------------------------------------------------------------------------------------

CUT = dict(nx=200, ny=70, win=(9, 5), cuts=((0, 6, 134, 200), (0, 23, 46, 70)), maxdist=180.0)


@pytest.mark.parametrize("grid", uic.GRIDS)
def test_source_rectangle_gives_the_whole_domain_field(grid):
    """200 x 70, window 9 x 5, a 3 x 3 cut whose second column of tiles lies 6 < 9 cells from the domain's edge.  On each of
    the twelve planes the whole-domain restatement run on a tile's source rectangle -- e* = min(window, beyond*) -- gives the
    whole-domain field cell for cell (tests/um_tile_ref.py's argument: the sweep classes are decided on differences), and
    the interior-only rule does not."""
    c, dt = CUT, np.float64
    nx, ny, win = c["nx"], c["ny"], c["win"]
    H = uti.halo_for(c)
    land, lf_L, planes = uic.make(nx, ny, H, dt)
    lat, lon = ur.grid_named(grid, nx, ny, dt)
    tiles = ut.tiles(c["cuts"])
    assert any(0 < b < w for t in tiles for b, w in zip(uti.beyond_of(t, nx, ny), (win[0], win[0], win[1], win[1])))
    done, interior_differs = {}, 0
    for n, ci in enumerate(planes):
        coast = np.ascontiguousarray(ur.edges_um(lf_L, ci, *H)[H[1]:H[1] + ny, H[0]:H[0] + nx])
        key = coast.tobytes()
        if key in done:
            continue
        done[key] = n
        whole = ut.whole_dist(coast, land, lat, lon, *win, c["maxdist"])
        assert (np.abs(whole) < 12000.0).any() and (whole >= 12000.0).any()
        for t in tiles:
            x0, x1, y0, y1 = t
            e = uti.sources(win, uti.beyond_of(t, nx, ny))
            # the source rectangle is um_tile_ref's extended rectangle: the window clipped at the domain's edge
            assert ut.extended(t, nx, ny, *win) == (x0 - e[0], x1 + e[1], y0 - e[2], y1 + e[3])
            got = ut.tile_dist(coast, land, lat, lon, t, *win, c["maxdist"])
            assert np.array_equal(got, whole[y0:y1, x0:x1]), (uic.PLANES[n], t)
            interior_differs += int(not np.array_equal(ut.tile_dist(coast, land, lat, lon, t, *win, c["maxdist"], reach=(0, 0)),
                                                       whole[y0:y1, x0:x1]))
    assert len(done) >= 8 and interior_differs > 0
