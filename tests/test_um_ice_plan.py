"""What an ice call of the UM layout decides on the host (seabreeze_param_amd/csrc/sb_ice_plan.hpp): which path it takes,
the sizes of its planes, and which workgroups of the UM distance kernels (4 rows x 64 columns) a changed word of the coast
bit plane marks -- the same sb_um_ice_reach that k_edge_bits_delta's UM instance marks with on the device.

tests/plan_dump.cpp (its `um_ice` lines) is built host-only with the compiler that builds the library.  Every word (x0, y) of every case
is walked.  Lower bound: a brute force over targets (tests/um_ice_ref.py) -- every target whose window holds a cell of the
word lies in a marked workgroup; under-marking would leave a stale distance.  Upper bound: no marked workgroup lies wholly
outside rows y-wj-3 .. y+wj+3 and columns x0-wi-63 .. x0+63+wi+63 (whole words, whole row groups, whole tiles: a condition
of the design, not a measurement).  A copy of the rule narrowed on purpose is caught by the lower bound.
"""
import numpy as np
import pytest

import plan_dump
import um_ice_ref as uir

#         nx   ny   wi   wj
CASES = [(200, 70, 0, 0), (200, 70, 7, 3), (200, 70, 15, 15), (200, 70, 40, 33), (130, 37, 255, 255), (64, 4, 15, 15),
         (65, 5, 15, 15)]
IDS = ["%dx%d-%d-%d" % c for c in CASES]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return plan_dump.ice_dump(tmp_path_factory, "um_ice")


def _word_cells(nx, x0, y):
    return [(x, y) for x in range(x0, min(x0 + 64, nx))]


def _marks_of_words(dump, nx, ny, wi, wj):
    """{(x0, y): marks} of every word of the grid, each marked alone"""
    words = [(x0, y) for y in range(ny) for x0 in range(0, nx, 64)]
    got = dump([f"M w{x0}y{y} {nx} {ny} {wi} {wj} 1 {x0} {y}" for x0, y in words])
    res = {}
    for x0, y in words:
        f = got[f"w{x0}y{y}"]
        assert (int(f[0]), int(f[1])) == (uir.groups(ny), uir.tiles(nx))
        res[(x0, y)] = np.array(f[2:], int).reshape(uir.groups(ny), uir.tiles(nx)).astype(bool)
    return res


def _box(nx, ny, c0, c1, r0, r1):
    """the workgroups that hold a cell of columns c0 .. c1, rows r0 .. r1 (clipped to the interior)"""
    m = np.zeros((uir.groups(ny), uir.tiles(nx)), bool)
    c0, c1, r0, r1 = max(c0, 0), min(c1, nx - 1), max(r0, 0), min(r1, ny - 1)
    m[r0 // uir.ROWS:r1 // uir.ROWS + 1, c0 // uir.COLS:c1 // uir.COLS + 1] = True
    return m


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_word(dump, case):
    nx, ny, wi, wj = case
    narrowed = {"wi-1": 0, "wj-1": 0, "no +63": 0}
    for (x0, y), marks in _marks_of_words(dump, nx, ny, wi, wj).items():
        cells = _word_cells(nx, x0, y)
        # the lower bound: the targets whose window holds a cell of the word, cell by cell (a box per cell: the brute force
        # of um_ice_ref.brute_marks, which test_brute_force_is_the_box pins against its loops)
        need = np.zeros_like(marks)
        for x, _ in cells:
            need |= _box(nx, ny, x - wi, x + wi, y - wj, y + wj)
        assert need.any()
        assert not (need & ~marks).any(), (x0, y, np.argwhere(need & ~marks)[:5])
        cap = uir.cap_marks(nx, ny, wi, wj, [(x0, y)])
        assert not (marks & ~cap).any(), (x0, y, np.argwhere(marks & ~cap)[:5])
        # the Python restatement the other tests model the marks with is the header's rule
        assert np.array_equal(uir.word_marks(nx, ny, wi, wj, [(x0, y)]), marks), (x0, y)
        # no wrap: a word at the west edge marks the east edge only where the window reaches it
        if x0 == 0 and 63 + wi < nx - 1 - (nx - 1) % 64:
            assert not marks[:, -1].any(), (x0, y)
        if (nx, ny, wi, wj) == (130, 37, 255, 255):
            assert marks.all()
        # a rule narrowed on purpose leaves a needed workgroup unmarked somewhere: the bound bites
        for nm, kw in (("wi-1", dict(dwi=-1)), ("wj-1", dict(dwj=-1)), ("no +63", dict(tail=0))):
            narrowed[nm] += int((need & ~uir.word_marks(nx, ny, wi, wj, [(x0, y)], **kw)).any())
    # wj-1 shows wherever a reach ends on a row group's edge and does not cover the grid; dropping the +63 wherever the
    # window leaves the word's own tile (wi > 0) and a tile lies east of it.  wi-1 shows only where a reach ends exactly on
    # a tile's edge, wi = 1 mod 64: none of these windows -- test_narrowed_columns_are_caught_at_a_tile_edge
    if (nx, ny) == (200, 70) and (wi, wj) != (0, 0):
        assert narrowed["wj-1"] > 0 and narrowed["no +63"] > 0, narrowed
    if (nx, ny) == (65, 5):
        assert narrowed["no +63"] > 0, narrowed
    assert narrowed["wi-1"] == 0


def test_narrowed_columns_are_caught_at_a_tile_edge(dump):
    """wi-1 shows only where the reach ends exactly on a tile's first or last column: 200 x 70 with wi = 1 -- the word at
    columns 64 .. 127 reaches column 63, the last of tile 0."""
    nx, ny, wi, wj = 200, 70, 1, 3
    marks = _marks_of_words(dump, nx, ny, wi, wj)[(64, 10)]
    need = np.zeros_like(marks)
    for x, y in _word_cells(nx, 64, 10):
        need |= _box(nx, ny, x - wi, x + wi, y - wj, y + wj)
    assert not (need & ~marks).any()
    assert (need & ~uir.word_marks(nx, ny, wi, wj, [(64, 10)], dwi=-1)).any()


def test_brute_force_is_the_box():
    """the per-cell box of test_every_word is the brute force over targets"""
    rng = np.random.default_rng(3)
    for nx, ny, wi, wj in ((200, 70, 7, 3), (65, 5, 15, 15), (130, 37, 255, 255), (200, 70, 0, 0)):
        for _ in range(4):
            x, y = int(rng.integers(nx)), int(rng.integers(ny))
            assert np.array_equal(uir.brute_marks(nx, ny, wi, wj, [(x, y)]), _box(nx, ny, x - wi, x + wi, y - wj, y + wj))


def test_many_words_mark_the_union(dump):
    nx, ny, wi, wj = 200, 70, 7, 3
    rng = np.random.default_rng(7)
    cells = [(int(rng.integers(nx)), int(rng.integers(ny))) for _ in range(12)]
    got = dump([" ".join(["M u", str(nx), str(ny), str(wi), str(wj), str(len(cells))] + [f"{x} {y}" for x, y in cells])])["u"]
    marks = np.array(got[2:], int).reshape(int(got[0]), int(got[1])).astype(bool)
    assert not (uir.brute_marks(nx, ny, wi, wj, cells) & ~marks).any()
    assert not (marks & ~uir.cap_marks(nx, ny, wi, wj, cells)).any()
    assert np.array_equal(marks, uir.word_marks(nx, ny, wi, wj, cells))


def test_path_sizes_and_refusal(dump):
    # (nx, ny, hi, hj, wi, wj, incremental) -> what
    want = {(200, 70, 15, 15, 15, 15, 1): "DELTA 4 18 4", (200, 70, 15, 15, 15, 15, 0): "WHOLE 4 18 4",
            (64, 4, 1, 1, 0, 0, 1): "DELTA 1 1 1", (65, 5, 2, 1, 255, 255, 1): "DELTA 2 2 2",
            (200, 70, 0, 1, 15, 15, 1): "NONE", (200, 70, 1, 0, 15, 15, 1): "NONE", (0, 70, 1, 1, 15, 15, 1): "NONE",
            (200, 0, 1, 1, 15, 15, 1): "NONE", (200, 70, 1, 1, 256, 15, 1): "NONE", (200, 70, 1, 1, 15, 256, 1): "NONE",
            (200, 70, 1, 1, -1, 15, 1): "NONE", (200, 70, 1, 1, 15, -1, 0): "NONE"}
    got = dump([f"P {'/'.join(map(str, key))} " + " ".join(map(str, key)) for key in want])
    for key, w in want.items():
        assert " ".join(got["/".join(map(str, key))]) == w, key
