"""What an ice call of a latitude band decides on the host (seabreeze_param_amd/csrc/sb_ice_plan.hpp): whether the band has
a plan at all (a cut side needs the (k+1)-th ghost row), which path it takes, and which (own row, 256-column tile) pairs a
changed word of the band's coast bit plane marks -- the same sb_band_ice_reach that k_edge_bits_delta's band instance marks
with on the device.

tests/plan_dump.cpp (its `band_ice` lines) is built host-only with the compiler that builds the library.  The expectation is a numpy
brute force over the distance kernels' window rule seen from a band (tests/band_ice_ref.py): every pair it finds must be
marked (under-marking would leave a stale distance), and no mark may lie outside rows +-k and the tile columns covering
+-(k + 63) of a changed cell (the cap is a condition of the design -- a word is 64 cells --, not a measurement).  Every word
of every source row is walked, once through its first cell and once through its last, for the shapes of
tests/test_band_ice_gpu.py.
"""
import numpy as np
import pytest

import band_ice_ref
import plan_dump
from band_frames import cuts_of

#        id              nx  kwin halo  band heights
CASES = [("BITS32",      320, 15, 16, (33, 33, 33)),
         ("BITS32-halo", 320, 15, 19, (33, 33, 33)),
         ("BITS64",      320, 20, 21, (31, 36, 32)),
         ("BITS_SMALL",   96, 15, 16, (33, 33, 33)),
         ("BYTES",        24, 15, 16, (17, 21, 19)),
         ("WIDE",        320, 40, 41, (50, 50, 50)),
         ("WIDE-odd",    320, 40, 41, (49, 51, 50)),
         ("BITS32-700",  700, 15, 16, (33, 33, 33)),
         ("SMALL-70",     70, 15, 16, (33, 33, 33))]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return plan_dump.ice_dump(tmp_path_factory, "band_ice")


def _plan(dump, nx, ny, halo, south, north, k, inc=1):
    return dump([f"P p {nx} {ny} {halo} {int(south)} {int(north)} {k} {inc}"])["p"]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_word_of_every_source_row(dump, case):
    _, nx, k, halo, heights = case
    bands, nyg = cuts_of(heights), sum(heights)
    for g0, g1 in bands:
        south, north, ny = g0 == 0, g1 == nyg, g1 - g0
        plan = _plan(dump, nx, ny, halo, south, north, k)
        f0, nys, r0, r1, nw, nt = (int(v) for v in plan[1:])
        # the source rows are the model's, stated from the band's place on the globe alone
        s_lo, s_hi = band_ice_ref.source_rows(g0, g1, nyg, k)
        assert (nys, r0, r1, nt, nw) == (s_hi - s_lo, g0 - s_lo, g0 - s_lo + ny, band_ice_ref.tiles(nx), (nx + 63) // 64)
        assert f0 == halo - r0                                   # frame row of source row 0
        cases = {}
        for s in range(nys):
            for w in range(nw):
                for x in {64 * w, min(64 * w + 63, nx - 1)}:
                    cases[f"s{s}x{x}"] = (x, s)
        lines = [f"M {name} {nx} {ny} {halo} {int(south)} {int(north)} {k} 1 {x} {s}" for name, (x, s) in cases.items()]
        got = dump(lines)
        for name, (x, s) in cases.items():
            assert int(got[name][0]) == nt
            marks = np.array(got[name][1:], int).reshape(ny, nt).astype(bool)
            cells = [(x, s_lo + s)]
            need = band_ice_ref.brute_marks(nx, g0, g1, k, cells)
            cap = band_ice_ref.cap_marks(nx, g0, g1, k, cells)
            assert need.any(), (name, "a source row no own row can see")
            assert not (need & ~marks).any(), (g0, g1, name, np.argwhere(need & ~marks)[:5])
            assert not (marks & ~cap).any(), (g0, g1, name, np.argwhere(marks & ~cap)[:5])


def test_many_words_mark_the_union(dump):
    nx, k, halo, (g0, g1), nyg = 700, 15, 16, (33, 66), 99
    rng = np.random.default_rng(7)
    s_lo, s_hi = band_ice_ref.source_rows(g0, g1, nyg, k)
    cells = [(int(rng.integers(nx)), int(rng.integers(s_lo, s_hi))) for _ in range(12)]
    line = " ".join(["M u", str(nx), str(g1 - g0), str(halo), "0 0", str(k), str(len(cells))] + [f"{x} {s - s_lo}" for x, s in cells])
    got = dump([line])["u"]
    marks = np.array(got[1:], int).reshape(g1 - g0, int(got[0])).astype(bool)
    assert not (band_ice_ref.brute_marks(nx, g0, g1, k, cells) & ~marks).any()
    assert not (marks & ~band_ice_ref.cap_marks(nx, g0, g1, k, cells)).any()


def test_a_far_ghost_row_reaches_the_band_edge_only(dump):
    """700 x 33 own rows, k = 15, both sides cut: source row 0 (the 15th ghost row south) reaches own row 0 alone, and a
    cell at column 400 (its word: columns 384 .. 447, with the window 369 .. 462) its own tile alone."""
    got = dump(["M c 700 33 16 0 0 15 1 400 0"])["c"]
    m = np.array(got[1:], int).reshape(33, 3).astype(bool)
    assert m[0, 1] and m.sum() == 1


def test_path_and_refusal(dump):
    # (nx, ny, halo, south, north, k, incremental) -> path; NONE: no plan
    want = {(320, 33, 16, 0, 0, 15, 1): "DELTA", (320, 33, 16, 0, 0, 15, 0): "WHOLE", (24, 21, 16, 0, 0, 15, 1): "WHOLE",
            (96, 33, 16, 0, 1, 15, 1): "DELTA", (320, 50, 41, 1, 0, 40, 1): "DELTA", (30, 50, 41, 0, 0, 40, 1): "DELTA",
            (62, 40, 32, 0, 0, 31, 1): "WHOLE", (63, 40, 32, 0, 0, 31, 1): "DELTA",
            (320, 33, 15, 0, 0, 15, 1): "NONE", (320, 33, 15, 1, 0, 15, 1): "NONE", (320, 33, 15, 0, 1, 15, 1): "NONE",
            (320, 33, 15, 1, 1, 15, 1): "DELTA", (320, 33, 0, 1, 1, 15, 1): "DELTA", (320, 33, 0, 0, 1, 0, 1): "NONE",
            (320, 33, 1, 0, 0, 0, 1): "DELTA"}
    got = dump([f"P {'/'.join(map(str, key))} " + " ".join(map(str, key)) for key in want])
    for key, w in want.items():
        assert got["/".join(map(str, key))][0] == w, key
    # one band owning the globe without a halo: the frame is the grid
    assert got["320/33/0/1/1/15/1"][1:5] == ["0", "33", "0", "33"]
