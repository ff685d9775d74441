"""What an ice call of a stream decides on the host (seabreeze_param_amd/csrc/sb_ice_plan.hpp): which path it takes, and
which (target row, 256-column tile) pairs a changed word of the coast bit plane marks -- the same sb_ice_reach that
k_edge_bits_delta's whole-grid instance marks with on the device.

tests/plan_dump.cpp (its `ice` lines) is built host-only with the compiler that builds the library.  The expectation is a numpy brute
force over the distance kernels' window rule (tests/ice_ref.py): every pair it finds must be marked (under-marking would
leave a stale distance), and no mark may lie outside rows +-k and the tile columns covering +-(k + 63) of a changed cell
(the cap is a condition of the design -- a word is 64 cells --, not a measurement).
"""
import numpy as np
import pytest

import ice_ref
import plan_dump

GRIDS = [(330, 40, 6), (200, 40, 6), (330, 60, 20), (700, 100, 40), (70, 40, 31), (24, 20, 15)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return plan_dump.ice_dump(tmp_path_factory, "ice")


def _cases(nx, ny, k):
    """label -> changed cells: every directed cell alone, the directed cells together, random sets of 1, 3 and 12 cells"""
    rng = np.random.default_rng(1000 * nx + k)
    cols = sorted({c for c in (0, 63, 64, nx - 1) if c < nx})
    rows = (0, ny // 2, ny - 1)
    cases = {f"d{x}_{y}": [(x, y)] for x in cols for y in rows}
    cases["dall"] = [(x, y) for x in cols for y in (0, ny - 1)]
    for n in (1, 1, 1, 3, 3, 12):
        cases[f"r{len(cases)}"] = [(int(rng.integers(nx)), int(rng.integers(ny))) for _ in range(n)]
    return cases


def _marks(dump, nx, ny, k, cases):
    lines = [" ".join(["M", name, str(nx), str(ny), str(k), str(len(cells))] + [f"{x} {y}" for x, y in cells])
             for name, cells in cases.items()]
    got = dump(lines)
    out = {}
    for name in cases:
        nt = int(got[name][0])
        assert nt == ice_ref.tiles(nx)
        out[name] = np.array(got[name][1:], int).reshape(ny, nt).astype(bool)
    return out


@pytest.mark.parametrize("nx,ny,k", GRIDS)
def test_marks_cover_the_reach_and_stay_within_the_cap(dump, nx, ny, k):
    cases = _cases(nx, ny, k)
    marks = _marks(dump, nx, ny, k, cases)
    for name, cells in cases.items():
        need = ice_ref.brute_marks(nx, ny, k, cells)
        cap = ice_ref.cap_marks(nx, ny, k, cells)
        assert need.any() and not (need & ~cap).any()
        assert not (need & ~marks[name]).any(), (name, cells, np.argwhere(need & ~marks[name])[:5])
        assert not (marks[name] & ~cap).any(), (name, cells, np.argwhere(marks[name] & ~cap)[:5])


def test_a_change_in_one_tile_leaves_the_far_tiles_clean(dump):
    """700 x 96, k = 6: a cell at column 20 reaches columns 14 .. 26 (tile 0); its word reaches -6 .. 69, round the seam into
    the last tile, and never tile 1."""
    m = _marks(dump, 700, 96, 6, {"c": [(20, 40)]})["c"]
    assert m[34:47, 0].all() and not m[:, 1].any() and not m[:34].any() and not m[47:].any()
    assert m.sum() in (13, 26)                                   # tile 0 alone, or with the seam's tile 2


def test_path(dump):
    want = {(330, 6, 1): "DELTA", (200, 6, 1): "DELTA", (330, 20, 1): "DELTA", (700, 40, 1): "DELTA", (70, 31, 1): "DELTA",
            (24, 15, 1): "WHOLE", (62, 31, 1): "WHOLE", (63, 31, 1): "DELTA", (30, 32, 1): "DELTA",
            (330, 6, 0): "WHOLE", (700, 40, 0): "WHOLE", (24, 15, 0): "WHOLE"}
    got = dump([f"P {nx}/{k}/{inc} {nx} {k} {inc}" for nx, k, inc in want])
    for (nx, k, inc), w in want.items():
        assert got[f"{nx}/{k}/{inc}"] == [w], (nx, k, inc)
