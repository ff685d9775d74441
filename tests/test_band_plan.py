"""What sb_band_get_dist_* decides on the host before it launches (seabreeze_param_amd/csrc/sb_dist_plan.hpp,
sb_band_rows): which rows of a band's ghost-celled frame may hold a source, which of them are targets, and that the
coordinate traits -- hence the cuts -- are formed over the latitudes of those rows alone, so that NaN in the entries
beyond a pole does not reach them.

tests/band_plan_dump.cpp is built host-only and prints the decisions; the expectations are written out by hand from the
rule in include/seabreeze_hip.h (kwin ghost rows on a cut side, none on a pole side)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAREST, CIRCLE, INNER, ROWS = 1, 2, 4, 8


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert shutil.which(cxx) or os.path.exists(cxx), "no hipcc to build tests/band_plan_dump.cpp with"
    exe = str(tmp_path_factory.mktemp("plan") / "band_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-x", "c++", os.path.join(ROOT, "tests", "band_plan_dump.cpp"), "-o", exe],
                   check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out.splitlines()}
        assert len(res) == len(lines)
        return res
    return run


#          ny halo south north k    f0  nys  r0  r1
ROWS_OF = {(33, 15, 0, 0, 15): (0, 63, 15, 48),       # an inner band: the whole frame
           (33, 19, 0, 0, 15): (4, 63, 15, 48),       # halo > kwin: the outer ghost rows are not sources
           (33, 15, 1, 0, 15): (15, 48, 0, 33),       # the south pole band: no source south of its first row
           (33, 15, 0, 1, 15): (0, 48, 15, 48),       # the north pole band
           (40, 0, 1, 1, 113): (0, 40, 0, 40),        # one band owning the globe: the grid
           (40, 7, 1, 1, 20): (7, 40, 0, 40),         # ... in a frame it does not need
           (240, 113, 0, 0, 113): (0, 466, 113, 353),
           (5, 4, 0, 0, 0): (4, 5, 0, 5)}             # a window of one cell reads no ghost row


def test_band_rows(dump):
    got = dump(["R {} {} {} {} {} {}".format("/".join(map(str, c)), *c) for c in ROWS_OF])
    for c, want in ROWS_OF.items():
        assert tuple(got["/".join(map(str, c))]) == want, c
        f0, nys, r0, r1 = want
        ny, halo, south, north, k = c
        assert r1 - r0 == ny and f0 + r0 == halo                       # the targets are the interior
        assert 0 <= f0 and f0 + nys <= ny + 2 * halo                   # the sources lie in the frame
        assert (r0 == 0) == bool(south or k == 0) and (r1 == nys) == bool(north or k == 0)


def _line(label, ny, halo, south, north, k, lon, latf):
    return " ".join(["T", label] + [str(v) for v in (ny, halo, south, north, k, len(lon))]
                    + [repr(float(v)) for v in lon] + [repr(float(v)) for v in latf])


def test_traits_see_only_the_rows_that_are_read(dump):
    nx, ny, halo, k = 64, 12, 6, 4
    lon = 360.0 * np.arange(nx) / nx
    lat = 30.0 + 0.5 * np.arange(ny + 2 * halo)
    full = NEAREST | CIRCLE | INNER | ROWS
    nan_s, nan_n = lat.copy(), lat.copy()
    nan_s[:halo] = np.nan
    nan_n[-halo:] = np.nan
    bad_outer = lat.copy()
    bad_outer[:halo - k] = 500.0                                        # beyond the window: not looked at
    bad_outer[-(halo - k):] = -500.0
    bad_inner = lat.copy()
    bad_inner[halo - 1] = lat[halo + 1]                                  # a ghost row in reach breaks the order
    got = dump([_line("inner", ny, halo, 0, 0, k, lon, lat),
                _line("south-nan", ny, halo, 1, 0, k, lon, nan_s),
                _line("north-nan", ny, halo, 0, 1, k, lon, nan_n),
                _line("south-nan-as-cut", ny, halo, 0, 0, k, lon, nan_s),
                _line("outer", ny, halo, 0, 0, k, lon, bad_outer),
                _line("reach", ny, halo, 0, 0, k, lon, bad_inner),
                _line("reach-at-pole", ny, halo, 1, 0, k, lon, bad_inner)])
    assert got["inner"] == [full, 1, 1, 1]
    assert got["south-nan"] == [full, 1, 1, 1] and got["north-nan"] == [full, 1, 1, 1]
    assert got["south-nan-as-cut"] == [0, 0, 0, 0]                       # (NaN that IS read switches every cut off)
    assert got["outer"] == [full, 1, 1, 1]
    assert got["reach"] == [CIRCLE | INNER, 1, 1, 0]                     # no row cut, hence no NEAREST
    assert got["reach-at-pole"] == [full, 1, 1, 1]
