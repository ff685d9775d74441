"""What get_dist decides before it launches (seabreeze_param_amd/csrc/sb_dist_plan.hpp): the cut bits, what the coordinates
allow, and which kernel runs.

tests/dist_plan_dump.cpp is built host-only with the compiler that builds the library and prints the decisions for every
case it is given.  The expectations below are written out by hand from the rules; nothing here is
produced by the header.  The kernels' tests on the GPU depend on the meaning of the four bits.
"""
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
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip("no hipcc to build tests/dist_plan_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("plan") / "dist_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-x", "c++", os.path.join(ROOT, "tests", "dist_plan_dump.cpp"), "-o", exe],
                   check=True)

    def run(lines):
        """-> {label: [fields]}"""
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        res = {ln.split()[0]: ln.split()[1:] for ln in out.splitlines()}
        assert len(res) == len(lines)
        return res
    return run


def _cuts_line(label, k, lon, lat):
    return " ".join(["C", label, str(k), str(len(lon)), str(len(lat))] + [repr(float(v)) for v in lon] + [repr(float(v)) for v in lat])


def test_cut_bits(dump):
    assert dump(["B bits"])["bits"] == ["1", "2", "4", "8"]
    assert (NEAREST, CIRCLE, INNER, ROWS) == (1, 2, 4, 8) and len({NEAREST, CIRCLE, INNER, ROWS}) == 4


KERNELS = {(512, 15): "BITS32", (512, 16): "BITS64", (287, 15): "BITS32", (286, 15): "BITS_SMALL", (63, 31): "BITS_SMALL",
           (62, 31): "BYTES", (258, 0): "BITS32", (257, 0): "BITS32", (256, 0): "BITS_SMALL", (1, 0): "BITS_SMALL",
           (40, 31): "BYTES", (30, 32): "WIDE", (512, 255): "WIDE"}


def test_kernel_choice(dump):
    got = dump([f"K {nx}/{k} {nx} {k}" for nx, k in KERNELS])
    for (nx, k), want in KERNELS.items():
        assert got[f"{nx}/{k}"] == [want], (nx, k)


def test_cuts(dump):
    ny = 40
    lat = -80.0 + 160.0 * np.arange(ny) / (ny - 1)
    glob = 0.703125 * np.arange(512)
    regional = np.linspace(100.0, 160.0, 150)
    ring = np.linspace(0.0, 357.6, 150)
    perm = np.random.default_rng(7).permutation
    lat91 = lat.copy()
    lat91[17] = 91.0
    cases = {
        "global_k9": (9, glob, lat, NEAREST | CIRCLE | INNER | ROWS),
        "global_k241": (241, glob, lat, 15),                     # 241 x 0.703125 = 169.45 degrees
        "global_k242": (242, glob, lat, ROWS),                   # 242 x 0.703125 = 170.15625 fails both 170-degree rules
        "regional_k9": (9, regional, lat, INNER | ROWS),         # closing step 300 degrees
        "regional_k0": (0, regional, lat, 15),
        "descending_k9": (9, np.linspace(357.6, 0.0, 150), lat, INNER | ROWS),
        "permuted_lon_k9": (9, ring[perm(150)], lat, ROWS),
        "doubled_lon_k9": (9, np.repeat(np.linspace(0.0, 357.6, 75), 2), lat, ROWS),
        "permuted_lat_k9": (9, glob, lat[perm(ny)], CIRCLE | INNER),
        "reversed_lat_k9": (9, glob, lat[::-1], 15),
        "lat91_k9": (9, glob, lat91, 0),
    }
    got = dump([_cuts_line(name, k, lon, la) for name, (k, lon, la, _) in cases.items()] + [_cuts_line("nx1", 0, [10.0], lat)])
    for name, (k, lon, la, want) in cases.items():
        assert [int(got[name][0]), int(got[name][1])] == [want, want], (name, got[name])
    # the traits themselves: circle, inner, latmono, maxstep, maxstep_inner (a swapped field would show here)
    tr = lambda name: [int(v) for v in got[name][2:5]] + [float(v) for v in got[name][5:7]]
    assert tr("global_k9") == [1, 1, 1, 0.703125, 0.703125]
    c, i, m, step, step_in = tr("regional_k9")
    assert (c, i, m) == (1, 1, 1) and abs(step - 300.0) < 1e-9 and abs(step_in - 60.0 / 149) < 1e-9
    c, i, m, step, step_in = tr("descending_k9")                 # every step is 357.6 degrees eastwards, 2.4 westwards
    assert (c, i, m) == (0, 1, 1) and abs(step_in - 2.4) < 1e-9
    assert tr("permuted_lat_k9")[:3] == [1, 1, 0] and tr("lat91_k9")[:3] == [0, 0, 0]
    assert tr("doubled_lon_k9")[:3] == [0, 0, 1]
    # one column: no column cut
    assert int(got["nx1"][0]) & ~ROWS == 0 and int(got["nx1"][1]) & ~ROWS == 0, got["nx1"]
