"""The reference of sigma's statistics (tests/stats_ref.py) against itself, and the host's moment functions of
seabreeze_param_amd/csrc/sb_device.hpp (moments_empty, moments_merge, moments_of_shifted) against it.

tests/moments_dump.cpp reads a partitioned sample from standard input and prints what those functions make of it, combined
in the orders the kernels use (its header lists them).  sb_device.hpp includes the HIP runtime's header, so the program
is compiled as HIP for gfx950; its main calls host functions only and never initialises a device.  Every result is held to
the bounds of tests/stats_ref.py: no tolerance here is fitted to what the functions return.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import stats_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
NY, NX = 75, 130
TAGS = ("seq", "wave", "shifted")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip("no hipcc to build tests/moments_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("moments") / "moments_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "--offload-arch=gfx950", "-x", "hip", os.path.join(ROOT, "tests", "moments_dump.cpp"),
                    "-o", exe], check=True)

    def run(parts):
        """parts: a list of 1-D float64 arrays -> {tag: five float64}"""
        text = [str(len(parts))] + [" ".join([str(len(p))] + [float(v).hex() for v in p]) for p in parts]
        env = dict(os.environ, HIP_VISIBLE_DEVICES="")          # (nothing in the program asks for a device)
        out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True, env=env).stdout
        res = {}
        for ln in out.split("\n")[:-1]:
            tag, *vals = ln.split()
            res[tag] = (np.array([float.fromhex(v) for v in vals]), vals)
        return res
    return run


def _field(name, dtype, **kw):
    """the field as a kernel sees it: rounded to the working precision, then widened"""
    return sr.family(name, NY, NX, seed=7, **kw).astype(dtype)


def _cut(x, sizes):
    """x.ravel() cut into consecutive parts of the given sizes (the last one takes the rest)"""
    flat = x.ravel().astype(np.float64)
    edges = np.minimum(np.cumsum([0] + list(sizes)), flat.size)
    parts = [flat[a:b] for a, b in zip(edges[:-1], edges[1:])]
    return parts + [flat[edges[-1]:]]


def _schemes(n):
    """name -> part sizes; what is left of the sample forms a last part"""
    rng = np.random.default_rng(5)
    sch = {"one": [], "two": [n // 3], "unequal": [1, 2, 9, 128, 700, 3, 4000],
           "singles": [1] * 40,
           "empty_first": [0, 17, 900], "empty_middle": [300, 0, 0, 45], "empty_last": [n - 1000, 1000, 0]}
    for k in (63, 64, 65, 130):
        cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False))
        sch[f"k{k}"] = list(np.diff(np.concatenate([[0], cuts])))
    return sch


SCHEMES = sorted(_schemes(NY * NX))


# ---------------------------------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sr.FAMILIES)
def test_ref_moments_of_a_field_is_the_merge_of_its_bands(name, dtype):
    """two passes over the whole field and a Chan merge of two passes over each band agree in long double, to the
    bounds of stats_ref with long double's unit roundoff in place of double's"""
    x = _field(name, dtype)
    whole = sr.ref_moments(x)
    u_ld = float(np.finfo(LD).eps) / 2
    for rows in ([1, 2, 9, 63], [75], [1] * 75, [37, 38]):
        acc = (LD(0), LD(0), LD(0), LD(np.inf), LD(-np.inf))
        r0 = 0
        for k in rows:
            b = sr.ref_moments(x[r0:r0 + k])
            acc = sr.ref_merge(acc, (b.n, b.mean, b.M2, b.mn, b.mx))
            r0 += k
        assert r0 == NY and acc[0] == whole.n and acc[3] == whole.mn and acc[4] == whole.mx
        # (a merge rounds the mean once more per band: len(rows) roundings of at most u |x|max each)
        assert abs(acc[1] - whole.mean) <= whole.mean_bound(u_ld) + len(rows) * u_ld * max(abs(whole.mn), abs(whole.mx))
        assert abs(acc[2] - whole.M2) <= whole.m2_bound(u_ld)


def test_families_are_what_the_tests_take_them_for():
    for dtype in (np.float64, np.float32):
        m = {name: sr.ref_moments(_field(name, dtype)) for name in sr.FAMILIES}
        assert 9.0e3 < m["outlier_first"].kappa < 1.0e4 and m["outlier_first"].c == 800
        assert m["negative"].mx < -990 and m["plain"].mn >= 0
        assert m["orography"].c == 0 and m["orography"].mn == 0 and 0.01 < np.mean(_field("orography", dtype) > 0) < 0.06
        assert m["tight_far"].c == 1010 and m["tight_far"].kappa > 1e3
        assert m["constant"].M2 == 0 and m["constant"].kappa == 0 and m["constant"].mn == m["constant"].mx == 3.25
        for name, mm in m.items():
            sr.assert_tame(mm, name)
        sd, r = sr.ref_scalars(m["constant"], dtype)
        assert np.isinf(sd) and r == 0 and np.all(sr.ref_sigmoid(_field("constant", dtype), sd, r) == 1)
    for where in sr.PLACES:
        for swapped in (False, True):
            x = sr.family("extreme_at", NY, NX, seed=7, where=where, swapped=swapped)
            a = sr.place(where, NY, NX)
            assert x[a] == (sr.LO if swapped else sr.HI) and (x.max(), x.min()) == (sr.HI, sr.LO)
    assert sr.place("seg_end", NY, NX) == (37, 127) and sr.place("seg_start", NY, NX) == (37, 128)
    assert sr.place("seg_end", 40, 63) == (20, 62) and sr.place("seg_start", 40, 63) == (21, 0)
    assert sr.place("seg_start", 1, 1) == (0, 0)


def test_ref_scalars_follow_the_working_precision():
    m = sr.ref_moments(_field("plain", np.float32))
    sd, r = sr.ref_scalars(m, np.float32)
    assert sd.dtype == np.float32 and r.dtype == np.float32
    var = np.float32(np.float64(m.M2))
    assert sd == np.float32(2) / np.sqrt(var / np.float32(m.n)) and r == (np.float32(m.mx) - np.float32(m.mn)) / np.float32(4)
    sd8, _ = sr.ref_scalars(m, np.float64)
    assert abs(float(sd) - float(sd8)) <= 4 * 2.0 ** -24 * float(sd8)


# ---------------------------------------------------------------------------------------- the host functions
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", sr.FAMILIES)
def test_host_merges_stay_within_the_bounds(dump, name, scheme, dtype):
    x = _field(name, dtype)
    ref = sr.ref_moments(x)
    res = dump(_cut(x, _schemes(x.size)[scheme]))
    for tag in TAGS:
        sr.assert_moments(res[tag][0], ref, f"{name} {scheme} {tag}")
    if name == "constant":
        assert all(res[tag][0][2] == 0.0 and res[tag][0][1] == 3.25 for tag in TAGS)
    # merging the empty set is the identity, bit for bit, on either side
    assert res["idl"][1] == res["seq"][1] == res["idr"][1]
    assert list(res["empty"][0]) == [0.0, 0.0, 0.0, 1.0e308, -1.0e308]


def test_extremes_in_single_element_and_edge_parts(dump):
    """the placed extremes alone in a part, first, last, and next to an empty part"""
    for where in sr.PLACES:
        for swapped in (False, True):
            x = sr.family("extreme_at", NY, NX, seed=11, where=where, swapped=swapped)
            ref = sr.ref_moments(x)
            a = int(np.ravel_multi_index(sr.place(where, NY, NX), x.shape))
            sizes = ([a] if a else []) + [1, 0]                 # ... | the placed cell | nothing | the rest
            res = dump(_cut(x, sizes))
            for tag in TAGS:
                sr.assert_moments(res[tag][0], ref, f"{where} {swapped} {tag}")


def test_every_part_empty_but_one(dump):
    x = _field("negative", np.float64).ravel()[:5]
    ref = sr.ref_moments(x)
    for pos in (0, 64, 129):
        parts = [np.zeros(0)] * 130
        parts[pos] = x
        res = dump(parts)
        for tag in TAGS:
            sr.assert_moments(res[tag][0], ref, f"alone at {pos} {tag}")
        assert res["seq"][1] == res["wave"][1]                   # (only identities were applied to it)
