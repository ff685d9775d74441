"""The guard's plan (sb_plan_guard, sb_diag_plan.hpp) beside the main launch plan, on the CPU.

sb_set_nonfinite_guard adds launches BETWEEN the steps of the main plan and never changes that plan: with the input on or
off, sb_plan_diag answers step for step what tests/f2py_table_plan_dump.cpp -- which does not know the input -- prints for
the same call.  Where the guard runs, k_guard_bits goes ahead of step 0 and the two taint passes and the repair behind the
CONTRAST step, which is the last but one, ahead of the final WIND; the reach is 16 for k_strip, 31 for k_strip32, 127 for
the tables and "by tile" (tile width x rows + LDS halo) for the tile kernel.  Band phases and calls with gathered moments
get no guard launch.  The expectations are written out by hand from the table of launch sequences in DESIGN.md section 2.3.
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("phases", "esize", "t0_fly", "hint", "no_wide", "no_fold", "no_cache", "late", "gathered", "mout", "reuse",
          "plan_use", "segs_built", "wgs", "fits", "table", "band_table", "f2py_table")
DEFAULT = dict(phases=3, esize=8, t0_fly=1, hint=6, no_wide=0, no_fold=0, no_cache=0, late=0, gathered=0, mout=0, reuse=0,
               plan_use=0, segs_built=0, wgs=12, fits=1, table=0, band_table=0, f2py_table=0)


def _line(label, guard=None, **kw):
    c = dict(DEFAULT, **kw)
    return "plan " + label + " " + " ".join(str(c[f]) for f in FIELDS) + ("" if guard is None else f" {guard}")


def _build(tmp, name):
    cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip(f"no hipcc to build tests/{name}.cpp with")
    out = str(tmp / name)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-x", "c++", os.path.join(ROOT, "tests", name + ".cpp"), "-o", out], check=True)
    return out


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("guard_plan")
    return _build(tmp, "guard_plan_dump"), _build(tmp, "f2py_table_plan_dump")


def _guard(exes, **kw):
    """-> (steps of the main plan, the guard's part) with the guard on"""
    ln = _run(exes[0], [_line("x", guard=1, **kw)])[0]
    parts = [s.strip() for s in ln.split("|")]
    return [s.split(":")[0] for s in parts[2].split()], parts[4]


FLAGS = ("no_wide", "no_fold", "no_cache", "late", "gathered", "mout", "reuse", "plan_use", "segs_built", "table", "band_table",
         "f2py_table")


def test_main_plan_is_the_one_without_the_input(exes):
    """Every combination of the switches, both flavours, every phase, the three radius classes: the main plan with the guard
    on and off is, to the letter, what the dump that does not know the input prints."""
    base, on, off = [], [], []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        for t0_fly, phases, (hint, esize) in itertools.product((0, 1), (1, 2, 3), ((6, 8), (24, 4), (24, 8), (31, 8))):
            k = dict(kw, t0_fly=t0_fly, phases=phases, hint=hint, esize=esize)
            lab = str(len(base))
            base.append(_line(lab, **k)); on.append(_line(lab, guard=1, **k)); off.append(_line(lab, guard=0, **k))
    want = _run(exes[1], base)
    for got in (_run(exes[0], on), _run(exes[0], off)):
        for w, g in zip(want, got):
            assert g.rsplit("|", 1)[0].rstrip() == w.rstrip(), (w, g)
    for g in _run(exes[0], off):
        assert g.rsplit("|", 1)[1].strip() == "guard=0 nlaunch=0", g


def test_rows_of_the_design_table(exes):
    """Where the guard's launches go and by how much it dilates, row by row."""
    # single domain, host-model flavour, k_strip, fold on: SCAN, CONTRAST, WIND
    assert _guard(exes) == (["SCAN", "CONTRAST", "WIND"], "guard=1 reach=16 bits_before=0 after=1 nlaunch=4")
    # ... k_strip32 (single precision, radius hint above 16)
    assert _guard(exes, esize=4, hint=24) == (["SCAN", "CONTRAST", "WIND"], "guard=1 reach=31 bits_before=0 after=1 nlaunch=4")
    # fold off: SCAN, PREP, CONTRAST, WIND
    assert _guard(exes, no_fold=1) == (["SCAN", "PREP", "CONTRAST", "WIND"], "guard=1 reach=16 bits_before=0 after=2 nlaunch=4")
    # the tile kernel: fp64 beyond 16 (halo 24: 32 x 32 tiles; halo 32: 32 x 16), sb_set_wide_strip(ctx, 0), a grid the strips cannot hold
    four = ["SCAN", "PREP", "CONTRAST", "WIND"]
    assert _guard(exes, hint=24) == (four, "guard=1 reach=tile:32x32+24 bits_before=0 after=2 nlaunch=4")
    assert _guard(exes, hint=31) == (four, "guard=1 reach=tile:32x16+32 bits_before=0 after=2 nlaunch=4")
    assert _guard(exes, esize=4, hint=24, no_wide=1) == (four, "guard=1 reach=tile:32x32+24 bits_before=0 after=2 nlaunch=4")
    assert _guard(exes, fits=0) == (four, "guard=1 reach=tile:32x32+24 bits_before=0 after=2 nlaunch=4")
    # f2py flavour: SCAN, PREP, T0, CONTRAST, WIND
    five = ["SCAN", "PREP", "T0", "CONTRAST", "WIND"]
    assert _guard(exes, t0_fly=0) == (five, "guard=1 reach=16 bits_before=0 after=3 nlaunch=4")
    assert _guard(exes, t0_fly=0, esize=4, hint=31) == (five, "guard=1 reach=31 bits_before=0 after=3 nlaunch=4")
    assert _guard(exes, t0_fly=0, hint=31) == (five, "guard=1 reach=tile:32x16+32 bits_before=0 after=3 nlaunch=4")
    # the tables, host-model and f2py flavour, whatever kernel the domain would otherwise get
    six = ["SCAN", "PREP", "TABLE_ROWS", "TABLE_COLS", "CONTRAST", "WIND"]
    for hint, esize in ((6, 8), (24, 4), (31, 8)):
        assert _guard(exes, table=1, hint=hint, esize=esize) == (six, "guard=1 reach=127 bits_before=0 after=4 nlaunch=4")
        assert _guard(exes, table=1, f2py_table=1, t0_fly=0, hint=hint, esize=esize) == \
            (six, "guard=1 reach=127 bits_before=0 after=4 nlaunch=4")
    # `table` alone does not serve the f2py flavour: its five steps, its own kernel's reach
    assert _guard(exes, table=1, t0_fly=0) == (five, "guard=1 reach=16 bits_before=0 after=3 nlaunch=4")


def test_band_phases_and_gathered_moments_get_none(exes):
    """The contrast kernel applies the update itself there (or thc is consumed in the same launch): exactly what runs without
    the switch, over every combination of the other switches."""
    lines = []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        for t0_fly, (hint, esize) in itertools.product((0, 1), ((6, 8), (24, 4), (31, 8))):
            for phases in (1, 2, 3):
                if phases == 3 and not kw["gathered"]:
                    continue
                lines.append(_line(str(len(lines)), guard=1, **dict(kw, t0_fly=t0_fly, phases=phases, hint=hint, esize=esize)))
    for g in _run(exes[0], lines):
        assert g.rsplit("|", 1)[1].strip() == "guard=0 nlaunch=0", g


def test_every_whole_call_without_gathered_moments_gets_it(exes):
    """... and the CONTRAST step it follows is the last but one, ahead of a final WIND."""
    lines = []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        if kw["gathered"]:
            continue
        for t0_fly, (hint, esize) in itertools.product((0, 1), ((6, 8), (24, 4), (24, 8), (31, 8))):
            lines.append(_line(str(len(lines)), guard=1, **dict(kw, t0_fly=t0_fly, hint=hint, esize=esize)))
    for g in _run(exes[0], lines):
        parts = [s.strip() for s in g.split("|")]
        steps = parts[2].split()
        assert parts[4].startswith("guard=1 ") and parts[4].endswith("nlaunch=4"), g
        after = int(parts[4].split("after=")[1].split()[0])
        assert after == len(steps) - 2 and steps[after].startswith("CONTRAST:") and ",update" not in steps[after], g
        assert steps[-1].startswith("WIND:") and ",final" in steps[-1], g
        assert len(steps) <= 7 and parts[3].endswith("max=7"), g
