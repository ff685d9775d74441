"""The guard's plan (sb_plan_guard, sb_diag_plan.hpp) beside the main launch plan, on the CPU.

sb_set_nonfinite_guard adds launches BETWEEN the steps of the main plan and never changes that plan: with the input on or
off, sb_plan_diag answers the same, step for step.  Where the guard runs, k_guard_bits goes ahead of step 0 and the two
taint passes and the repair behind the CONTRAST step, which is the last but one, ahead of the final WIND; the reach is 16
for k_strip, 31 for k_strip32, 127 for the tables and "by tile" (tile width x rows + LDS halo) for the tile kernel.  Band
phases and calls with gathered moments get no guard launch.  The expectations are written out by hand from the table of
launch sequences in DESIGN.md section 2.3.  tests/plan_dump.cpp is built host-only (tests/plan_dump.py).
"""
import itertools

import pytest

import plan_dump as pd

_line = pd.line


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pd.build(tmp_path_factory)


def _guard(exe, **kw):
    """-> (steps of the main plan, the guard's part) with the guard on"""
    p = pd.parse(pd.run(exe, [_line("x", guard=1, **kw)])[0])[1]
    return pd.names(p.steps), p.guard


FLAGS = ("no_wide", "no_fold", "no_cache", "late", "gathered", "mout", "reuse", "plan_use", "segs_built", "table", "band_table",
         "f2py_table")


def test_main_plan_is_the_one_without_the_input(exe):
    """Every combination of the switches, both flavours, every phase, the three radius classes: the main plan with the guard
    on is, to the letter, the main plan with it off, and with it off the guard's part says so."""
    on, off = [], []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        for t0_fly, phases, (hint, esize) in itertools.product((0, 1), (1, 2, 3), ((6, 8), (24, 4), (24, 8), (31, 8))):
            k = dict(kw, t0_fly=t0_fly, phases=phases, hint=hint, esize=esize)
            lab = str(len(on))
            on.append(_line(lab, guard=1, **k)); off.append(_line(lab, guard=0, **k))
    for w, g in zip(pd.run(exe, off), pd.run(exe, on)):
        (lw, pw), (lg, pg) = pd.parse(w), pd.parse(g)
        assert (lw, pw[:3]) == (lg, pg[:3]), (w, g)
        assert (pw.guard, pw.tail) == (pd.GUARD_OFF, pd.TAIL_OFF) and pg.tail == pd.TAIL_OFF, (w, g)


def test_rows_of_the_design_table(exe):
    """Where the guard's launches go and by how much it dilates, row by row."""
    # single domain, host-model flavour, k_strip, fold on: SCAN, CONTRAST, WIND
    assert _guard(exe) == (["SCAN", "CONTRAST", "WIND"], "guard=1 reach=16 bits_before=0 after=1 nlaunch=4")
    # ... k_strip32 (single precision, radius hint above 16)
    assert _guard(exe, esize=4, hint=24) == (["SCAN", "CONTRAST", "WIND"], "guard=1 reach=31 bits_before=0 after=1 nlaunch=4")
    # fold off: SCAN, PREP, CONTRAST, WIND
    assert _guard(exe, no_fold=1) == (["SCAN", "PREP", "CONTRAST", "WIND"], "guard=1 reach=16 bits_before=0 after=2 nlaunch=4")
    # the tile kernel: fp64 beyond 16 (halo 24: 32 x 32 tiles; halo 32: 32 x 16), sb_set_wide_strip(ctx, 0), a grid the strips cannot hold
    four = ["SCAN", "PREP", "CONTRAST", "WIND"]
    assert _guard(exe, hint=24) == (four, "guard=1 reach=tile:32x32+24 bits_before=0 after=2 nlaunch=4")
    assert _guard(exe, hint=31) == (four, "guard=1 reach=tile:32x16+32 bits_before=0 after=2 nlaunch=4")
    assert _guard(exe, esize=4, hint=24, no_wide=1) == (four, "guard=1 reach=tile:32x32+24 bits_before=0 after=2 nlaunch=4")
    assert _guard(exe, fits=0) == (four, "guard=1 reach=tile:32x32+24 bits_before=0 after=2 nlaunch=4")
    # f2py flavour: SCAN, PREP, T0, CONTRAST, WIND
    five = ["SCAN", "PREP", "T0", "CONTRAST", "WIND"]
    assert _guard(exe, t0_fly=0) == (five, "guard=1 reach=16 bits_before=0 after=3 nlaunch=4")
    assert _guard(exe, t0_fly=0, esize=4, hint=31) == (five, "guard=1 reach=31 bits_before=0 after=3 nlaunch=4")
    assert _guard(exe, t0_fly=0, hint=31) == (five, "guard=1 reach=tile:32x16+32 bits_before=0 after=3 nlaunch=4")
    # the tables, host-model and f2py flavour, whatever kernel the domain would otherwise get
    six = ["SCAN", "PREP", "TABLE_ROWS", "TABLE_COLS", "CONTRAST", "WIND"]
    for hint, esize in ((6, 8), (24, 4), (31, 8)):
        assert _guard(exe, table=1, hint=hint, esize=esize) == (six, "guard=1 reach=127 bits_before=0 after=4 nlaunch=4")
        assert _guard(exe, table=1, f2py_table=1, t0_fly=0, hint=hint, esize=esize) == \
            (six, "guard=1 reach=127 bits_before=0 after=4 nlaunch=4")
    # `table` alone does not serve the f2py flavour: its five steps, its own kernel's reach
    assert _guard(exe, table=1, t0_fly=0) == (five, "guard=1 reach=16 bits_before=0 after=3 nlaunch=4")


def test_band_phases_and_gathered_moments_get_none(exe):
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
    for g in pd.run(exe, lines):
        assert pd.parse(g)[1].guard == "guard=0 nlaunch=0", g


def test_every_whole_call_without_gathered_moments_gets_it(exe):
    """... and the CONTRAST step it follows is the last but one, ahead of a final WIND."""
    lines = []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        if kw["gathered"]:
            continue
        for t0_fly, (hint, esize) in itertools.product((0, 1), ((6, 8), (24, 4), (24, 8), (31, 8))):
            lines.append(_line(str(len(lines)), guard=1, **dict(kw, t0_fly=t0_fly, hint=hint, esize=esize)))
    for g in pd.run(exe, lines):
        parts = [s.strip() for s in g.split("|")]
        steps = parts[2].split()
        assert parts[4].startswith("guard=1 ") and parts[4].endswith("nlaunch=4"), g
        after = int(parts[4].split("after=")[1].split()[0])
        assert after == len(steps) - 2 and steps[after].startswith("CONTRAST:") and ",update" not in steps[after], g
        assert steps[-1].startswith("WIND:") and ",final" in steps[-1], g
        assert len(steps) <= 7 and parts[3].endswith("max=7"), g
