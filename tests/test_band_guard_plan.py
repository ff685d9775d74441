"""The guard's plan with sb_set_nonfinite_guard_bands beside it (sb_plan_guard, sb_diag_plan.hpp), on the CPU.

The switch adds two cases to the one tests/test_guard_plan.py holds.  Where the CONTRAST step applies the update itself --
phase 2 of a band step, a one-sequence call with gathered moments -- k_guard_bits and both taint passes go directly ahead
of that step (for the tables between TABLE_COLS and the query) and the repair directly behind it, with `update` set; a call
with gathered moments in the single-domain order (sb_set_band_order: CONTRAST, then a final WIND) runs as a whole call
does.  Phase 1 and the f2py flavour get nothing.  The main plan never changes, and with the new input off nothing runs
ahead of the CONTRAST step.  The expectations are written out by hand from the table of launch sequences in
DESIGN.md section 2.3.  tests/plan_dump.cpp is built host-only (tests/plan_dump.py).
"""
import itertools

import pytest

import plan_dump as pd

# the combinations tests/test_guard_plan.py sweeps
FLAGS = ("no_wide", "no_fold", "no_cache", "late", "gathered", "mout", "reuse", "plan_use", "segs_built", "table", "band_table",
         "f2py_table")
CLASSES = ((6, 8), (24, 4), (24, 8), (31, 8))


def _line(label, guard, bands, **kw):
    return pd.line(label, guard=guard, guard_bands=bands, **kw)


def _run(exe, lines):
    out = pd.run(exe, lines)
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pd.build(tmp_path_factory)


def _sweep():
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        for t0_fly, phases, (hint, esize) in itertools.product((0, 1), (1, 2, 3), CLASSES):
            yield dict(kw, t0_fly=t0_fly, phases=phases, hint=hint, esize=esize)


def _both(exe, **kw):
    """-> (steps of the main plan, the guard's part, the new fields) with both switches on"""
    p = pd.parse(_run(exe, [_line("x", 1, 1, **kw)])[0])[1]
    return pd.names(p.steps), p.guard, p.tail


def test_main_plan_is_the_one_without_the_inputs(exe):
    """sb_plan_diag reads neither switch: over every combination, with the two inputs in every state, the main plan is to the
    letter the one with both off."""
    cases = list(_sweep())
    want = _run(exe, [_line(str(i), 0, 0, **k) for i, k in enumerate(cases)])
    for guard, bands in ((0, 1), (1, 0), (1, 1)):
        got = _run(exe, [_line(str(i), guard, bands, **k) for i, k in enumerate(cases)])
        for w, g in zip(want, got):
            assert g.rsplit("|", 2)[0].rstrip() == w.rsplit("|", 2)[0].rstrip(), (w, g)
    for w in want:
        assert w.split("|", 4)[4].strip() == "guard=0 nlaunch=0 | taint_before=-1 update=0", w


def test_new_input_off_is_the_guard_plan_as_it_was(exe):
    """guard_bands = 0: nothing runs ahead of CONTRAST; the new switch alone (the old one off) gives no guard at all."""
    cases = list(_sweep())
    for guard in (0, 1):
        for g in _run(exe, [_line(str(i), guard, 0, **k) for i, k in enumerate(cases)]):
            assert g.rsplit("|", 1)[1].strip() == "taint_before=-1 update=0", g
    for g in _run(exe, [_line(str(i), 0, 1, **k) for i, k in enumerate(cases)]):
        assert g.split("|", 4)[4].strip() == "guard=0 nlaunch=0 | taint_before=-1 update=0", g


def test_whole_calls_do_not_depend_on_the_new_input(exe):
    cases = [k for k in _sweep() if k["phases"] == 3 and not k["gathered"]]
    a = _run(exe, [_line(str(i), 1, 0, **k) for i, k in enumerate(cases)])
    b = _run(exe, [_line(str(i), 1, 1, **k) for i, k in enumerate(cases)])
    assert a == b


def test_rows_of_the_design_table_phase_two(exe):
    """phase 2 of a band step: everything but the repair directly ahead of the CONTRAST step, the repair behind it, with the update"""
    ph2 = dict(phases=2, gathered=1)
    one = ["CONTRAST"]
    ahead = "taint_before=0 update=1"
    # k_strip (fold on and off: the step is the same), k_strip32, the tile kernel (fp64 beyond 16; sb_set_wide_strip(ctx, 0))
    assert _both(exe, **ph2) == (one, "guard=1 reach=16 bits_before=0 after=0 nlaunch=4", ahead)
    assert _both(exe, no_fold=1, **ph2) == (one, "guard=1 reach=16 bits_before=0 after=0 nlaunch=4", ahead)
    assert _both(exe, esize=4, hint=24, **ph2) == (one, "guard=1 reach=31 bits_before=0 after=0 nlaunch=4", ahead)
    assert _both(exe, hint=24, **ph2) == (one, "guard=1 reach=tile:32x32+24 bits_before=0 after=0 nlaunch=4", ahead)
    assert _both(exe, hint=31, **ph2) == (one, "guard=1 reach=tile:32x16+32 bits_before=0 after=0 nlaunch=4", ahead)
    assert _both(exe, esize=4, hint=24, no_wide=1, **ph2) == (one, "guard=1 reach=tile:32x32+24 bits_before=0 after=0 nlaunch=4", ahead)
    # the tables: MERGE, TABLE_ROWS, TABLE_COLS, then the query -- between the column pass and the query
    four = ["MERGE", "TABLE_ROWS", "TABLE_COLS", "CONTRAST"]
    for hint, esize in ((6, 8), (24, 4), (31, 8)):
        assert _both(exe, table=1, band_table=1, hint=hint, esize=esize, **ph2) == \
            (four, "guard=1 reach=127 bits_before=3 after=3 nlaunch=4", "taint_before=3 update=1")
    # static sigma: no MERGE
    assert _both(exe, table=1, band_table=1, reuse=1, **ph2) == \
        (four[1:], "guard=1 reach=127 bits_before=2 after=2 nlaunch=4", "taint_before=2 update=1")
    # a band step in the single-domain order: CONTRAST, WIND -- as a whole call, CONTRAST being step 0
    assert _both(exe, late=1, **ph2) == (["CONTRAST", "WIND"], "guard=1 reach=16 bits_before=0 after=0 nlaunch=4", "taint_before=-1 update=0")


def test_rows_of_the_design_table_gathered_moments(exe):
    """a one-sequence call with gathered moments, both band orders"""
    g = dict(phases=3, gathered=1)
    seq = ["SCAN", "PREP", "WIND", "CONTRAST"]
    # order 0: SCAN, PREP, WIND to the scratch planes, CONTRAST with the update
    assert _both(exe, **g) == (seq, "guard=1 reach=16 bits_before=3 after=3 nlaunch=4", "taint_before=3 update=1")
    assert _both(exe, esize=4, hint=24, **g) == (seq, "guard=1 reach=31 bits_before=3 after=3 nlaunch=4", "taint_before=3 update=1")
    assert _both(exe, hint=24, **g) == (seq, "guard=1 reach=tile:32x32+24 bits_before=3 after=3 nlaunch=4", "taint_before=3 update=1")
    # ... the stored plan trusted: no PREP
    assert _both(exe, plan_use=1, segs_built=1, **g) == \
        (["SCAN", "WIND", "CONTRAST"], "guard=1 reach=16 bits_before=2 after=2 nlaunch=4", "taint_before=2 update=1")
    # ... the tables: seven steps
    seven = ["SCAN", "PREP", "WIND", "MERGE", "TABLE_ROWS", "TABLE_COLS", "CONTRAST"]
    assert _both(exe, table=1, band_table=1, **g) == (seven, "guard=1 reach=127 bits_before=6 after=6 nlaunch=4", "taint_before=6 update=1")
    # order 1 (sb_set_band_order): SCAN, CONTRAST, a final WIND -- exactly as a whole call: bits ahead of step 0, taint and
    # repair between CONTRAST and WIND, no update
    late = ["SCAN", "CONTRAST", "WIND"]
    assert _both(exe, late=1, **g) == (late, "guard=1 reach=16 bits_before=0 after=1 nlaunch=4", "taint_before=-1 update=0")
    assert _both(exe, late=1, esize=4, hint=24, **g) == (late, "guard=1 reach=31 bits_before=0 after=1 nlaunch=4", "taint_before=-1 update=0")
    # ... which only a folding strip kernel takes: the tile kernel, fold off and the tables stay in order 0
    assert _both(exe, late=1, hint=24, **g) == (seq, "guard=1 reach=tile:32x32+24 bits_before=3 after=3 nlaunch=4", "taint_before=3 update=1")
    assert _both(exe, late=1, no_fold=1, **g) == (seq, "guard=1 reach=16 bits_before=3 after=3 nlaunch=4", "taint_before=3 update=1")
    assert _both(exe, late=1, table=1, band_table=1, **g) == (seven, "guard=1 reach=127 bits_before=6 after=6 nlaunch=4", "taint_before=6 update=1")


def test_phase_one_and_the_f2py_flavour_get_none(exe):
    none = "guard=0 nlaunch=0 | taint_before=-1 update=0"
    lines = [_line(str(i), 1, 1, **k) for i, k in enumerate(_sweep())
             if k["phases"] == 1 or (not k["t0_fly"] and (k["phases"] == 2 or k["gathered"]))]
    assert len(lines) > 1000
    for g in _run(exe, lines):
        assert g.split("|", 4)[4].strip() == none, g


def test_every_served_call_has_its_launches_round_the_contrast_step(exe):
    """host-model flavour, phase 2 or gathered moments, both switches on: always served; the positions follow from whether a
    final WIND stands behind the CONTRAST step"""
    cases = [k for k in _sweep() if k["t0_fly"] and (k["phases"] == 2 or (k["phases"] == 3 and k["gathered"]))]
    for g in _run(exe, [_line(str(i), 1, 1, **k) for i, k in enumerate(cases)]):
        parts = [s.strip() for s in g.split("|")]
        steps = parts[2].split()
        assert parts[4].startswith("guard=1 ") and parts[4].endswith("nlaunch=4"), g
        f = dict(kv.split("=") for kv in (parts[4] + " " + parts[5]).split() if "=" in kv)
        bits, after, taint, update = int(f["bits_before"]), int(f["after"]), int(f["taint_before"]), int(f["update"])
        assert steps[after].startswith("CONTRAST:"), g
        if steps[-1].startswith("WIND:") and after == len(steps) - 2:
            assert ",final" in steps[-1] and ",update" not in steps[after] and (bits, taint, update) == (0, -1, 0), g
        else:
            assert after == len(steps) - 1 and (bits, taint, update) == (after, after, 1), g
            assert ",update" in steps[after] or "wind_scratch=1" in parts[3], g
        assert len(steps) <= 7 and "max=7" in parts[3], g
