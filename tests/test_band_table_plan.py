"""The launch plan with the band switch of the table contrast (SbPlanIn::band_table, sb_set_table_contrast_bands beside
sb_set_table_contrast): a band step of the host-model flavour becomes SCAN, PREP, WIND | join | MERGE, TABLE_ROWS, TABLE_COLS,
CONTRAST (the table query, which applies the update); a whole call with gathered moments the same seven steps in one sequence.
Every other call -- and every call while `table` is off -- keeps the sequence it has without the switch.

tests/plan_dump.cpp is built host-only (tests/plan_dump.py); `gathered`, `table` and `band_table` are 1 here unless a case
says otherwise.  The expectations are written out by hand from the table of launch sequences in DESIGN.md section 2.3.
"""
import itertools

import pytest

import plan_dump as pd


def _line(label, **kw):
    return pd.line(label, **dict(dict(gathered=1, table=1, band_table=1), **kw))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = pd.build(tmp_path_factory)
    return lambda lines: pd.plans(exe, lines)       # -> {label: (contrast, [steps], kept, guard, guard tail)}


# phase 1 of a band step (k_scan publishes the band's moments), phase 2, and the gathered call: no step is `final` -- k_wind
# leaves its winds in the scratch planes and the query applies them
PH1 = ["SCAN:prof=scan,stats=partials*0,publish", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0"]
PH1_REUSE = ["SCAN:prof=scan,stats=none*0", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0"]
MERGE = ["MERGE:prof=none,stats=gathered*0"]
TABLES = ["TABLE_ROWS:prof=t0,stats=none*0", "TABLE_COLS:prof=thc,stats=none*0", "CONTRAST:prof=thc,stats=none*0,table"]
KEPT = lambda nsteps: pd.kept(0, 1, 1, nsteps)      # segs_built=0 wind_scratch=1 scan_wgs=12 table=1, and the step count

GRID = list(itertools.product((8, 4), (6, 24, 31)))         # both precisions, the strip kernels' and the tile kernel's radius hints


def test_band_step_phases(dump):
    """Phase 1 ahead of the join, phase 2 behind it, with and without the scalars of an earlier call."""
    want, lines = {}, []
    for esize, hint in GRID:
        for reuse in (0, 1):
            k = f"{esize}/{hint}/{reuse}"
            lines.append(_line("ph1/" + k, phases=1, mout=0 if reuse else 1, reuse=reuse, esize=esize, hint=hint))
            want["ph1/" + k] = PH1_REUSE if reuse else PH1
            lines.append(_line("ph2/" + k, phases=2, reuse=reuse, esize=esize, hint=hint))
            want["ph2/" + k] = TABLES if reuse else MERGE + TABLES
    got = dump(lines)
    for k, steps in want.items():
        assert got[k][1] == steps and got[k][2] == KEPT(len(steps)), (k, got[k])


def test_whole_call_with_gathered_moments(dump):
    """The torch transport: the same steps in one sequence; k_scan forms no statistics (they came gathered)."""
    want, lines = {}, []
    for esize, hint in GRID:
        for reuse in (0, 1):
            k = f"{esize}/{hint}/{reuse}"
            lines.append(_line(k, reuse=reuse, esize=esize, hint=hint))
            want[k] = PH1_REUSE + ([] if reuse else MERGE) + TABLES
    got = dump(lines)
    for k, steps in want.items():
        assert got[k][1] == steps and got[k][2] == KEPT(len(steps)), (k, got[k])
    assert len(want["8/6/0"]) == 7


def test_knobs_of_the_other_kernels_do_not_matter(dump):
    """sb_set_band_order, the fold, the plan cache, the wide strip, a stored plan, a grid the strip kernels cannot hold:
    k_prep runs every call, k_wind never trusts the lists of the call before, the order is never the single domain's."""
    cases = {"knobs": dict(no_wide=1, no_fold=1, no_cache=1), "late": dict(late=1), "late32": dict(late=1, esize=4, hint=24),
             "stored_plan": dict(plan_use=1, segs_built=1), "nofit": dict(fits=0)}
    lines = []
    for k, kw in cases.items():
        lines += [_line(k + "/ph1", phases=1, mout=1, **kw), _line(k + "/ph2", phases=2, **kw), _line(k + "/whole", **kw)]
    got = dump(lines)
    for k in cases:
        assert got[k + "/ph1"][1] == PH1 and got[k + "/ph2"][1] == MERGE + TABLES, (k, got[k + "/ph1"], got[k + "/ph2"])
        assert got[k + "/whole"][1] == PH1_REUSE + MERGE + TABLES, (k, got[k + "/whole"])
        assert all(got[f"{k}/{p}"][2] == KEPT(n) for p, n in (("ph1", 3), ("ph2", 4), ("whole", 7))), k


FLAGS = ("no_wide", "no_fold", "no_cache", "late", "mout", "reuse", "plan_use", "segs_built")


def _pairs(dump, sels, fixed_on, fixed_off):
    """every combination of FLAGS x sels x (hint, esize): the plan with `fixed_on` against the plan with `fixed_off`"""
    lines = []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        for name, sel in sels:
            for hint, esize in ((6, 8), (24, 4), (31, 8)):
                for tag, fx in (("0", fixed_off), ("1", fixed_on)):
                    lines.append(_line(f"{name}/{len(lines)}/{tag}", **dict(dict(hint=hint, esize=esize, **sel, **kw), **fx)))
    got = dump(lines)
    labels = list(got)
    assert len(labels) == 256 * len(sels) * 3 * 2
    return got, list(zip(labels[0::2], labels[1::2]))


def test_switch_is_ignored_where_it_does_not_apply(dump):
    """A whole call without gathered moments (it has the table switch proper) and the f2py flavour, as a whole call, as
    band phases and with gathered moments: the plan with band_table = 0, step for step."""
    sels = (("whole", dict(gathered=0)), ("f2py", dict(gathered=0, t0_fly=0)), ("f2py_gathered", dict(t0_fly=0)),
            ("f2py_ph1", dict(phases=1, t0_fly=0)), ("f2py_ph2", dict(phases=2, t0_fly=0)))
    for table in (0, 1):
        got, pairs = _pairs(dump, sels, dict(band_table=1, table=table), dict(band_table=0, table=table))
        for off, on in pairs:
            assert off.endswith("/0") and on.endswith("/1")
            assert got[on] == got[off], (on, got[on], got[off])


def test_nothing_changes_while_the_table_switch_is_off(dump):
    """band_table = 1 with table = 0: every kind of call keeps today's plan, no table step anywhere."""
    sels = (("whole", dict(gathered=0)), ("ph1", dict(phases=1)), ("ph2", dict(phases=2)), ("gathered", dict()),
            ("ph1_alone", dict(phases=1, gathered=0)), ("ph2_alone", dict(phases=2, gathered=0)), ("f2py", dict(gathered=0, t0_fly=0)))
    got, pairs = _pairs(dump, sels, dict(band_table=1, table=0), dict(band_table=0, table=0))
    for off, on in pairs:
        assert got[on] == got[off], (on, got[on], got[off])
        assert " table=0 " in got[on][2] and not any("TABLE" in s or s.endswith(",table") for s in got[on][1])


def test_switch_off_is_the_plan_of_today(dump):
    """band_table = 0 with table = 1 on a band step and on a gathered call: the sequences tests/test_table_plan.py names."""
    want = {
        "band_ph1": (dict(phases=1, mout=1), PH1),
        "band_ph2": (dict(phases=2), ["CONTRAST:prof=thc,stats=gathered*0,fold,final,update"]),
        "gathered": (dict(), PH1_REUSE + ["CONTRAST:prof=thc,stats=gathered*0,fold,final,update"]),
    }
    got = dump([_line(k, band_table=0, **kw) for k, (kw, _) in want.items()])
    for k, (_, steps) in want.items():
        assert got[k][1] == steps and " table=0 " in got[k][2], (k, got[k])
