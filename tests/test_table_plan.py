"""The launch plan with the table switch (SbPlanIn::table, sb_set_table_contrast): a whole single-domain call of the host-model
flavour becomes SCAN, PREP, TABLE_ROWS, TABLE_COLS, CONTRAST (the table query), WIND -- six launches, the two table passes
not fused; every other call keeps the sequence it has without the switch.

tests/plan_dump.cpp is built host-only (tests/plan_dump.py); `table` is 1 here unless a case says otherwise.  The
expectations are written out by hand from the table of launch sequences in DESIGN.md section 2.3.  The boundary mode is
not the planner's business: the caller sets `table` for SB_BND_GLOBAL and SB_BND_HALO alike (the GPU tests run both), and
the plan of a table call does not depend on the contrast kernel the domain would otherwise get -- the cases run every
radius hint and both precisions.
"""
import itertools

import pytest

import plan_dump as pd


def _line(label, **kw):
    return pd.line(label, **dict(dict(table=1), **kw))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = pd.build(tmp_path_factory)
    return lambda lines: pd.plans(exe, lines)       # -> {label: (contrast, [steps], kept, guard, guard tail)}


TABLE_STEPS = ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final",
               "TABLE_ROWS:prof=t0,stats=none*0,final", "TABLE_COLS:prof=thc,stats=none*0,final",
               "CONTRAST:prof=thc,stats=none*0,final,table", "WIND:prof=wind,stats=none*0,final"]
TABLE_KEPT = "segs_built=0 wind_scratch=0 scan_wgs=12 table=1 nsteps=6 max=7"


def test_whole_host_model_call_takes_the_tables(dump):
    """Whatever the radius hint, the precision and the knobs of the strip kernels: the six steps, k_prep's lists rebuilt every
    call (no stored plan is trusted), nothing kept for the strip kernel's sake."""
    cases = {}
    for esize, hint in itertools.product((8, 4), (6, 16, 24, 31)):
        cases[f"plain/{esize}/{hint}"] = dict(esize=esize, hint=hint)
    cases["knobs"] = dict(no_wide=1, no_fold=1, no_cache=1, late=1)
    cases["stored_plan"] = dict(plan_use=1, segs_built=1)
    cases["nofit"] = dict(fits=0)
    got = dump([_line(k, **kw) for k, kw in cases.items()])
    for k in cases:
        assert got[k][1] == TABLE_STEPS and got[k][2] == TABLE_KEPT, (k, got[k])
    # static sigma: the scalars of an earlier call stand, k_scan forms no moments and k_prep merges none
    got = dump([_line("reuse", reuse=1)])
    assert got["reuse"][1] == ["SCAN:prof=scan,stats=none*0,final", "PREP:prof=prep,stats=none*0,final"] + TABLE_STEPS[2:]


def test_switch_is_ignored_where_it_does_not_apply(dump):
    """The f2py flavour, a band step (both phases, both orders) and gathered moments: the sequence of today, step for step."""
    flags = ("no_wide", "no_fold", "no_cache", "late", "mout", "reuse", "plan_use", "segs_built")
    lines = []
    for bits in itertools.product((0, 1), repeat=len(flags)):
        kw = dict(zip(flags, bits))
        for name, sel in (("f2py", dict(t0_fly=0)), ("ph1", dict(phases=1, gathered=1)), ("ph2", dict(phases=2, gathered=1)),
                          ("ph1_alone", dict(phases=1)), ("ph2_alone", dict(phases=2)),
                          ("gathered", dict(gathered=1)), ("gathered_f2py", dict(gathered=1, t0_fly=0))):
            for hint, esize in ((6, 8), (24, 4)):
                for table in (0, 1):
                    lines.append(_line(f"{name}/{len(lines)}/{table}", hint=hint, esize=esize, table=table, **sel, **kw))
    got = dump(lines)
    labels = list(got)
    assert len(labels) == 256 * 7 * 2 * 2
    for off, on in zip(labels[0::2], labels[1::2]):
        assert off.endswith("/0") and on.endswith("/1")
        assert got[on] == got[off], (on, got[on], got[off])
        assert " table=0 " in got[on][2] and not any("TABLE" in s or s.endswith(",table") for s in got[on][1])


def test_named_sequences_with_the_switch_set(dump):
    """... and by name, as tests/test_diag_plan.py writes them out."""
    want = {
        "f2py": (dict(t0_fly=0), ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final",
                                  "T0:prof=t0,stats=none*0,final", "CONTRAST:prof=thc,stats=none*0,final",
                                  "WIND:prof=wind,stats=none*0,final"]),
        "band_ph1": (dict(phases=1, gathered=1, mout=1),
                     ["SCAN:prof=scan,stats=partials*0,publish", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0"]),
        "band_ph2": (dict(phases=2, gathered=1), ["CONTRAST:prof=thc,stats=gathered*0,fold,final,update"]),
        "gathered": (dict(gathered=1), ["SCAN:prof=scan,stats=none*0", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0",
                                        "CONTRAST:prof=thc,stats=gathered*0,fold,final,update"]),
    }
    got = dump([_line(k, **kw) for k, (kw, _) in want.items()])
    for k, (_, steps) in want.items():
        assert got[k][1] == steps, (k, got[k])


def test_switch_off_is_the_plan_of_today(dump):
    """table = 0 on a whole host-model call: the three launches of the strip kernel with the fold."""
    got = dump([_line("off", table=0)])
    assert got["off"][1] == ["SCAN:prof=scan,stats=partials*0,final", "CONTRAST:prof=thc,stats=partials*12,fold,final",
                             "WIND:prof=wind,stats=none*0,final"]
    assert got["off"][2] == "segs_built=1 wind_scratch=0 scan_wgs=12 table=0 nsteps=3 max=7"
