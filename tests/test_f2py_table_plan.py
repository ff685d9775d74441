"""The launch plan with the f2py switch of the table contrast (SbPlanIn::f2py_table, sb_set_table_contrast_f2py beside
sb_set_table_contrast): a whole call of the f2py flavour becomes SCAN, PREP, TABLE_ROWS (timed in k_t0's pair: the row pass
writes the t0 plane), TABLE_COLS, CONTRAST (the table query), WIND -- six launches where the flavour runs five, no k_t0.
Every other call -- the host-model flavour, band phases, gathered moments, and every call while `table` is off -- keeps the
plan it has without the input.

tests/plan_dump.cpp is built host-only (tests/plan_dump.py); here `t0_fly` is 0, `table` and `f2py_table` are 1 unless a case
says otherwise.  The program also drives the host's half of the window cache (sb_table_cache.hpp) for the keys of wrapper
calls.  The expectations are written out by hand from the table of launch sequences in DESIGN.md section 2.3.
"""
import itertools

import pytest

import plan_dump as pd
from plan_dump import BND_GLOBAL, BND_WRAPPER


def _line(label, **kw):
    return pd.line(label, **dict(dict(t0_fly=0, table=1, f2py_table=1), **kw))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pd.build(tmp_path_factory)


@pytest.fixture(scope="module")
def dump(exe):
    return lambda lines: pd.plans(exe, lines)       # -> {label: (contrast, [steps], kept, guard, guard tail)}


SIX = ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final", "TABLE_ROWS:prof=t0,stats=none*0,final",
       "TABLE_COLS:prof=thc,stats=none*0,final", "CONTRAST:prof=thc,stats=none*0,final,table", "WIND:prof=wind,stats=none*0,final"]
SIX_REUSE = ["SCAN:prof=scan,stats=none*0,final", "PREP:prof=prep,stats=none*0,final"] + SIX[2:]
KEPT = "segs_built=0 wind_scratch=0 scan_wgs=12 table=1 nsteps=6 max=7"
GRID = list(itertools.product((8, 4), (6, 24, 31)))         # both precisions, the strip kernels' and the tile kernel's radius hints


def test_six_steps_no_k_t0(dump):
    """The sequence of the issue, whatever the precision and the radius hint; with standing scalars k_scan and k_prep form none."""
    lines, want = [], {}
    for esize, hint in GRID:
        for reuse in (0, 1):
            k = f"{esize}/{hint}/{reuse}"
            lines.append(_line(k, esize=esize, hint=hint, reuse=reuse))
            want[k] = SIX_REUSE if reuse else SIX
    got = dump(lines)
    for k, steps in want.items():
        assert got[k][1] == steps and got[k][2] == KEPT, (k, got[k])
        assert not any(s.startswith("T0:") for s in got[k][1])
    assert len(SIX) == 6


def test_the_other_kernels_knobs_do_not_matter(dump):
    cases = {"knobs": dict(no_wide=1, no_fold=1, no_cache=1), "late": dict(late=1), "stored_plan": dict(plan_use=1, segs_built=1),
             "nofit": dict(fits=0), "band_switch": dict(band_table=1)}
    got = dump([_line(k, **kw) for k, kw in cases.items()])
    for k in cases:
        assert got[k][1] == SIX and got[k][2] == KEPT, (k, got[k])


def test_without_the_input_the_flavour_keeps_its_five(dump):
    """`table` alone (sb_set_table_contrast, with or without the band switch) never changes an f2py-flavour call."""
    five = ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final", "T0:prof=t0,stats=none*0,final",
            "CONTRAST:prof=thc,stats=none*0,final", "WIND:prof=wind,stats=none*0,final"]
    got = dump([_line(f"{t}{b}", f2py_table=0, table=t, band_table=b) for t in (0, 1) for b in (0, 1)])
    for k, g in got.items():
        assert g[1] == five and g[2] == "segs_built=0 wind_scratch=0 scan_wgs=12 table=0 nsteps=5 max=7", (k, g)


FLAGS = ("no_wide", "no_fold", "no_cache", "late", "mout", "reuse", "plan_use", "segs_built", "band_table")


def test_input_changes_nothing_where_it_does_not_apply(dump):
    """t0_fly (the host-model flavour), gathered moments, a band phase, `table` off: the plan with f2py_table = 0, step for
    step, over every combination of the other switches; and no plan is longer than SB_PLAN_MAX_STEPS."""
    sels = (("t0_fly", dict(t0_fly=1)), ("t0_fly_gathered", dict(t0_fly=1, gathered=1)), ("gathered", dict(gathered=1)),
            ("ph1", dict(phases=1)), ("ph2", dict(phases=2)), ("ph1_gathered", dict(phases=1, gathered=1)),
            ("ph2_gathered", dict(phases=2, gathered=1)), ("table_off", dict(table=0)), ("table_off_t0_fly", dict(table=0, t0_fly=1)))
    lines = []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, bits))
        for name, sel in sels:
            for hint, esize in ((6, 8), (24, 4), (31, 8)):
                for tag in (0, 1):
                    lines.append(_line(f"{name}/{len(lines)}/{tag}", **dict(dict(hint=hint, esize=esize, **kw), **sel, f2py_table=tag)))
    got = dump(lines)
    labels = list(got)
    assert len(labels) == (1 << len(FLAGS)) * len(sels) * 3 * 2
    for off, on in zip(labels[0::2], labels[1::2]):
        assert off.endswith("/0") and on.endswith("/1")
        assert got[on] == got[off], (on, got[on], got[off])
        n, mx = (int(s.split("=")[1]) for s in got[on][2].split()[-2:])
        assert n == len(got[on][1]) <= mx == 7
    # ... and where it does apply, every combination of the other switches gives six steps
    lines = []
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        lines.append(_line(f"on/{len(lines)}", **dict(zip(FLAGS, bits))))
    for k, g in dump(lines).items():
        assert len(g[1]) == 6 and g[2].endswith("table=1 nsteps=6 max=7"), (k, g)


def _cache(exe, lines):
    return pd.run(exe, lines)


def test_window_cache_host_half_for_wrapper_calls(exe):
    """The key of a wrapper call carries SB_BND_WRAPPER and rows = nlats - 1: stream steps on a standing mask are steady
    from the second on; a host-model table call on the same planes in between has another key, and so has the wrapper
    call after it; a call that is no such table call (the switch off, another flavour without its switch) drops the key."""
    nx, ny = 160, 112
    wr = lambda seq: f"call {nx} {ny} 0 {BND_WRAPPER} {ny - 1} 1 2 3 4 {seq}"
    gl = lambda seq: f"call {nx} {ny} 0 {BND_GLOBAL} {ny} 1 2 3 4 {seq}"
    assert _cache(exe, [wr(1), wr(2), wr(3)]) == ["no_key", "steady", "steady"]
    assert _cache(exe, [wr(1), gl(2), wr(3), wr(4)]) == ["no_key", "key_differs", "key_differs", "steady"]
    assert _cache(exe, [wr(1), "other", wr(3), wr(4)]) == ["no_key", "other_call", "steady"]
    assert _cache(exe, [wr(5), wr(5)]) == ["no_key", "seq_restart"]
