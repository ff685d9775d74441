"""The launch plan of a diag call (seabreeze_param_amd/csrc/sb_diag_plan.hpp): which kernels, in which order, in which mode.

tests/plan_dump.cpp is built host-only with the compiler that builds the library and prints the plan of every case
it is given (tests/plan_dump.py).  The expectations below are written out by hand from the table of launch sequences in
DESIGN.md section 2.3; nothing here is produced by the planner.  The domain is 200 x 96 cells, k_scan runs 12 workgroups there.
"""
import itertools

import pytest

import plan_dump as pd

_line = pd.line


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = pd.build(tmp_path_factory)
    return lambda lines: pd.plans(exe, lines)       # -> {label: (contrast, [steps], kept, guard, guard tail)}


STRIP = "strip=1 Hk=16 tile=32x16 grid=7x6 vb=1 nflag=58"          # 7 strips x (6 + 2 virtual) blocks + 2 counters
STRIP32 = "strip=2 Hk=32 tile=32x16 grid=7x6 vb=2 nflag=72"        # 7 x (6 + 4) + 2
TILE24 = "strip=0 Hk=24 tile=32x32 grid=7x3 vb=0 nflag=23"         # 7 x 3 tiles + 2
TILE32 = "strip=0 Hk=32 tile=32x16 grid=7x6 vb=0 nflag=44"

# label -> (inputs, contrast kernel per precision {8:, 4:}, steps, segs_built after the call, k_wind's scratch planes needed)
BOTH = lambda k: {8: k, 4: k}
CASES = {
    # single domain, host-model flavour, strip kernel, fold on: 3 launches
    "single_fold": (dict(), BOTH(STRIP),
                    ["SCAN:prof=scan,stats=partials*0,final", "CONTRAST:prof=thc,stats=partials*12,fold,final",
                     "WIND:prof=wind,stats=none*0,final"], 1, 0),
    "single_fold_wide": (dict(hint=24), {8: None, 4: STRIP32},
                         ["SCAN:prof=scan,stats=partials*0,final", "CONTRAST:prof=thc,stats=partials*12,fold,final",
                          "WIND:prof=wind,stats=none*0,final"], 1, 0),
    "single_fold_static_sigma": (dict(reuse=1), BOTH(STRIP),
                                 ["SCAN:prof=scan,stats=none*0,final", "CONTRAST:prof=thc,stats=partials*0,fold,final",
                                  "WIND:prof=wind,stats=none*0,final"], 1, 0),
    # lists_stand iff a plan is in use, the lists were built and the plan cache is on
    "single_fold_lists_stand": (dict(plan_use=1, segs_built=1), BOTH(STRIP),
                                ["SCAN:prof=scan,stats=partials*0,final,stand", "CONTRAST:prof=thc,stats=partials*12,fold,final,stand",
                                 "WIND:prof=wind,stats=none*0,final,stand"], 1, 0),
    "single_fold_no_plan": (dict(plan_use=0, segs_built=1), BOTH(STRIP),
                            ["SCAN:prof=scan,stats=partials*0,final", "CONTRAST:prof=thc,stats=partials*12,fold,final",
                             "WIND:prof=wind,stats=none*0,final"], 1, 0),
    "single_fold_lists_not_built": (dict(plan_use=1, segs_built=0), BOTH(STRIP),
                                    ["SCAN:prof=scan,stats=partials*0,final", "CONTRAST:prof=thc,stats=partials*12,fold,final",
                                     "WIND:prof=wind,stats=none*0,final"], 1, 0),
    "single_fold_no_cache": (dict(plan_use=1, segs_built=1, no_cache=1), BOTH(STRIP),
                             ["SCAN:prof=scan,stats=partials*0,final", "CONTRAST:prof=thc,stats=partials*12,fold,final",
                              "WIND:prof=wind,stats=none*0,final"], 1, 0),
    # sb_set_fold(0), or the tile kernel: 4 launches
    "single_no_fold": (dict(no_fold=1, plan_use=1, segs_built=1), BOTH(STRIP),
                       ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final",
                        "CONTRAST:prof=thc,stats=none*0,final", "WIND:prof=wind,stats=none*0,final"], 0, 0),
    "single_tile": (dict(hint=24, no_wide=1), BOTH(TILE24),
                    ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final",
                     "CONTRAST:prof=thc,stats=none*0,final", "WIND:prof=wind,stats=none*0,final"], 0, 0),
    "single_tile_fp64": (dict(hint=24), {8: TILE24, 4: None},
                         ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final",
                          "CONTRAST:prof=thc,stats=none*0,final", "WIND:prof=wind,stats=none*0,final"], 0, 0),
    # f2py flavour: 5 launches
    "single_f2py": (dict(t0_fly=0), BOTH(STRIP),
                    ["SCAN:prof=scan,stats=partials*0,final", "PREP:prof=prep,stats=partials*12,final", "T0:prof=t0,stats=none*0,final",
                     "CONTRAST:prof=thc,stats=none*0,final", "WIND:prof=wind,stats=none*0,final"], 0, 0),
    # band step, default order
    "band_ph1_first": (dict(phases=1, gathered=1, mout=1), BOTH(STRIP),
                       ["SCAN:prof=scan,stats=partials*0,publish", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0"], 0, 1),
    "band_ph1_lists_stand": (dict(phases=1, gathered=1, mout=1, plan_use=1, segs_built=1), BOTH(STRIP),
                             ["SCAN:prof=scan,stats=partials*0,publish", "WIND:prof=wind,stats=none*0,trust"], 0, 1),
    "band_ph1_static_sigma": (dict(phases=1, gathered=1, mout=0, reuse=1, plan_use=1, segs_built=1), BOTH(STRIP),
                              ["SCAN:prof=scan,stats=none*0", "WIND:prof=wind,stats=none*0,trust"], 0, 1),
    "band_ph2": (dict(phases=2, gathered=1), BOTH(STRIP), ["CONTRAST:prof=thc,stats=gathered*0,fold,final,update"], 1, 1),
    "band_ph2_no_fold": (dict(phases=2, gathered=1, no_fold=1), BOTH(STRIP), ["CONTRAST:prof=thc,stats=gathered*0,final,update"], 0, 1),
    "band_ph2_static_sigma": (dict(phases=2, gathered=1, reuse=1), BOTH(STRIP), ["CONTRAST:prof=thc,stats=none*0,fold,final,update"], 1, 1),
    "band_ph2_tile": (dict(phases=2, gathered=1, hint=24, no_wide=1), BOTH(TILE24), ["CONTRAST:prof=thc,stats=gathered*0"], 0, 1),
    # band step, sb_set_band_order(1), strip kernel, fold on
    "late_ph1": (dict(phases=1, gathered=1, mout=1, late=1), BOTH(STRIP), ["SCAN:prof=none,stats=partials*0,publish,final"], 0, 0),
    "late_ph2": (dict(phases=2, gathered=1, late=1, plan_use=1, segs_built=1), BOTH(STRIP),
                 ["CONTRAST:prof=none,stats=gathered*0,fold,final", "WIND:prof=none,stats=none*0,final"], 1, 0),
    # ... which needs the fold: without it the default order stands
    "late_no_fold_ph1": (dict(phases=1, gathered=1, mout=1, late=1, no_fold=1), BOTH(STRIP),
                         ["SCAN:prof=scan,stats=partials*0,publish", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0"], 0, 1),
    # plain call with sb_use_gathered_moments (Python-driven bands)
    "gathered_host_model": (dict(gathered=1), BOTH(STRIP),
                            ["SCAN:prof=scan,stats=none*0", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0",
                             "CONTRAST:prof=thc,stats=gathered*0,fold,final,update"], 1, 1),
    "gathered_f2py": (dict(gathered=1, t0_fly=0), BOTH(STRIP),
                      ["SCAN:prof=scan,stats=none*0", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0",
                       "MERGE:prof=none,stats=gathered*0", "T0:prof=t0,stats=none*0", "CONTRAST:prof=thc,stats=none*0,final,update"], 0, 1),
    "gathered_f2py_static_sigma": (dict(gathered=1, t0_fly=0, reuse=1), BOTH(STRIP),
                                   ["SCAN:prof=scan,stats=none*0", "PREP:prof=prep,stats=none*0", "WIND:prof=wind,stats=none*0",
                                    "T0:prof=t0,stats=none*0", "CONTRAST:prof=thc,stats=none*0,final,update"], 0, 1),
}


def test_named_cases(dump):
    lines, want = [], {}
    for name, (kw, contrast, steps, built, scratch) in CASES.items():
        for esize in (8, 4):
            if contrast[esize] is None:
                continue
            lines.append(_line(f"{name}/{esize}", esize=esize, **kw))
            want[f"{name}/{esize}"] = (contrast[esize], steps, pd.kept(built, scratch, 0, len(steps)),
                                       pd.GUARD_OFF, pd.TAIL_OFF)
    got = dump(lines)
    for label in want:
        assert got[label] == want[label], label


def test_contrast_kernel_by_radius_hint(dump):
    """Halos up to 16: the strip kernel; beyond, the 96-column strip kernel in single precision and tiles in double."""
    want = {(8, 8): STRIP, (8, 16): STRIP, (8, 17): TILE24, (8, 24): TILE24, (8, 31): TILE32,
            (4, 8): STRIP, (4, 16): STRIP, (4, 17): STRIP32, (4, 24): STRIP32, (4, 31): STRIP32}
    got = dump([_line(f"{e}/{h}", esize=e, hint=h) for e, h in want])
    for (e, h), k in want.items():
        assert got[f"{e}/{h}"][0] == k, (e, h)
    # sb_set_wide_strip(0), and a block grid the position plane cannot hold: tiles
    got = dump([_line("narrow", esize=4, hint=31, no_wide=1), _line("nofit16", hint=16, fits=0), _line("nofit31", esize=4, hint=31, fits=0)])
    assert [got[k][0] for k in ("narrow", "nofit16", "nofit31")] == [TILE32, TILE24, TILE32]


def test_invariants_over_the_input_space(dump):
    flags = ("t0_fly", "no_wide", "no_fold", "no_cache", "late", "gathered", "mout", "reuse", "plan_use", "segs_built")
    lines = []
    for phases, esize, hint, wgs in itertools.product((1, 2, 3), (8, 4), (16, 24, 31), (12, 1025)):
        for bits in itertools.product((0, 1), repeat=len(flags)):
            lines.append(_line(f"c{len(lines)}", phases=phases, esize=esize, hint=hint, wgs=wgs, **dict(zip(flags, bits))))
    got = dump(lines)
    assert len(got) == 3 * 2 * 3 * 2 * 1024
    for label, (contrast, steps, kept, _, _) in got.items():
        names = [s.split(":")[0] for s in steps]
        assert 1 <= len(steps) <= 6, (label, steps)
        assert names.count("CONTRAST") <= 1 and names.count("WIND") <= 1, (label, steps)
        fold = False
        if "CONTRAST" in names:
            fold = "fold" in steps[names.index("CONTRAST")].split(",")
        if "WIND" in names and "CONTRAST" in names:
            final = "final" in steps[names.index("WIND")].split(",")
            assert final == (names.index("WIND") > names.index("CONTRAST")), (label, steps)
        assert kept.split()[0] == f"segs_built={int(fold)}", (label, steps, kept)
