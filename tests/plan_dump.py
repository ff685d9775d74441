"""tests/plan_dump.cpp for the tests of seabreeze_param_amd/csrc/sb_diag_plan.hpp, sb_table_cache.hpp and sb_ice_plan.hpp: built
host-only with the compiler that builds the library, once per session; the lines it reads and the sections of the lines it
prints.

A plan's line is  label | contrast | steps | kept | guard | guard tail;  `parse` gives the five sections behind the label,
the steps as a list.  The domain is 200 x 96 cells, k_scan runs 12 workgroups there.
"""
import collections
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the inputs of a `plan` line and the defaults plan_dump.cpp gives them: a line names only what differs
FIELDS = ("phases", "esize", "t0_fly", "hint", "no_wide", "no_fold", "no_cache", "late", "gathered", "mout", "reuse",
          "plan_use", "segs_built", "wgs", "fits", "nx", "table", "band_table", "f2py_table", "guard", "guard_bands")
DEFAULT = dict(phases=3, esize=8, t0_fly=1, hint=6, no_wide=0, no_fold=0, no_cache=0, late=0, gathered=0, mout=0, reuse=0,
               plan_use=0, segs_built=0, wgs=12, fits=1, nx=200, table=0, band_table=0, f2py_table=0, guard=0, guard_bands=0)
# ... and of a `switches` line beside them: the context's six switches and what run_diag knows of the call
SWITCHES = ("sw_table", "sw_table_bands", "sw_table_f2py", "sw_table_cache", "sw_guard", "sw_guard_bands")
CALL_DEFAULT = dict(dict.fromkeys(SWITCHES, 0), host_model=1, bnd=1, ghost=0, band_geo=0)
BND_WRAPPER, BND_GLOBAL, BND_HALO = 0, 1, 2
# the section of a call the guard does not serve, and the fields sb_set_nonfinite_guard_bands adds where it does not apply
GUARD_OFF, TAIL_OFF = "guard=0 nlaunch=0", "taint_before=-1 update=0"

Plan = collections.namedtuple("Plan", "contrast steps kept guard tail")
_exe = None


def build(tmp_path_factory):
    global _exe
    if _exe is None:
        cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not (shutil.which(cxx) or os.path.exists(cxx)):
            pytest.skip("no hipcc to build tests/plan_dump.cpp with")
        out = str(tmp_path_factory.mktemp("plan_dump") / "plan_dump")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-x", "c++", os.path.join(ROOT, "tests", "plan_dump.cpp"), "-o", out], check=True)
        _exe = out
    return _exe


def _pairs(defaults, kw):
    unknown = set(kw) - set(defaults)
    assert not unknown, unknown
    return [f"{k}={v}" for k, v in kw.items() if v != defaults[k]]


def line(label, **kw):
    return " ".join(["plan", label] + _pairs(DEFAULT, kw))


def switches_line(label, **kw):
    return " ".join(["switches", label] + _pairs(dict(DEFAULT, **CALL_DEFAULT), kw))


def run(exe, lines):
    """-> the lines the program prints (one for every `plan`, `switches`, `call` and `word`)"""
    return subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]


def ice_dump(tmp_path_factory, layout):
    """-> run(lines) over the `layout` lines ("ice", "band_ice", "um_ice": sb_ice_plan.hpp) of the program: it takes P and M
    lines without the layout's word and gives {label: [the fields behind the label]}"""
    exe = build(tmp_path_factory)

    def run_layout(lines):
        res = {ln.split()[0]: ln.split()[1:] for ln in run(exe, [f"{layout} {ln}" for ln in lines])}
        assert len(res) == len(lines)
        return res
    return run_layout


def parse(ln):
    """-> (label, Plan)"""
    label, contrast, steps, kept, guard, tail = (s.strip() for s in ln.split("|"))
    return label, Plan(contrast, steps.split(), kept, guard, tail)


def plans(exe, lines):
    """-> {label: Plan} of `plan` lines with labels of their own"""
    res = dict(parse(ln) for ln in run(exe, lines))
    assert len(res) == len(lines)
    return res


def kept(segs_built, wind_scratch, table, nsteps):
    return f"segs_built={segs_built} wind_scratch={wind_scratch} scan_wgs=12 table={table} nsteps={nsteps} max=7"


def names(steps):
    return [s.split(":")[0] for s in steps]


def parse_switches(ln):
    """-> (label, {field: int}) of a `switches` line"""
    label, rest = ln.split("|", 1)
    return label.strip(), {k: int(v) for k, v in (kv.split("=") for kv in rest.replace("|", " ").split())}
