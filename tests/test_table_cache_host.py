"""The host's half of the window cache of the table contrast (sb_set_table_window_cache; seabreeze_param_amd/csrc/
sb_table_cache.hpp): when the host forces a table call to search every window again, and the word of plane W.

The device's half -- k_scan reports a changed plane under the call's number -- sees a coast that moved, but only the host
knows which call left the planes k_scan compared with.  tests/plan_dump.cpp drives the decision from standard input
(its `call`, `other`, `failed`, `toggled` and `word` commands); it is built host-only (tests/plan_dump.py).  Every forcing
condition is run on its own from a steady state, and the call after it is steady again.
"""
import numpy as np
import pytest

import plan_dump as pd
import table_ref as tr

FIELDS = ("nx", "ny", "h", "bnd", "rows", "band", "cls", "W", "C")
KEY = dict(nx=160, ny=112, h=0, bnd=1, rows=112, band=4096, cls=8192, W=12288, C=16384)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = pd.build(tmp_path_factory)
    return lambda lines: pd.run(exe, lines)


def _call(seq, **kw):
    k = dict(KEY, **kw)
    return "call " + " ".join(str(k[f]) for f in FIELDS) + f" {seq}"


def test_first_call_fills_and_the_coast_that_stands_is_steady(dump):
    assert dump([_call(1), _call(2), _call(3), _call(50)]) == ["no_key", "steady", "steady", "steady"]


@pytest.mark.parametrize("field", FIELDS)
def test_every_field_of_the_key_forces(dump, field):
    """geometry, boundary rule, ghost width, rows, and the addresses of both planes, of W and of C (a reallocated workspace)"""
    other = _call(3, **{field: KEY[field] + 1})
    assert dump([_call(1), _call(2), other, _call(4, **{field: KEY[field] + 1}), _call(5)]) == \
        ["no_key", "steady", "key_differs", "steady", "key_differs"]


def test_call_numbers_that_start_over_force(dump):
    assert dump([_call(0x7ffffffe), _call(0x7fffffff), _call(1), _call(2)]) == ["no_key", "steady", "seq_restart", "steady"]
    assert dump([_call(7), _call(7)]) == ["no_key", "seq_restart"]


@pytest.mark.parametrize("event, why", [("toggled", "toggled"), ("failed", "failed"), ("other", "other_call")])
def test_events_between_two_calls_force_once(dump, event, why):
    """the switch was set; a launch of the call before failed; another diag call or band step ran k_scan on the planes (the
    dangerous one: that call's k_scan took the report of a moved coast with it)"""
    assert dump([_call(1), _call(2), event, _call(3), _call(4)]) == ["no_key", "steady", why, "steady"]
    assert dump([event, _call(1), _call(2)]) == [why, "steady"]
    assert dump([_call(1), event, event, "other", _call(2), _call(3)])[1:] == [why if event != "other" else "other_call", "steady"]


def test_word_of_w_on_the_block_grid(dump):
    """pack then unpack gives table_ref.table_thc's radius back, and the land-side count of that window; 0 where the tables
    do not answer"""
    nx, ny, w = tr.BLOCK
    land = tr.block_land(nx, ny, w, nx)
    t0 = np.zeros((ny, nx))
    _, nn = tr.table_thc(t0, land)
    assert nn.max() == 40 and nn.min() >= 1
    # (a row of the grid that holds no window: the same cells on a grid the tables cannot answer at all)
    nn0 = tr.table_thc(t0[:, :2], land[:, :2])[1]
    assert not nn0.any()
    Cn = tr._prefix(land, np.uint32)
    yy, xx = (a.ravel() for a in np.mgrid[0:ny, 0:nx])
    nl = tr._window(Cn, True, nx, ny, 0, yy, xx, nn.ravel()).astype(np.int64)
    assert np.all((nl > 0) & (nl < (2 * nn.ravel() + 1) ** 2))
    lines = [f"word 1 {r} {c}" for r, c in zip(nn.ravel(), nl)] + [f"word 0 {r} 0" for r in nn0.ravel()]
    got = np.array([[int(v) for v in ln.split()] for ln in dump(lines)])
    k = nn.size
    assert np.array_equal(got[:k, 1], nn.ravel()) and np.array_equal(got[:k, 2], nl) and np.all(got[:k, 0] != 0)
    assert not got[k:].any()
    # the ends of both fields: radius 1 and the reach, one land-side cell and all but one
    side = (2 * tr.TAB_REACH + 1) ** 2
    ends = dump([f"word 1 1 1", f"word 1 1 8", f"word 1 {tr.TAB_REACH} 1", f"word 1 {tr.TAB_REACH} {side - 1}"])
    assert [ln.split()[1:] for ln in ends] == [["1", "1"], ["1", "8"], [str(tr.TAB_REACH), "1"], [str(tr.TAB_REACH), str(side - 1)]]
    assert all(0 < int(ln.split()[0]) < 2 ** 32 for ln in ends)
