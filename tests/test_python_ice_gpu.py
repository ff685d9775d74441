"""seabreezediag.diag(..., ice_on_device=True): one stream for the whole call, the ice planes handed to the device ahead
of their steps (python_wrapper/seabreezediag/__init__.py; seabreeze_f2py.f90: stream_coast, stream_ice,
stream_ice_report), against the same call on the step-by-step path -- get_edges + get_dist on the host for every plane
that differs -- bit for bit.  Without the keyword the driver still closes and reopens its stream round a new distance
field."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

PW = os.path.join(ROOT, "python_wrapper")
pytestmark = pytest.mark.gpu


def _import_surface():
    assert any(f.startswith("seabreeze.") and f.endswith(".so") for f in os.listdir(PW)), \
        "python_wrapper extension missing: __graft_entry__.build() makes it"
    if PW not in sys.path:
        sys.path.insert(0, PW)
    import seabreeze
    import seabreezediag
    assert os.path.dirname(seabreeze.__file__) == PW, seabreeze.__file__
    return seabreeze, seabreezediag


class _Reader:
    """A file-variable stand-in: every read hands out a view of a fresh buffer (tests/test_python_surface.py)."""

    def __init__(self, planes):
        self.planes, self.shape = planes, planes.shape

    def __getitem__(self, ts):
        buf = np.empty((1,) + self.planes.shape[1:], np.float32)
        buf[0] = self.planes[ts]
        return np.ma.MaskedArray(buf[0])


def _case(nt, nlat, nlon, nlev):
    """Inputs in the reference driver's conventions; the ice changes ahead of steps 3, 4 and 7 (counted from 1), each time
    by a row of the northern sea -- on the 0.25-degree regional grid a window of six cells sees it, on the global one the
    coast cells themselves move."""
    from seabreeze_param_amd import synth
    st = synth.static_fields(nlon, nlat, np.float32)
    if nlon == 700:
        st.lon = (100.0 + 0.25 * np.arange(nlon)).astype(np.float32)
        st.lat = (70.0 + 0.25 * (np.arange(nlat) - nlat // 2)).astype(np.float32)
        r = synth.hash_uniform((nlat, nlon), 3, 78)
        s = r + np.roll(r, 1, 1) + np.roll(r, 1, 0) + np.roll(r, -1, 1)
        st.landfrac = (s > 2.45).astype(np.float32)
    pres = (synth.pressure_1d(nlev, np.float32) / 100.0).astype(np.float32)
    t = np.stack([synth.theta_step(st, k + 1, np.float32) for k in range(nt)])
    uv = [synth.wind_step(st, nlev, k + 1, np.float32) for k in range(nt)]
    u = np.stack([a for a, _ in uv]); v = np.stack([b for _, b in uv])
    rows = np.array([8, 8, 9, 11, 11, 11, 10, 10, 10, 10, 10, 10])[:nt]          # changes at steps 3, 4, 7
    sea = st.landfrac == 0
    ci = np.stack([np.where((np.arange(nlat)[:, None] >= nlat - r) & sea, 0.6, 0.0) for r in rows]).astype(np.float32)
    return st, pres, u, v, t, ci


@pytest.mark.parametrize("reader", [False, True], ids=["array", "reader"])
@pytest.mark.parametrize("shape", [(96, 72), (700, 96)])
def test_ice_on_device_equals_the_step_by_step_driver(monkeypatch, shape, reader):
    seabreeze, sbd = _import_surface()
    nlon, nlat = shape
    nt, nlev = 12, 4
    st, pres, u, v, t, ci = _case(nt, nlat, nlon, nlev)
    args = (st.landfrac, st.z, st.sigma, st.lon, st.lat, pres)
    kw = dict(timestep=120.0, maxdist=700.0 if nlon == 96 else 180.0, ice_on_device=True)
    ice = (lambda a: _Reader(a)) if reader else (lambda a: a)
    reports = []

    def run():
        monkeypatch.setitem(sbd._dist_cache, "key", None)
        a = sbd.diag(1, *args, u[:9], v[:9], t[:9], ice(ci[:9]), **kw)
        reports.append((sbd.stream_stats()[0], [int(x) for x in seabreeze.stream_ice_report()]))
        b = sbd.diag(a[0], *args, u[9:], v[9:], t[9:], ice(ci[9:]), ws=a[3], wd=a[4], thc=a[2], **kw)    # the state is carried on
        return a, b

    monkeypatch.delenv("SEABREEZE_NO_STREAM", raising=False)
    opened = {"n": 0}
    begin = seabreeze.stream_begin
    monkeypatch.setattr(seabreeze, "stream_begin", lambda *a, **k: (opened.__setitem__("n", opened["n"] + 1), begin(*a, **k))[1])
    sa, sb_ = run()
    assert opened["n"] == 2                                       # one stream per call, whatever the ice did
    steps, rep = reports[0]
    assert steps == 9                                             # nine steps in one stream
    tiles = nlat * ((nlon + 255) // 256)
    assert rep[0] == 9 and rep[1] == 3 and rep[3] == tiles        # nine ice calls, three of them moved the coast
    assert 0 <= rep[2] <= tiles
    monkeypatch.setenv("SEABREEZE_NO_STREAM", "1")
    ca, cb = run()
    for x, y in ((sa, ca), (sb_, cb)):
        assert x[0] == y[0]
        assert np.array_equal(x[1][:, :-1], y[1][:, :-1])         # sb_con: same kernels, same distance fields, same bits
        for k in (2, 3, 4):
            assert np.array_equal(x[k][:-1], y[k][:-1])
    assert (sa[1][:, :-1] < 1e19).any()                           # (band cells exist: the comparison is of numbers)


def test_no_ice_is_one_call_with_zeros(monkeypatch):
    seabreeze, sbd = _import_surface()
    st, pres, u, v, t, ci = _case(4, 72, 96, 3)
    args = (st.landfrac, st.z, st.sigma, st.lon, st.lat, pres)
    monkeypatch.delenv("SEABREEZE_NO_STREAM", raising=False)
    monkeypatch.setitem(sbd._dist_cache, "key", None)
    a = sbd.diag(1, *args, u, v, t, None, timestep=120.0, maxdist=700.0, ice_on_device=True)
    assert [int(x) for x in seabreeze.stream_ice_report()][:2] == [1, 0]
    b = sbd.diag(1, *args, u, v, t, None, timestep=120.0, maxdist=700.0)
    assert np.array_equal(a[1][:, :-1], b[1][:, :-1]) and all(np.array_equal(a[k][:-1], b[k][:-1]) for k in (2, 3, 4))


def test_without_the_keyword_the_stream_still_closes_and_reopens(monkeypatch):
    """The sequence of test_streamed_driver_equals_step_by_step_driver (tests/test_python_surface.py): the ice grows once,
    ahead of step 6 of the first call, so that call opens two streams and the second call one."""
    seabreeze, sbd = _import_surface()
    from test_python_surface import _stream_case
    nt, nlat, nlon, nlev = 9, 72, 96, 4
    st, pres, u, v, t, ci = _stream_case(nt, nlat, nlon, nlev, ice_change_at=5)
    args = (st.landfrac, st.z, st.sigma, st.lon, st.lat, pres)
    kw = dict(timestep=120.0, maxdist=700.0)
    monkeypatch.delenv("SEABREEZE_NO_STREAM", raising=False)
    monkeypatch.setitem(sbd._dist_cache, "key", None)
    opened = {"n": 0, "coast": 0}
    begin = seabreeze.stream_begin
    monkeypatch.setattr(seabreeze, "stream_begin", lambda *a, **k: (opened.__setitem__("n", opened["n"] + 1), begin(*a, **k))[1])
    coast = seabreeze.stream_coast
    monkeypatch.setattr(seabreeze, "stream_coast", lambda *a, **k: (opened.__setitem__("coast", opened["coast"] + 1), coast(*a, **k))[1])
    a = sbd.diag(1, *args, u[:6], v[:6], t[:6], ci[:6], **kw)
    assert opened["n"] == 2
    sbd.diag(a[0], *args, u[6:], v[6:], t[6:], ci[6:], ws=a[3], wd=a[4], thc=a[2], **kw)
    assert opened["n"] == 3 and opened["coast"] == 0
    assert sbd.stream_stats()[0] == 3                             # the last stream of the second call, as ever
