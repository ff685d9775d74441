"""Python driver layer over the `seabreeze` extension module (MI355X build).

Counterpart of the reference's ``seabreezediag`` package
(ref: python_wrapper/seabreezediag/__init__.py:13-40 ``c2f``, :91-263 ``diag``): same call
signature, same array conventions, same return tuple, so scripts written against the
reference keep working with ``import seabreezediag``.  The `seabreeze` module it imports
is the f2py surface built from python_wrapper/seabreeze_f2py.f90, whose routines run on
the GPU through libseabreeze_hip.so.

Conventions kept from the reference
  * 2-D fields are C-ordered ``(lat, lon)``, winds ``([time,] pres, lat, lon)``; ``c2f``
    flips them into the Fortran ``(lon, lat[, pres])`` layout the kernels use.
  * ``tt`` is the running timestep number (clamped to >= 1) and comes back advanced by the
    number of steps processed.
  * The second returned state array is the sea-level temperature t0 (output plane 2), which
    the reference hands back under the name ``thc`` (ref :244); the
    kernel never reads that state, so this is harmless and kept.
  * The last latitude row of every output plane is never written by the kernel
    (ref: seabreeze_diag_python.f90:165).

Differences (both are crashes in the reference)
  * ``ci=None`` works: no sea ice, the coast distance is computed once.
  * inputs without a time axis work.

Streaming.  The reference's loop hands the kernel the same ``z``, ``std`` and distance
field at every step and threads ``ws, wd, thc`` through its return values (ref :222-245).  Where the extension
offers ``stream_begin / stream_step / stream_end`` (this build does) those planes stay on the device for the whole
call: a step uploads ``theta`` and the one ``u, v`` plane the pressure vector selects and receives the ``sb_con``
plane of the step before it, written in place into the result array, so the host copies of step i+1 overlap the
device work of step i.  Same numbers as the step-by-step path (``SEABREEZE_NO_STREAM=1`` selects that one).

A failed device call (no GPU, out of memory, ...) raises ``RuntimeError`` with the library's message: the
extension records a status instead of stopping the interpreter, and every call here checks it.
"""
import os
import warnings

import numpy as np

import seabreeze as _ext

__all__ = ["diag", "c2f", "read_nc", "get_edges", "get_dist", "stream_stats"]

_HAVE_STREAM = all(hasattr(_ext, n) for n in ("stream_begin", "stream_step", "stream_end"))


def _check(what):
    """Raise if the last call into the extension failed (it records a status; it never stops the interpreter)."""
    if hasattr(_ext, "last_status") and _ext.last_status() != 0:
        msg = _ext.last_message()
        msg = msg.decode(errors="replace") if isinstance(msg, bytes) else str(msg)
        raise RuntimeError(f"{what}: {msg.strip()}")


def get_edges(lsm, ci, **kw):
    out = _ext.get_edges(lsm, ci, **kw)
    _check("get_edges")
    return out


def get_dist(coast, mask, lon, lat, **kw):
    out = _ext.get_dist(coast, mask, lon, lat, **kw)
    _check("get_dist")
    return out


def _diag_kernel(*args, **kw):
    out = _ext.diag(*args, **kw)
    _check("diag")
    return out


def stream_stats():
    """(steps, [host copies, enqueueing, waiting] in seconds) of the last streamed ``diag`` call."""
    return _ext.stream_stats() if hasattr(_ext, "stream_stats") else (0, [0.0, 0.0, 0.0])


def c2f(array):
    """Reinterpret a C-ordered array as the Fortran-ordered array with reversed shape.  Element for
    element that is the transpose whatever the memory layout of the input (ravel in C order, refill in
    Fortran order), so the transpose *view* is returned: no copy for C- or Fortran-contiguous input."""
    return np.asarray(array).T


def _pop(kwargs, key, default=None):
    return kwargs.pop(key) if key in kwargs else default


_dist_cache = {"key": None, "dist": None}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _coast_distance(lsm, ice, lon, lat, static_known_same=False):
    """Signed coast distance for this land mask and sea-ice field.  The reference recomputes it at
    every timestep (ref :223-228); the result depends only on these four inputs, so the last one is
    kept and reused while they compare equal to the copies kept with it --
    sea ice in reanalysis files changes daily, not with every model step.  An exact comparison
    (a memcmp-speed pass) rather than a digest: cheaper, and no collision to argue about.
    `static_known_same`: the caller has already compared lsm, lon, lat with the kept copies (they do not
    change inside one diag call), so only the ice field is compared."""
    key = _dist_cache["key"]
    same = key is not None and _same(ice, key[1]) and (
        static_known_same or (_same(lsm, key[0]) and _same(lon, key[2]) and _same(lat, key[3])))
    if not same:
        _dist_cache["dist"] = c2f(get_dist(get_edges(c2f(lsm), c2f(ice)), c2f(lsm), lon, lat))
        _dist_cache["key"] = tuple(np.array(a, copy=True) for a in (lsm, ice, lon, lat))
    return _dist_cache["dist"]


def _set_table_contrast(on, keep_windows=False):
    """The extension's table switches (seabreeze_f2py.f90: set_table_contrast) on the module's device context."""
    if not hasattr(_ext, "set_table_contrast"):
        raise RuntimeError("table_contrast=True: this build of the `seabreeze` extension has no set_table_contrast")
    _ext.set_table_contrast(1 if on else 0, 1 if (on and keep_windows) else 0)
    _check("set_table_contrast")


def _set_nonfinite_guard(on):
    """The extension's guard switch (seabreeze_f2py.f90: set_nonfinite_guard) on the module's device context."""
    if not hasattr(_ext, "set_nonfinite_guard"):
        raise RuntimeError("guard_nonfinite=True: this build of the `seabreeze` extension has no set_nonfinite_guard")
    _ext.set_nonfinite_guard(1 if on else 0)
    _check("set_nonfinite_guard")


def diag(tt, lsm, z, std, lon, lat, pres, *args, **kwargs):
    """Potential sea-breeze convergence strength in the coastal band
    (Bergemann et al. 2017, doi:10.1002/2017MS001048).

    Positional: ``tt, lsm, z, std, lon, lat, pres, u, v, t, ci`` -- or pass ``meta=`` (an
    object with attributes ``u, v, theta`` and optionally ``ci``) instead of the last four.
    Keywords: state ``ws, wd, thc`` from the previous call (default zeros); ``out`` -- a float64
    ``(ntime, lat, lon)`` array to receive ``sb_con`` in place of a fresh one (not in the reference;
    every plane is overwritten); plus the kernel
    tunables ``target_plev`` [hPa], ``thresh_wind``, ``thresh_winddir``, ``thresh_windch``,
    ``thresh_thc``, ``target_time`` [h], ``maxdist`` [km], ``timestep`` [min].
    ``table_contrast=True`` (not in the reference; off by default): every step of this call takes the land-sea
    contrast from device-wide summed-area tables, at a cost per band cell that does not depend on the radius of its
    window -- for grids of a few km, whose band cells lie further than 32 cells from the other class (radii up to 127;
    include/seabreeze_hip.h: ``sb_set_table_contrast`` with ``sb_set_table_contrast_f2py``).  ``keep_windows=True``
    beside it keeps every band cell's window while the coast stands (``sb_set_table_window_cache``): the same
    numbers, less work per step.  Both are switched on before the first step and off again when the call returns.
    ``guard_nonfinite=True`` (not in the reference; off by default): NaN, Inf and missing values (2e20) in ``t`` -- what
    reanalysis files carry -- reach ``thc`` and ``sb_con`` as they do in the reference: every step finds such cells and
    computes the band cells whose windows hold them again, the reference's way (``sb_set_nonfinite_guard``; without it
    those cells hold finite, wrong numbers).  Switched on before the first step and off again when the call returns.

    ``ice_on_device=True`` (not in the reference; off by default): for sea ice that moves.  The stream is opened once and
    keeps the land mask and the coast on the device; every step whose ice plane is not provably the memory of the step
    before hands its plane to ``stream_ice``, which finds the coast cells that changed and computes again only the part
    of the distance field they can reach -- the same numbers as ``get_edges`` + ``get_dist`` of every step, with no
    distance field, comparison or close-and-reopen on the host (``sb_diag_stream_coast``, ``sb_diag_stream_ice``).  The
    distance field is made with ``get_dist``'s default ``maxdist`` of 180 km, as by the driver without the keyword.  On
    the step-by-step path (``SEABREEZE_NO_STREAM=1``) the keyword changes nothing.

    Returns ``(tt, sb_con, thc, ws, wd)``; ``sb_con`` is float64 ``(ntime, lat, lon)``.
    """
    table = bool(_pop(kwargs, "table_contrast", False))
    keep = bool(_pop(kwargs, "keep_windows", False))
    guard = bool(_pop(kwargs, "guard_nonfinite", False))
    if not table and not guard:
        return _diag(tt, lsm, z, std, lon, lat, pres, *args, **kwargs)
    if guard:
        _set_nonfinite_guard(True)
    try:
        if table:
            _set_table_contrast(True, keep)
        return _diag(tt, lsm, z, std, lon, lat, pres, *args, **kwargs)
    finally:
        try:
            if table:
                _set_table_contrast(False)
        finally:
            if guard:
                _set_nonfinite_guard(False)


def _diag(tt, lsm, z, std, lon, lat, pres, *args, **kwargs):
    ice_dev = bool(_pop(kwargs, "ice_on_device", False))
    ws, wd, thc = (_pop(kwargs, k) for k in ("ws", "wd", "thc"))
    meta = _pop(kwargs, "meta")
    out_arr = _pop(kwargs, "out")
    if meta is None:
        u, v, t, ci = args
    else:
        u, v, t = meta.u, meta.v, meta.theta
        ci = getattr(meta, "ci", None)
    tt = max(1, tt)
    names = {"ws": "Windspeed", "wd": "Wind direction", "thc": "Heating contrast"}
    state = {}
    for key, val in (("ws", ws), ("wd", wd), ("thc", thc)):
        if val is None:
            if tt > 1:
                warnings.warn(f"{names[key]} should be given from previous timestep")
            val = np.zeros_like(lsm)
        state[key] = val
    # The kernels update windspeed / winddir / thc in place (ref: seabreeze_diag_python.f90:237-239,
    # 268-273) and f2py hands Fortran-contiguous float32 arrays through without a copy, so the state is
    # kept in private arrays: the caller's arrays (e.g. what an earlier call returned) are never written.
    # thc is write-only in the kernel: one scratch plane serves every step.
    ws, wd = (np.array(state[k], dtype=np.float32, order="C") for k in ("ws", "wd"))
    thc = np.empty_like(ws)

    # arrays or file variables (netCDF4 / scipy: they carry `shape`, and only slicing reads them)
    shape_of = lambda a: tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    has_time = len(shape_of(v)) > 3
    nt = shape_of(v)[0] if has_time else 1
    nlat, nlon = shape_of(t)[-2:]
    if out_arr is None:
        sb_all = np.zeros([nt, nlat, nlon])       # float64 like the reference's (ref :214)
    else:
        # the caller's result array, written in place and returned (a driver that steps through many chunks hands the
        # same array in again and pays the page faults of a fresh (nt, lat, lon) float64 array once, not per chunk)
        if not (isinstance(out_arr, np.ndarray) and out_arr.dtype == np.float64 and out_arr.shape == (nt, nlat, nlon)
                and out_arr.flags.c_contiguous and out_arr.flags.writeable):
            raise ValueError(f"out= must be a writeable C-contiguous float64 array of shape {(nt, nlat, nlon)}")
        sb_all = out_arr
        sb_all[:, -1, :] = 0.0                    # (the kernels leave the last latitude row alone, ref seabreeze_diag_python.f90:165:
                                                  #  in a fresh result array it reads 0.0, so it does here)
    streaming = _HAVE_STREAM and not os.environ.get("SEABREEZE_NO_STREAM")
    ice_dev = ice_dev and streaming                # (the step-by-step path has no resident distance field to update)
    if ice_dev and not all(hasattr(_ext, n) for n in ("stream_coast", "stream_ice")):
        raise RuntimeError("ice_on_device=True: this build of the `seabreeze` extension has no stream_coast / stream_ice")
    dist = None if (ci is not None or ice_dev) else _coast_distance(lsm, np.zeros_like(lsm), lon, lat)

    static_seen = [False]
    last_ice = [None]                                        # the ice plane of the step before, where it is PROVABLY this one

    def ice_plane(ts):
        """The step's ice plane as float32, and where it lies if it is provably the caller's own memory (else None)."""
        ice = ci[ts] if has_time else ci
        ice = ice.filled(0) if hasattr(ice, "filled") else ice
        ice = np.asarray(ice, dtype=np.float32)              # what f2py would make of it (file data may be big-endian)
        provable = isinstance(ci, np.ndarray) and np.may_share_memory(ice, ci)
        return ice, ((ice.__array_interface__["data"][0], ice.shape, ice.strides) if provable else None)

    def step_inputs(ts):
        nonlocal dist
        if ci is not None and not ice_dev:
            ice, where = ice_plane(ts)
            # the reference recomputes it every step (:223-228); here: when the ice changes.  lsm, lon, lat are this
            # call's arguments: compared with the kept copies at the first step only.  The comparison of the ice plane
            # itself (0.3 ms at 1024 x 768) is skipped only where the plane is provably the memory of the step before:
            # `ci` is an array the CALLER holds (so it outlives this loop and no reader refills it between steps) and
            # this step's plane is the same window into it -- a broadcast time axis, or no time axis.  An equal address
            # alone proves nothing: a file reader hands out views of per-read temporaries (netCDF4's `data[...]`, a
            # nomask MaskedArray's `filled()`), and the next read may land where the last one was freed.
            if not (static_seen[0] and where is not None and where == last_ice[0]):
                dist = _coast_distance(lsm, ice, lon, lat, static_known_same=static_seen[0])
            last_ice[0] = where
            static_seen[0] = True
        return (t[ts], v[ts], u[ts]) if has_time else (t[:], v[:], u[:])

    f32 = lambda a: np.asarray(a, dtype=np.float32)
    if ice_dev:
        # one stream for the whole call: the land mask and the coast stay on the device beside z, std and the state, and
        # an ice plane that may differ from the one before is handed over ahead of its step -- the device finds out what
        # moved and computes that part of the distance field again (seabreeze_f2py.f90: stream_coast, stream_ice).  No
        # distance field on the host, no comparison of planes, no close and reopen.
        zf, sdf, pf = c2f(f32(z)), c2f(f32(std)), c2f(f32(pres))
        scratch = np.zeros((nlon, nlat), order="F")
        nothing = np.zeros((nlon, nlat), np.float32, order="F")
        _ext.stream_begin(zf, sdf, nothing, c2f(f32(ws)), c2f(f32(wd)), c2f(f32(thc)))     # (the first ice call fills cdist)
        _check("stream_begin")
        _ext.stream_coast(c2f(f32(lsm)), f32(lon), f32(lat))     # get_dist's default maxdist, as the reference's driver (ref :228)
        _check("stream_coast")
        last = None
        for ts in range(nt):
            if ci is None:
                ice, where = nothing.T, "no ice"
            else:
                ice, where = ice_plane(ts)
            if where is None or where != last:
                _ext.stream_ice(c2f(ice))
                _check("stream_ice")
            last = where
            tk, vk, uk = step_inputs(ts)
            _ext.stream_step(tt, pf, c2f(f32(tk)), c2f(f32(vk)), c2f(f32(uk)), scratch if ts == 0 else c2f(sb_all[ts - 1]), **kwargs)
            _check("stream_step")
            tt += 1
        out, ws, wd, thc = _ext.stream_end(c2f(sb_all[nt - 1]))
        _check("stream_end")
        out = c2f(out)
        return tt, sb_all, np.array(out[1]), np.array(out[2]), np.array(out[3])
    if streaming:
        # z, std, the distance field and the carried state stay on the device; sb_con of step ts-1 arrives while
        # step ts is being staged, straight into its plane of sb_all (the transpose view of a C-ordered plane is
        # the Fortran-ordered array the extension writes in place)
        zf, sdf, pf = c2f(f32(z)), c2f(f32(std)), c2f(f32(pres))
        scratch = np.zeros((nlon, nlat), order="F")
        live, out = None, None                       # the distance field the open stream was begun with
        for ts in range(nt):
            tk, vk, uk = step_inputs(ts)
            if live is not dist:
                if live is not None:                  # the ice moved: close the stream, carry the state over
                    out, ws, wd, thc = _ext.stream_end(c2f(sb_all[ts - 1]))
                    _check("stream_end")
                    ws, wd, thc = c2f(ws), c2f(wd), c2f(thc)
                _ext.stream_begin(zf, sdf, c2f(f32(dist)), c2f(f32(ws)), c2f(f32(wd)), c2f(f32(thc)))
                _check("stream_begin")
                live, fresh = dist, True
            prev = scratch if (ts == 0 or fresh) else c2f(sb_all[ts - 1])
            _ext.stream_step(tt, pf, c2f(f32(tk)), c2f(f32(vk)), c2f(f32(uk)), prev, **kwargs)
            _check("stream_step")
            fresh = False
            tt += 1
        out, ws, wd, thc = _ext.stream_end(c2f(sb_all[nt - 1]))
        _check("stream_end")
        out = c2f(out)
        # what the reference returns as "thc" is the t0 plane (ref :244)
        return tt, sb_all, np.array(out[1]), np.array(out[2]), np.array(out[3])

    t0 = thc
    for ts in range(nt):
        tk, vk, uk = step_inputs(ts)
        out = c2f(_diag_kernel(tt, c2f(pres), c2f(z), c2f(std), c2f(tk), c2f(vk), c2f(uk), c2f(dist),
                               c2f(ws), c2f(wd), c2f(thc), **kwargs))
        sb_all[ts] = out[0]
        t0, ws, wd = out[1], out[2], out[3]              # views: the next step reads them where they lie
        tt += 1
    # what the reference returns as "thc" is the t0 plane (ref :244); copies, so that the arrays handed out
    # do not alias the (4-plane) output buffer of the last step
    return tt, sb_all, np.array(t0), np.array(ws), np.array(wd)


def read_nc(fnv, fnu, fntheta, fnci, vv="v", vu="u", vtheta="t2m", vci="ci", vpres="pres", vtime="time"):
    """Open the four NetCDF inputs and return an object usable as ``diag(..., meta=...)``
    (ref: python_wrapper/seabreezediag/__init__.py:53-89): attributes ``u, v, theta, ci`` (the file variables, sliced
    step by step by ``diag``), ``time`` (datetimes), ``pres`` (the level axis), ``dt`` (minutes between the first two
    time slices) and ``nc`` (the open files, for the caller to close).  Files are read through ``ncio`` (netCDF4
    where it can be imported, scipy's classic-format reader otherwise)."""
    from types import SimpleNamespace

    from . import ncio

    files = {"v": fnv, "u": fnu, "theta": fntheta, "ci": fnci}
    varname = {"v": vv, "u": vu, "theta": vtheta, "ci": vci}
    meta = SimpleNamespace(nc={k: ncio.open_dataset(f) for k, f in files.items()})
    for key, ds in meta.nc.items():
        setattr(meta, key, ds.variables[varname[key]])
    tvar = meta.nc["v"].variables[vtime]
    meta.time = ncio.num2date(tvar[:], tvar.units)
    meta.pres = np.array(meta.nc["v"].variables[vpres][:])
    meta.dt = (meta.time[1] - meta.time[0]).seconds / 60.0 if len(meta.time) > 1 else 0.0
    return meta
