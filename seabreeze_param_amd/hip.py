"""ctypes binding of libseabreeze_hip.so (include/seabreeze_hip.h).

This is plumbing only: every numerical result comes from the HIP kernels behind
the C ABI.  There is no CPU fallback -- a missing library or a missing gfx950
device raises.

Arrays: C-contiguous numpy with reversed shape == Fortran (lon, lat[, lev]);
see seabreeze_param_amd/synth.py.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEABREEZE_HIP_LIB", os.path.join(_HERE, "libseabreeze_hip.so"))

SB_BND_WRAPPER, SB_BND_GLOBAL, SB_BND_HALO = 0, 1, 2
SB_UM_THETA_TO_T0, SB_UM_LEVEL_WALK = 1, 2
SB_DIST_MAX_WINDOW = 255            # include/seabreeze_hip.h: the widest get_dist window (kwin, or the derived half-width)
SB_DIST_UM_MAX_WINDOW = 255         # include/seabreeze_hip.h: the widest window of get_dist_um_win, each way
# include/seabreeze_hip.h: the sides of a tile (tile_get_edges_um, tile_get_dist_um) that are the domain's edge
SB_TILE_WEST, SB_TILE_EAST, SB_TILE_SOUTH, SB_TILE_NORTH = 1, 2, 4, 8

_SFX = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
_CT = {np.dtype(np.float32): C.c_float, np.dtype(np.float64): C.c_double}


class SeabreezeHipError(RuntimeError):
    pass


class Tunables(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "target_plev_pa", "thresh_wind", "thresh_winddir", "thresh_windch",
        "thresh_thc", "target_time_s", "maxdist_km")]


_lib = None


def load_library() -> C.CDLL:
    """Load the product library; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SeabreezeHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        _lib = C.CDLL(LIB_PATH)
        _lib.sb_last_error.restype = C.c_char_p
        _lib.sb_last_error.argtypes = [C.c_void_p]
        _lib.sb_version.restype = C.c_char_p
    return _lib


def hip_runtimes():
    """Paths of the HIP runtimes (libamdhip64) mapped into this process.  PyTorch bundles a runtime of its own and
    loads it by path; libseabreeze_hip.so asks for the soname.  So with `import torch` FIRST the library binds to
    torch's copy and the process has ONE runtime -- a torch stream handle is then a valid hipStream_t for the C ABI --
    while with the library loaded first there are TWO, whose streams and synchronisation know nothing of each other (and
    of which, on this pool, only the first to initialise finds the GPU)."""
    seen = []
    try:
        for ln in open("/proc/self/maps"):
            i = ln.find("/")
            path = ln[i:].strip() if i >= 0 else ""
            if "libamdhip64.so" in path and path not in seen:
                seen.append(path)
    except OSError:
        pass
    return seen


def torch_stream_handle(torch):
    """The hipStream_t to hand to the `_dev` entry points from a process that also runs PyTorch: torch's current stream.
    Valid only when torch and the library share ONE HIP runtime, i.e. when torch was imported before the library was
    loaded; with two runtimes in a process only the one that initialises first finds the GPU at all (measured on this
    pool: the other reports no device), so that order is refused here rather than timed wrongly."""
    rts = hip_runtimes()
    if len(rts) != 1:
        raise SeabreezeHipError("torch and libseabreeze_hip.so must share one HIP runtime: import torch BEFORE the library is "
                                f"loaded (mapped runtimes: {rts})")
    return torch.cuda.current_stream().cuda_stream


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(int(a))       # raw device address


def _host(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return a


class Context:
    """One HIP device + stream + workspace (sb_ctx)."""

    def __init__(self, device: int = -1):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.sb_create(C.byref(h), C.c_int(device))
        if rc != 0:
            raise SeabreezeHipError(f"sb_create failed ({rc}): {self.lib.sb_last_error(None).decode()}")
        self.h = h
        self._stream = None          # (dtype, nx, ny) of the stream begun last (stream_begin)
        self._um = None              # (dtype, nx, ny, halo_i, halo_j) of the open UM coast (um_coast_open)
        self._um_tile = None         # the same of the open UM tile coast (um_tile_coast_open)

    def close(self):
        if getattr(self, "h", None):
            self.lib.sb_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise SeabreezeHipError(f"{what} failed ({rc}): {self.lib.sb_last_error(self.h).decode()}")

    def synchronize(self):
        self._chk(self.lib.sb_synchronize(self.h), "sb_synchronize")

    def set_search_radius_hint(self, r: int):
        self._chk(self.lib.sb_set_search_radius_hint(self.h, C.c_int(r)), "sb_set_search_radius_hint")

    def set_fold(self, on: bool):
        """k_prep's work inside the contrast kernel (default) or as a kernel of its own (measurement / test knob)."""
        self._chk(self.lib.sb_set_fold(self.h, C.c_int(1 if on else 0)), "sb_set_fold")

    def set_plan_cache(self, on: bool):
        """The strip kernel keeps its plan while the band plane stands (default) or plans every call (measurement / test knob)."""
        self._chk(self.lib.sb_set_plan_cache(self.h, C.c_int(1 if on else 0)), "sb_set_plan_cache")

    def set_wide_strip(self, on: bool):
        """Radii beyond 16 in single precision: the 96-column strip kernel (default) or the tile kernel (test knob)."""
        self._chk(self.lib.sb_set_wide_strip(self.h, C.c_int(1 if on else 0)), "sb_set_wide_strip")

    def set_workgroups(self, n: int):
        """Persistent workgroups of the one-per-CU kernels (0: the device's compute units); a test knob."""
        self._chk(self.lib.sb_set_workgroups(self.h, C.c_int(int(n))), "sb_set_workgroups")

    def set_band_order(self, contrast_first: bool):
        """A band step runs k_scan, k_wind | join | contrast (default) or k_scan | join | contrast, k_wind (measurement knob)."""
        self._chk(self.lib.sb_set_band_order(self.h, C.c_int(1 if contrast_first else 0)), "sb_set_band_order")

    def set_wind_pairs(self, on: bool):
        """k_wind walks two cells and two levels per 16-byte load where the call allows it (default) or one everywhere (measurement / test knob)."""
        self._chk(self.lib.sb_set_wind_pairs(self.h, C.c_int(1 if on else 0)), "sb_set_wind_pairs")

    def last_wind_pairs(self) -> int:
        """1: the last diag call's k_wind was the paired instance; 0: it was not."""
        ran = C.c_int(0)
        self._chk(self.lib.sb_last_wind_pairs(self.h, C.byref(ran)), "sb_last_wind_pairs")
        return ran.value

    def set_static_sigma(self, on: bool):
        """Opt-in: sigma does not change between calls; its statistics are formed once (include/seabreeze_hip.h)."""
        self._chk(self.lib.sb_set_static_sigma(self.h, C.c_int(1 if on else 0)), "sb_set_static_sigma")

    def set_table_contrast(self, on: bool):
        """Opt-in: whole single-domain host-model calls take the contrast from device-wide summed-area tables, radii up
        to 127 at a cost that does not depend on the radius (include/seabreeze_hip.h)."""
        self._chk(self.lib.sb_set_table_contrast(self.h, C.c_int(1 if on else 0)), "sb_set_table_contrast")

    def set_table_contrast_bands(self, on: bool):
        """Opt-in, with set_table_contrast: band steps and diag calls with gathered moments take the table contrast too;
        the ghost width must cover the largest radius (include/seabreeze_hip.h)."""
        self._chk(self.lib.sb_set_table_contrast_bands(self.h, C.c_int(1 if on else 0)), "sb_set_table_contrast_bands")

    def set_table_contrast_f2py(self, on: bool):
        """Opt-in, with set_table_contrast: whole calls of the f2py flavour (diag, stream steps) take the table contrast
        too -- six launches, the wrapper's column rule by tables over the effective row (include/seabreeze_hip.h)."""
        self._chk(self.lib.sb_set_table_contrast_f2py(self.h, C.c_int(1 if on else 0)), "sb_set_table_contrast_f2py")

    def set_table_window_cache(self, on: bool):
        """Opt-in, with set_table_contrast: a table call keeps every band cell's window while the coast stands; the same
        bits, less work per call (include/seabreeze_hip.h)."""
        self._chk(self.lib.sb_set_table_window_cache(self.h, C.c_int(1 if on else 0)), "sb_set_table_window_cache")

    def table_cache_report(self):
        """Band cells of the last diag call answered from stored windows / searched; calls that searched / ran with the
        cache in effect since it was switched on."""
        arr = (C.c_longlong * 4)()
        self._chk(self.lib.sb_table_cache_report(self.h, arr), "sb_table_cache_report")
        return dict(stored_cells=arr[0], searched_cells=arr[1], fills=arr[2], calls=arr[3])

    def set_nonfinite_guard(self, on: bool):
        """Opt-in: whole diag calls find NaN, Inf and missing (2e20) temperatures and compute the band cells whose windows
        hold them again as the reference does, between the contrast kernel and k_wind (include/seabreeze_hip.h)."""
        self._chk(self.lib.sb_set_nonfinite_guard(self.h, C.c_int(1 if on else 0)), "sb_set_nonfinite_guard")

    def set_nonfinite_guard_bands(self, on: bool):
        """Opt-in, with set_nonfinite_guard: band steps and host-model diag calls with gathered moments are guarded too --
        the taint is found ahead of the contrast kernel, ws / wd of the tainted cells are put aside and the update is
        applied again behind it; theta gets the whole swap_bounds in a band step (include/seabreeze_hip.h)."""
        self._chk(self.lib.sb_set_nonfinite_guard_bands(self.h, C.c_int(1 if on else 0)), "sb_set_nonfinite_guard_bands")

    def guard_report(self):
        """Bad frame cells the last diag call found / band cells it computed again; calls that found a bad cell / ran with
        the guard in effect since the switch was last set.  All 0 after a call the guard did not serve."""
        arr = (C.c_longlong * 4)()
        self._chk(self.lib.sb_guard_report(self.h, arr), "sb_guard_report")
        return dict(bad_cells=arr[0], repaired_cells=arr[1], calls_with_bad=arr[2], calls=arr[3])

    def last_step_report(self):
        """What the last diag call / band step enqueued on this rank."""
        arr = (C.c_int * 4)()
        self._chk(self.lib.sb_last_step_report(self.h, arr), "sb_last_step_report")
        return dict(kernel_launches=arr[0], rccl_ops=arr[1], rccl_groups=arr[2], d2d_copies=arr[3])

    def last_counters(self):
        arr = (C.c_longlong * 4)()
        self._chk(self.lib.sb_last_counters(self.h, arr), "sb_last_counters")
        return dict(band_cells=arr[0], global_path_cells=arr[1], one_class_cells=arr[2], max_radius=arr[3])

    def profile_begin(self, max_calls: int):
        self._chk(self.lib.sb_profile_begin(self.h, C.c_int(max_calls)), "sb_profile_begin")

    def profile_end(self):
        """-> ({'k_scan', 'k_wind', 'k_t0', 'k_thc', 'k_prep'} -> ms, ncalls): HIP-event averages of the
        launches of one diag call.  k_thc is k_thc3 (t0, tables, search); k_t0 exists for the f2py flavour
        only (0.0 where a call does not launch it); k_prep is the list / statistics kernel after k_scan."""
        ms = (C.c_double * 5)()
        n = C.c_int(0)
        self._chk(self.lib.sb_profile_end(self.h, ms, C.byref(n)), "sb_profile_end")
        return dict(k_scan=ms[0], k_wind=ms[1], k_t0=ms[2], k_thc=ms[3], k_prep=ms[4]), n.value

    # ------------------------------------------------------------------ host-pointer API
    def seabreeze_diag(self, timestep, tn, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con,
                       halo=0, bnd=SB_BND_GLOBAL, tunables: Tunables | None = None):
        """generic/sea_breeze_diag.f90:55 semantics; ws, wd, thc, sb_con updated in place."""
        dt = np.dtype(ws.dtype)
        sfx, ct = _SFX[dt], _CT[dt]
        p = _host(p, dt); u = _host(u, dt); v = _host(v, dt)
        theta = _host(theta, dt); mask = _host(mask, dt); z = _host(z, dt); sigma = _host(sigma, dt)
        nz, ny, nx = p.shape
        for a in (theta, mask, z, sigma):
            if a.shape != (ny + 2 * halo, nx + 2 * halo):
                raise ValueError(f"2-D input shape {a.shape} != {(ny + 2 * halo, nx + 2 * halo)}")
        for a in (ws, wd, thc, sb_con):
            if a.shape != (ny, nx) or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("state arrays must be C-contiguous (ny, nx) of the working dtype")
        fn = getattr(self.lib, f"sb_seabreeze_diag_{sfx}")
        rc = fn(self.h, ct(timestep), C.c_int(tn), C.c_int(nx), C.c_int(ny), C.c_int(nz), C.c_int(halo),
                C.c_int(bnd), _p(p), _p(u), _p(v), _p(theta), _p(mask), _p(z), _p(sigma),
                _p(ws), _p(wd), _p(thc), _p(sb_con), C.byref(tunables) if tunables is not None else None)
        self._chk(rc, "sb_seabreeze_diag")
        return sb_con

    def seabreeze_diag_um(self, timestep, tn, p, u, v, theta, z, sigma, mask, ws, wd, thc, sb_con,
                          halo_s, halo_l, flags=0):
        """UM vn10.7 layout and argument order (UM/vn10.7/sea_breeze_diag.F90:55-117): theta, z, sigma carry halo_s
        ghost cells, mask halo_l >= halo_s; theta is overwritten with t0 under SB_UM_THETA_TO_T0.  Returns `error`."""
        dt = np.dtype(ws.dtype)
        sfx, ct = _SFX[dt], _CT[dt]
        p = _host(p, dt); u = _host(u, dt); v = _host(v, dt)
        z = _host(z, dt); sigma = _host(sigma, dt); mask = _host(mask, dt)
        if theta.dtype != dt or not theta.flags.c_contiguous:
            raise ValueError("theta must be a C-contiguous array of the working dtype (it may be overwritten)")
        nz, ny, nx = p.shape if p.ndim == 3 else (0, 0, 0)
        err = C.c_int(0)
        fn = getattr(self.lib, f"sb_seabreeze_diag_um_{sfx}")
        rc = fn(self.h, ct(timestep), C.c_int(tn), C.c_int(nx), C.c_int(ny), C.c_int(nz), C.c_int(halo_s), C.c_int(halo_l),
                _p(p), _p(u), _p(v), _p(theta), _p(z), _p(sigma), _p(mask), _p(ws), _p(wd), _p(thc), _p(sb_con),
                C.c_int(flags), C.byref(err))
        self._chk(rc, "sb_seabreeze_diag_um")
        return err.value

    def diag(self, tn, p, z, std, theta, v, u, cdist, ws, wd, thc, output=None,
             target_plev=700.0, thresh_wind=11.0, thresh_winddir=90.0, thresh_windch=5.0,
             thresh_thc=0.75, target_time=6.0, maxdist=180.0, timestep=24.0):
        """seabreeze_diag_python.f90:49 semantics; ws, wd, thc updated in place; returns output(4, ny, nx)."""
        dt = np.dtype(ws.dtype)
        sfx, ct = _SFX[dt], _CT[dt]
        p = _host(p, dt); z = _host(z, dt); std = _host(std, dt); theta = _host(theta, dt)
        v = _host(v, dt); u = _host(u, dt); cdist = _host(cdist, dt)
        nps = p.shape[0]
        ny, nx = z.shape
        if u.shape != (nps, ny, nx) or v.shape != (nps, ny, nx):
            raise ValueError("u, v must be (nps, ny, nx)")
        if output is None:
            output = np.zeros((4, ny, nx), dtype=dt)
        fn = getattr(self.lib, f"sb_diag_{sfx}")
        rc = fn(self.h, C.c_int(tn), _p(p), _p(z), _p(std), _p(theta), _p(v), _p(u), _p(cdist),
                _p(ws), _p(wd), _p(thc), ct(target_plev), ct(thresh_wind), ct(thresh_winddir),
                ct(thresh_windch), ct(thresh_thc), ct(target_time), ct(maxdist), ct(timestep),
                C.c_int(nps), C.c_int(nx), C.c_int(ny), _p(output))
        self._chk(rc, "sb_diag")
        return output

    # ------------------------------------------------------------------ the streamed f2py flavour (sb_diag_stream_*)
    # Planes are C-ordered (ny, nx) arrays of one working dtype (that of `z`); the stream keeps that dtype.
    def _stream_shape(self):
        if self._stream is None:
            raise SeabreezeHipError("no stream: call stream_begin first")
        return self._stream

    def stream_begin(self, z, std, cdist, ws, wd, thc):
        """z, std, cdist and the carried state go to the device and stay there until stream_end."""
        z = np.ascontiguousarray(z)
        dt = np.dtype(z.dtype)
        ny, nx = z.shape
        std, cdist, ws, wd, thc = (_host(a, dt) for a in (std, cdist, ws, wd, thc))
        fn = getattr(self.lib, f"sb_diag_stream_begin_{_SFX[dt]}")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), _p(z), _p(std), _p(cdist), _p(ws), _p(wd), _p(thc)), "sb_diag_stream_begin")
        self._stream = (dt, nx, ny)

    def stream_step(self, tn, p, theta, v, u, sb_con_prev=None, target_plev=700.0, thresh_wind=11.0, thresh_winddir=90.0,
                    thresh_windch=5.0, thresh_thc=0.75, target_time=6.0, maxdist=180.0, timestep=24.0):
        """One step; sb_con of the step before lands in rows 0 .. ny-2 of sb_con_prev (float64 (ny, nx)).  Returns whether
        it did."""
        dt, nx, ny = self._stream_shape()
        ct = _CT[dt]
        p = _host(p, dt); theta = _host(theta, dt); v = _host(v, dt); u = _host(u, dt)
        if sb_con_prev is not None and not (sb_con_prev.dtype == np.float64 and sb_con_prev.flags.c_contiguous):
            raise ValueError("sb_con_prev must be a C-contiguous float64 array")
        have = C.c_int(0)
        fn = getattr(self.lib, f"sb_diag_stream_step_{_SFX[dt]}")
        rc = fn(self.h, C.c_int(tn), _p(p), C.c_int(p.shape[0]), _p(theta), _p(v), _p(u), ct(target_plev), ct(thresh_wind),
                ct(thresh_winddir), ct(thresh_windch), ct(thresh_thc), ct(target_time), ct(maxdist), ct(timestep),
                _p(sb_con_prev), C.byref(have))
        self._chk(rc, "sb_diag_stream_step")
        return bool(have.value)

    def stream_end(self):
        """-> (output (4, ny, nx) of the last step, ws, wd, thc)."""
        dt, nx, ny = self._stream_shape()
        out = np.zeros((4, ny, nx), dt)
        ws, wd, thc = (np.zeros((ny, nx), dt) for _ in range(3))
        fn = getattr(self.lib, f"sb_diag_stream_end_{_SFX[dt]}")
        self._chk(fn(self.h, None, _p(out), _p(ws), _p(wd), _p(thc)), "sb_diag_stream_end")
        return out, ws, wd, thc

    def stream_coast(self, lsm, lon, lat, maxdist=180.0, incremental=True, dtype=None):
        """Opt-in, between stream_begin and the first step: the stream's coast follows the sea ice on the device
        (include/seabreeze_hip.h: sb_diag_stream_coast).  dtype: the precision of the call (default: the stream's)."""
        dt = np.dtype(dtype) if dtype is not None else self._stream_shape()[0]
        lsm = _host(lsm, dt); lon = _host(lon, dt); lat = _host(lat, dt)
        fn = getattr(self.lib, f"sb_diag_stream_coast_{_SFX[dt]}")
        self._chk(fn(self.h, _p(lsm), _p(lon), _p(lat), _CT[dt](maxdist), C.c_int(1 if incremental else 0)), "sb_diag_stream_coast")

    def stream_ice(self, ci, dtype=None):
        """Enqueue the coast and distance update of the stream's resident cdist for this ice plane; no synchronisation."""
        dt = np.dtype(dtype) if dtype is not None else self._stream_shape()[0]
        ci = _host(ci, dt)
        self._chk(getattr(self.lib, f"sb_diag_stream_ice_{_SFX[dt]}")(self.h, _p(ci)), "sb_diag_stream_ice")

    def stream_ice_report(self):
        """Ice calls of the stream / those after the first whose coast differed (-1 on the whole-grid path) / (row, tile)
        pairs the last call marked / pairs of the grid.  Synchronises."""
        arr = (C.c_longlong * 4)()
        self._chk(self.lib.sb_diag_stream_ice_report(self.h, arr), "sb_diag_stream_ice_report")
        return dict(calls=arr[0], changed_calls=arr[1], tiles_marked=arr[2], tiles=arr[3])

    def stream_ice_time(self):
        """HIP-event time [ms] of the last ice call's device work (upload, clear, kernels).  Waits for it."""
        ms = C.c_double(0.0)
        self._chk(self.lib.sb_diag_stream_ice_time(self.h, C.byref(ms)), "sb_diag_stream_ice_time")
        return ms.value

    def stream_get_cdist(self):
        """The stream's resident distance plane (ny, nx).  Synchronises."""
        dt, nx, ny = self._stream_shape()
        out = np.empty((ny, nx), dt)
        self._chk(getattr(self.lib, f"sb_diag_stream_get_cdist_{_SFX[dt]}")(self.h, _p(out)), "sb_diag_stream_get_cdist")
        return out

    def sigmoid(self, ary):
        ary = np.ascontiguousarray(ary)
        dt = np.dtype(ary.dtype)
        ny, nx = ary.shape
        sm = np.empty_like(ary)
        rc = getattr(self.lib, f"sb_sigmoid_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), _p(ary), _p(sm))
        self._chk(rc, "sb_sigmoid")
        return sm

    def get_edges(self, lsm, ci, rule=0, bnd=SB_BND_WRAPPER):
        lsm = np.ascontiguousarray(lsm)
        dt = np.dtype(lsm.dtype)
        ci = _host(ci, dt)
        ny, nx = lsm.shape
        coast = np.empty_like(lsm)
        rc = getattr(self.lib, f"sb_get_edges_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), _p(lsm), _p(ci),
                                                          C.c_int(rule), C.c_int(bnd), _p(coast))
        self._chk(rc, "sb_get_edges")
        return coast

    def get_dist(self, coast, mask, lon, lat, maxdist=180.0, kwin=-1):
        """Signed coast distance (km); kwin < 0 derives the window from the grid spacing (dist_window).  The window may
        reach SB_DIST_MAX_WINDOW cells each way; on km-scale grids use float64 (see include/seabreeze_hip.h)."""
        coast = np.ascontiguousarray(coast)
        dt = np.dtype(coast.dtype)
        mask = _host(mask, dt); lon = _host(lon, dt); lat = _host(lat, dt)
        ny, nx = coast.shape
        cdist = np.empty_like(coast)
        rc = getattr(self.lib, f"sb_get_dist_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), _p(coast), _p(mask),
                                                         _p(lon), _p(lat), _CT[dt](maxdist), C.c_int(kwin),
                                                         _p(cdist))
        self._chk(rc, "sb_get_dist")
        return cdist

    def get_edges_um(self, landfrac_l, icefrac_l, halo_i, halo_j, out=None):
        """UM vn10.7 get_edges(mask, icefrac, landfrac) on the tdims_l layout: landfrac_l, icefrac_l are
        (ny + 2*halo_j, nx + 2*halo_i) with their ghost cells filled; returns coast of that shape with 0/1 in the
        interior.  Its ghost cells are those of `out` (zeros without it): they are not touched."""
        landfrac_l = np.ascontiguousarray(landfrac_l)
        dt = np.dtype(landfrac_l.dtype)
        icefrac_l = _host(icefrac_l, dt)
        ny, nx = landfrac_l.shape[0] - 2 * halo_j, landfrac_l.shape[1] - 2 * halo_i
        if icefrac_l.shape != landfrac_l.shape:
            raise ValueError("landfrac_l and icefrac_l must have the same shape")
        coast = np.zeros_like(landfrac_l) if out is None else out
        if coast.shape != landfrac_l.shape or coast.dtype != dt or not coast.flags.c_contiguous:
            raise ValueError("out must be C-contiguous, of the input's shape and dtype")
        rc = getattr(self.lib, f"sb_get_edges_um_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i),
                                                             C.c_int(halo_j), _p(landfrac_l), _p(icefrac_l), _p(coast))
        self._chk(rc, "sb_get_edges_um")
        return coast

    def get_dist_um(self, coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, maxdist=180.0, out=None):
        """UM vn10.7 get_dist(landfrac, coast): coast_l (ny + 2*halo_j, nx + 2*halo_i), landfrac and the 2-D
        coordinates true_lat, true_lon (degrees) (ny, nx).  Returns the signed coast distance on coast_l's layout:
        the interior is written, the ghost cells are those of `out` (zeros without it).  out may be coast_l itself."""
        coast_l = np.ascontiguousarray(coast_l)
        dt = np.dtype(coast_l.dtype)
        landfrac = _host(landfrac, dt); true_lat = _host(true_lat, dt); true_lon = _host(true_lon, dt)
        ny, nx = landfrac.shape
        if coast_l.shape != (ny + 2 * halo_j, nx + 2 * halo_i):
            raise ValueError(f"coast_l shape {coast_l.shape} != {(ny + 2 * halo_j, nx + 2 * halo_i)}")
        if true_lat.shape != (ny, nx) or true_lon.shape != (ny, nx):
            raise ValueError("true_lat, true_lon must be (ny, nx) like landfrac")
        cdist = np.zeros_like(coast_l) if out is None else out
        if cdist.shape != coast_l.shape or cdist.dtype != dt or not cdist.flags.c_contiguous:
            raise ValueError("out must be C-contiguous, of coast_l's shape and dtype")
        rc = getattr(self.lib, f"sb_get_dist_um_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i),
                                                            C.c_int(halo_j), _p(coast_l), _p(landfrac), _p(true_lat),
                                                            _p(true_lon), _CT[dt](maxdist), _p(cdist))
        self._chk(rc, "sb_get_dist_um")
        return cdist

    def get_dist_um_win(self, coast_l, landfrac, true_lat, true_lon, halo_i, halo_j, win_i, win_j, maxdist=180.0,
                        out=None):
        """get_dist_um with the window stated apart from the layout: +-win_i columns x +-win_j rows, each 0 ..
        SB_DIST_UM_MAX_WINDOW, wider or narrower than the ghost width; halo_i, halo_j >= 0 only say where the interior of
        coast_l (ny + 2*halo_j, nx + 2*halo_i) lies.  Shapes, `out` and the result are get_dist_um's."""
        coast_l = np.ascontiguousarray(coast_l)
        dt = np.dtype(coast_l.dtype)
        landfrac = _host(landfrac, dt); true_lat = _host(true_lat, dt); true_lon = _host(true_lon, dt)
        ny, nx = landfrac.shape
        if halo_i < 0 or halo_j < 0 or coast_l.shape != (ny + 2 * halo_j, nx + 2 * halo_i):
            raise ValueError(f"coast_l shape {coast_l.shape} != {(ny + 2 * halo_j, nx + 2 * halo_i)}")
        if true_lat.shape != (ny, nx) or true_lon.shape != (ny, nx):
            raise ValueError("true_lat, true_lon must be (ny, nx) like landfrac")
        cdist = np.zeros_like(coast_l) if out is None else out
        if cdist.shape != coast_l.shape or cdist.dtype != dt or not cdist.flags.c_contiguous:
            raise ValueError("out must be C-contiguous, of coast_l's shape and dtype")
        rc = getattr(self.lib, f"sb_get_dist_um_win_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i),
                                                                C.c_int(halo_j), C.c_int(win_i), C.c_int(win_j),
                                                                _p(coast_l), _p(landfrac), _p(true_lat), _p(true_lon),
                                                                _CT[dt](maxdist), _p(cdist))
        self._chk(rc, "sb_get_dist_um_win")
        return cdist

    def tile_get_edges_um(self, landfrac_l, icefrac_l, halo_i, halo_j, ext_i, ext_j, sides, out=None):
        """get_edges_um for one tile of a 2-D domain decomposition (include/seabreeze_hip.h: sb_tile_get_edges_um):
        landfrac_l, icefrac_l are the tile's frames (ny + 2*halo_j, nx + 2*halo_i), ghost cells filled; sides is a sum of
        SB_TILE_* (a set bit: that side is the domain's edge).  Returns coast on that frame with 0/1 in the interior and in
        the ghost cells within ext_i columns / ext_j rows of it on every cut side (halo >= ext + 1 there); every other cell
        is that of `out` (zeros without it)."""
        landfrac_l = np.ascontiguousarray(landfrac_l)
        dt = np.dtype(landfrac_l.dtype)
        icefrac_l = _host(icefrac_l, dt)
        ny, nx = landfrac_l.shape[0] - 2 * halo_j, landfrac_l.shape[1] - 2 * halo_i
        if icefrac_l.shape != landfrac_l.shape:
            raise ValueError("landfrac_l and icefrac_l must have the same shape")
        coast = np.zeros_like(landfrac_l) if out is None else out
        if coast.shape != landfrac_l.shape or coast.dtype != dt or not coast.flags.c_contiguous:
            raise ValueError("out must be C-contiguous, of the input's shape and dtype")
        rc = getattr(self.lib, f"sb_tile_get_edges_um_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i),
                                                                  C.c_int(halo_j), C.c_int(ext_i), C.c_int(ext_j),
                                                                  C.c_int(sides), _p(landfrac_l), _p(icefrac_l), _p(coast))
        self._chk(rc, "sb_tile_get_edges_um")
        return coast

    def tile_get_dist_um(self, coast_l, landfrac_l, true_lat_l, true_lon_l, halo_i, halo_j, win_i, win_j, sides,
                         maxdist=180.0, out=None):
        """get_dist_um_win for one tile of a 2-D domain decomposition (include/seabreeze_hip.h: sb_tile_get_dist_um): every
        field is the tile's frame (ny + 2*halo_j, nx + 2*halo_i), the coordinates included; sources are the coast cells of
        the interior and of the ghost cells within the window on every cut side (halo >= win there).  Returns the signed
        distance on the frame: the interior is written -- the tile's cells of the whole-domain field -- the ghost cells are
        those of `out` (zeros without it).  out may be coast_l itself."""
        coast_l = np.ascontiguousarray(coast_l)
        dt = np.dtype(coast_l.dtype)
        landfrac_l = _host(landfrac_l, dt); true_lat_l = _host(true_lat_l, dt); true_lon_l = _host(true_lon_l, dt)
        ny, nx = coast_l.shape[0] - 2 * halo_j, coast_l.shape[1] - 2 * halo_i
        if halo_i < 0 or halo_j < 0 or any(a.shape != coast_l.shape for a in (landfrac_l, true_lat_l, true_lon_l)):
            raise ValueError("landfrac_l, true_lat_l, true_lon_l must be frames of coast_l's shape")
        cdist = np.zeros_like(coast_l) if out is None else out
        if cdist.shape != coast_l.shape or cdist.dtype != dt or not cdist.flags.c_contiguous:
            raise ValueError("out must be C-contiguous, of coast_l's shape and dtype")
        rc = getattr(self.lib, f"sb_tile_get_dist_um_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i),
                                                                 C.c_int(halo_j), C.c_int(win_i), C.c_int(win_j),
                                                                 C.c_int(sides), _p(coast_l), _p(landfrac_l), _p(true_lat_l),
                                                                 _p(true_lon_l), _CT[dt](maxdist), _p(cdist))
        self._chk(rc, "sb_tile_get_dist_um")
        return cdist

    def band_get_edges(self, lsm_f, ci_f, halo, south, north, rule=1, out=None):
        """get_edges(rule, SB_BND_GLOBAL) for one latitude band in the band step's frame: lsm_f, ci_f are
        (ny + 2*halo, nx + 2*halo) with the ghost row next to the interior filled on every cut side (south / north False);
        ghost rows on a pole side and the east-west ghost columns are never read.  Returns coast on that frame with 0/1 in
        the interior, the whole-grid call's bits; the ghost cells are those of `out` (zeros without it)."""
        lsm_f = np.ascontiguousarray(lsm_f)
        dt = np.dtype(lsm_f.dtype)
        ci_f = _host(ci_f, dt)
        ny, nx = lsm_f.shape[0] - 2 * halo, lsm_f.shape[1] - 2 * halo
        if ci_f.shape != lsm_f.shape:
            raise ValueError("lsm_f and ci_f must have the same shape")
        coast = np.zeros_like(lsm_f) if out is None else out
        if coast.shape != lsm_f.shape or coast.dtype != dt or not coast.flags.c_contiguous:
            raise ValueError("out must be C-contiguous, of the input's shape and dtype")
        rc = getattr(self.lib, f"sb_band_get_edges_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo),
                                                               C.c_int(1 if south else 0), C.c_int(1 if north else 0),
                                                               _p(lsm_f), _p(ci_f), C.c_int(rule), _p(coast))
        self._chk(rc, "sb_band_get_edges")
        return coast

    def band_get_dist(self, coast_f, mask_f, lon, lat_f, halo, south, north, kwin, maxdist=180.0, out=None):
        """get_dist(kwin) for one latitude band in the band step's frame: coast_f, mask_f (ny + 2*halo, nx + 2*halo), lon
        (nx), lat_f (ny + 2*halo: one latitude per frame row).  kwin ghost rows of coast_f are read on every cut side
        (kwin <= halo there), none on a pole side.  Returns the signed distance on the frame, the interior being the
        whole-grid call's bits; the ghost cells are those of `out` (zeros without it)."""
        coast_f = np.ascontiguousarray(coast_f)
        dt = np.dtype(coast_f.dtype)
        mask_f = _host(mask_f, dt); lon = _host(lon, dt); lat_f = _host(lat_f, dt)
        ny, nx = coast_f.shape[0] - 2 * halo, coast_f.shape[1] - 2 * halo
        if mask_f.shape != coast_f.shape or lon.shape != (nx,) or lat_f.shape != (ny + 2 * halo,):
            raise ValueError("mask_f must have coast_f's shape, lon nx entries, lat_f ny + 2*halo")
        cdist = np.zeros_like(coast_f) if out is None else out
        if cdist.shape != coast_f.shape or cdist.dtype != dt or not cdist.flags.c_contiguous:
            raise ValueError("out must be C-contiguous, of coast_f's shape and dtype")
        rc = getattr(self.lib, f"sb_band_get_dist_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo),
                                                              C.c_int(1 if south else 0), C.c_int(1 if north else 0),
                                                              _p(coast_f), _p(mask_f), _p(lon), _p(lat_f), _CT[dt](maxdist),
                                                              C.c_int(kwin), _p(cdist))
        self._chk(rc, "sb_band_get_dist")
        return cdist

    def _search_radius(self, fn_name, mask, maxdist, halo, nhist, lead):
        mask = np.ascontiguousarray(mask)
        dt = np.dtype(mask.dtype)
        if dt not in _SFX or mask.ndim != 2:
            raise ValueError("mask must be a 2-D float32 or float64 array")
        ny, nx = mask.shape[0] - 2 * halo, mask.shape[1] - 2 * halo
        radius = np.empty((max(ny, 0), max(nx, 0)), dtype=np.int32)
        summary = (C.c_longlong * 4)()
        hist = np.zeros(nhist, dtype=np.int64) if nhist else None
        rc = getattr(self.lib, f"{fn_name}_{_SFX[dt]}")(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo), *lead, _p(mask),
                                                       _CT[dt](maxdist), _p(radius), summary, _p(hist), C.c_int(nhist))
        self._chk(rc, fn_name)
        return radius, dict(band_cells=summary[0], with_radius=summary[1], without_window=summary[2],
                            max_radius=summary[3]), hist

    def search_radius(self, mask, maxdist=180.0, halo=0, bnd=SB_BND_GLOBAL, nhist=0):
        """Every band cell's window radius from mask alone, before any diag call: mask is (ny + 2*halo, nx + 2*halo), halo 0
        unless bnd is SB_BND_HALO.  Returns (radius (ny, nx) int32: 0 off the band, nn >= 1, -1 where the window never holds
        both classes within the diag call's cap; summary: band_cells, with_radius, without_window, max_radius -- what
        last_counters() would say after a diag call; hist (nhist bins: [0] the -1 cells, [k] radius k, the last bin radius
        >= nhist - 1) or None).  No effect on what a later diag call enqueues or returns."""
        return self._search_radius("sb_search_radius", mask, maxdist, halo, nhist, (C.c_int(bnd),))

    def band_search_radius(self, mask_f, halo, south, north, maxdist=180.0, nhist=0):
        """search_radius for one latitude band in the band step's frame: mask_f (ny + 2*halo, nx + 2*halo) with its ghost
        rows filled on every cut side (south / north False); ghost rows on a pole side and the east-west ghost columns are
        never read.  A window may use the ghost rows and no more: with halo >= the whole grid's max_radius the interior is
        the whole-grid SB_BND_GLOBAL plane's rows, with less the cells that need more come back -1."""
        return self._search_radius("sb_band_search_radius", mask_f, maxdist, halo, nhist,
                                   (C.c_int(1 if south else 0), C.c_int(1 if north else 0)))

    # ------------------------------------------------------------------ device-pointer API
    def search_radius_dev(self, dtype, nx, ny, halo, bnd, mask, radius, summary, hist=None, nhist=0, maxdist=180.0,
                          stream=None):
        """search_radius on device arrays (raw addresses): radius (ny, nx) int32, summary 4 int64, hist nhist int64, any of
        the three None; zeroes summary and hist on the stream and enqueues without synchronising."""
        dt = np.dtype(dtype)
        fn = getattr(self.lib, f"sb_search_radius_{_SFX[dt]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo), C.c_int(bnd), _p(mask), _CT[dt](maxdist), _p(radius),
                     _p(summary), _p(hist), C.c_int(nhist), C.c_void_p(stream) if stream else None), "sb_search_radius_dev")

    def band_search_radius_dev(self, dtype, nx, ny, halo, south, north, mask_f, radius, summary, hist=None, nhist=0,
                               maxdist=180.0, stream=None):
        """band_search_radius on a device frame (raw addresses); enqueues without synchronising."""
        dt = np.dtype(dtype)
        fn = getattr(self.lib, f"sb_band_search_radius_{_SFX[dt]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo), C.c_int(1 if south else 0), C.c_int(1 if north else 0),
                     _p(mask_f), _CT[dt](maxdist), _p(radius), _p(summary), _p(hist), C.c_int(nhist),
                     C.c_void_p(stream) if stream else None), "sb_band_search_radius_dev")

    def sigmoid_dev(self, dtype, nx, ny, ary, sm, stream=None):
        """sm = 1/(1+exp(-std*(ary-r))) on device arrays (raw addresses); enqueues without synchronising."""
        fn = getattr(self.lib, f"sb_sigmoid_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), _p(ary), _p(sm), C.c_void_p(stream) if stream else None), "sb_sigmoid_dev")

    def seabreeze_diag_dev(self, dtype, timestep, tn, nx, ny, nz, halo, bnd, p, u, v, theta, mask, z, sigma,
                           ws, wd, thc, sb_con, stream=None, tunables: Tunables | None = None):
        """All array arguments are raw device addresses (ints); enqueues without synchronising."""
        dt = np.dtype(dtype)
        fn = getattr(self.lib, f"sb_seabreeze_diag_{_SFX[dt]}_dev")
        rc = fn(self.h, _CT[dt](timestep), C.c_int(tn), C.c_int(nx), C.c_int(ny), C.c_int(nz), C.c_int(halo),
                C.c_int(bnd), _p(p), _p(u), _p(v), _p(theta), _p(mask), _p(z), _p(sigma), _p(ws), _p(wd),
                _p(thc), _p(sb_con), C.byref(tunables) if tunables is not None else None,
                C.c_void_p(stream) if stream else None)
        self._chk(rc, "sb_seabreeze_diag_dev")

    def diag_dev(self, dtype, tn, nps, nx, ny, p, z, std, theta, v, u, cdist, ws, wd, thc, output, stream=None,
                 target_plev=700.0, thresh_wind=11.0, thresh_winddir=90.0, thresh_windch=5.0,
                 thresh_thc=0.75, target_time=6.0, maxdist=180.0, timestep=24.0):
        """The f2py flavour (sb_diag_*_dev) on device arrays (raw addresses); output is (4, ny, nx), of which the kernels
        write rows 1 .. ny - 1 of every plane; enqueues without synchronising."""
        dt = np.dtype(dtype)
        ct = _CT[dt]
        fn = getattr(self.lib, f"sb_diag_{_SFX[dt]}_dev")
        rc = fn(self.h, C.c_int(tn), _p(p), _p(z), _p(std), _p(theta), _p(v), _p(u), _p(cdist), _p(ws), _p(wd), _p(thc),
                ct(target_plev), ct(thresh_wind), ct(thresh_winddir), ct(thresh_windch), ct(thresh_thc), ct(target_time),
                ct(maxdist), ct(timestep), C.c_int(nps), C.c_int(nx), C.c_int(ny), _p(output),
                C.c_void_p(stream) if stream else None)
        self._chk(rc, "sb_diag_dev")


    def get_edges_dev(self, dtype, nx, ny, lsm, ci, coast, rule=0, bnd=SB_BND_WRAPPER, stream=None):
        """get_edges on device arrays (raw addresses); enqueues without synchronising."""
        fn = getattr(self.lib, f"sb_get_edges_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), _p(lsm), _p(ci), C.c_int(rule), C.c_int(bnd), _p(coast),
                     C.c_void_p(stream) if stream else None), "sb_get_edges_dev")

    def get_dist_dev(self, dtype, nx, ny, coast, mask, lon, lat, cdist, maxdist=180.0, kwin=-1, stream=None):
        """get_dist on device arrays (raw addresses); lon, lat are host vectors."""
        dt = np.dtype(dtype)
        lon = _host(lon, dt); lat = _host(lat, dt)
        fn = getattr(self.lib, f"sb_get_dist_{_SFX[dt]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), _p(coast), _p(mask), _p(lon), _p(lat), _CT[dt](maxdist),
                     C.c_int(kwin), _p(cdist), C.c_void_p(stream) if stream else None), "sb_get_dist_dev")

    def band_get_edges_dev(self, dtype, nx, ny, halo, south, north, lsm_f, ci_f, coast_f, rule=1, stream=None):
        """band_get_edges on device frames (raw addresses); enqueues without synchronising."""
        fn = getattr(self.lib, f"sb_band_get_edges_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo), C.c_int(1 if south else 0), C.c_int(1 if north else 0),
                     _p(lsm_f), _p(ci_f), C.c_int(rule), _p(coast_f), C.c_void_p(stream) if stream else None),
                  "sb_band_get_edges_dev")

    def band_get_dist_dev(self, dtype, nx, ny, halo, south, north, coast_f, mask_f, lon, lat_f, cdist_f, kwin,
                          maxdist=180.0, stream=None):
        """band_get_dist on device frames (raw addresses); lon (nx) and lat_f (ny + 2*halo) are host vectors."""
        dt = np.dtype(dtype)
        lon = _host(lon, dt); lat_f = _host(lat_f, dt)
        if lon.shape != (nx,) or lat_f.shape != (ny + 2 * halo,):
            raise ValueError("lon must have nx entries, lat_f ny + 2*halo")
        fn = getattr(self.lib, f"sb_band_get_dist_{_SFX[dt]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo), C.c_int(1 if south else 0), C.c_int(1 if north else 0),
                     _p(coast_f), _p(mask_f), _p(lon), _p(lat_f), _CT[dt](maxdist), C.c_int(kwin), _p(cdist_f),
                     C.c_void_p(stream) if stream else None), "sb_band_get_dist_dev")

    def band_coast_open(self, dtype, nx, ny, halo, south, north, lon, lat_f, kwin, rule=1, maxdist=180.0, incremental=True):
        """Open the band's moving coast (include/seabreeze_hip.h: sb_band_coast_open): lon (nx) and lat_f (ny + 2*halo,
        one per frame row) are host vectors and are copied; a cut side needs kwin + 1 <= halo."""
        dt = np.dtype(dtype)
        lon = _host(lon, dt); lat_f = _host(lat_f, dt)
        if lon.shape != (nx,) or lat_f.shape != (ny + 2 * halo,):
            raise ValueError("lon must have nx entries, lat_f ny + 2*halo")
        fn = getattr(self.lib, f"sb_band_coast_open_{_SFX[dt]}")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo), C.c_int(1 if south else 0), C.c_int(1 if north else 0),
                     _p(lon), _p(lat_f), _CT[dt](maxdist), C.c_int(kwin), C.c_int(rule), C.c_int(1 if incremental else 0)),
                  "sb_band_coast_open")

    def band_ice_dev(self, dtype, lsm_f, ci_f, cdist_f, stream=None):
        """Enqueue the coast and distance update of the band's cdist frame for this ice frame (device frames, raw
        addresses, the precision the coast was opened with); no synchronisation."""
        fn = getattr(self.lib, f"sb_band_ice_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, _p(lsm_f), _p(ci_f), _p(cdist_f), C.c_void_p(stream) if stream else None), "sb_band_ice_dev")

    def band_ice_report(self):
        """Ice calls since the open / those after the first whose coast differed (-1 on the whole path) / (own row, tile)
        pairs the last call marked / pairs of the band.  Synchronises."""
        arr = (C.c_longlong * 4)()
        self._chk(self.lib.sb_band_ice_report(self.h, arr), "sb_band_ice_report")
        return dict(calls=arr[0], changed_calls=arr[1], tiles_marked=arr[2], tiles=arr[3])

    def band_coast_close(self):
        self._chk(self.lib.sb_band_coast_close(self.h), "sb_band_coast_close")

    def um_coast_open(self, dtype, nx, ny, halo_i, halo_j, win_i, win_j, true_lat, true_lon, maxdist=180.0, incremental=True):
        """Open the UM layout's moving coast (include/seabreeze_hip.h: sb_um_coast_open): true_lat, true_lon (ny, nx),
        degrees, are host arrays and are copied to the device; halo_i, halo_j >= 1 say where the interior of the ice
        calls' (ny + 2*halo_j, nx + 2*halo_i) frames lies, the window is +-win_i x +-win_j, each 0 .. SB_DIST_UM_MAX_WINDOW."""
        dt = np.dtype(dtype)
        true_lat = _host(true_lat, dt); true_lon = _host(true_lon, dt)
        if true_lat.shape != (ny, nx) or true_lon.shape != (ny, nx):
            raise ValueError("true_lat, true_lon must be (ny, nx)")
        fn = getattr(self.lib, f"sb_um_coast_open_{_SFX[dt]}")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i), C.c_int(halo_j), C.c_int(win_i), C.c_int(win_j),
                     _p(true_lat), _p(true_lon), _CT[dt](maxdist), C.c_int(1 if incremental else 0)), "sb_um_coast_open")
        self._um = (dt, nx, ny, halo_i, halo_j)

    def um_ice_dev(self, dtype, landfrac_l, icefrac_l, cdist_l, stream=None):
        """Enqueue the coast and distance update of the interior of cdist_l for this ice frame (device frames, raw
        addresses, the precision the coast was opened with); no synchronisation."""
        fn = getattr(self.lib, f"sb_um_ice_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, _p(landfrac_l), _p(icefrac_l), _p(cdist_l), C.c_void_p(stream) if stream else None), "sb_um_ice_dev")

    def um_ice(self, landfrac_l, icefrac_l, cdist_l):
        """The ice call on host frames (ny + 2*halo_j, nx + 2*halo_i) of the precision the coast was opened with: stages
        them, synchronises and writes the interior of cdist_l in place (its ghost cells are untouched; what the call before
        left in its interior must still be there).  Returns cdist_l."""
        if getattr(self, "_um", None) is None:
            raise SeabreezeHipError("um_ice without um_coast_open")
        dt, nx, ny, hi, hj = self._um
        shape = (ny + 2 * hj, nx + 2 * hi)
        landfrac_l = _host(landfrac_l, dt); icefrac_l = _host(icefrac_l, dt)
        if landfrac_l.shape != shape or icefrac_l.shape != shape:
            raise ValueError(f"landfrac_l and icefrac_l must be {shape}")
        if not isinstance(cdist_l, np.ndarray) or cdist_l.shape != shape or cdist_l.dtype != dt or not cdist_l.flags.c_contiguous:
            raise ValueError(f"cdist_l must be a C-contiguous {shape} array of the coast's dtype")
        self._chk(getattr(self.lib, f"sb_um_ice_{_SFX[dt]}")(self.h, _p(landfrac_l), _p(icefrac_l), _p(cdist_l)), "sb_um_ice")
        return cdist_l

    def um_ice_report(self):
        """Ice calls since the open / those after the first whose coast differed (-1 on the whole path) / workgroup tiles
        (4 rows x 64 columns) the last call marked / tiles of the grid.  Synchronises."""
        arr = (C.c_longlong * 4)()
        self._chk(self.lib.sb_um_ice_report(self.h, arr), "sb_um_ice_report")
        return dict(calls=arr[0], changed_calls=arr[1], tiles_marked=arr[2], tiles=arr[3])

    def um_coast_close(self):
        self._chk(self.lib.sb_um_coast_close(self.h), "sb_um_coast_close")
        self._um = None

    def um_tile_coast_open(self, dtype, nx, ny, halo_i, halo_j, win_i, win_j, beyond, true_lat_l, true_lon_l, maxdist=180.0,
                           incremental=True):
        """Open the moving coast of one tile of a 2-D domain decomposition (include/seabreeze_hip.h:
        sb_um_tile_coast_open): every field is the rank's (ny + 2*halo_j, nx + 2*halo_i) frame; true_lat_l, true_lon_l,
        degrees, are host frames and are copied to the device.  beyond: the domain cells beyond the tile's west, east, south
        and north side (0: the domain's edge).  The window is +-win_i x +-win_j, each 0 .. SB_DIST_UM_MAX_WINDOW; every side
        needs halo >= min(win, beyond) + 1."""
        dt = np.dtype(dtype)
        true_lat_l = _host(true_lat_l, dt); true_lon_l = _host(true_lon_l, dt)
        shape = (ny + 2 * halo_j, nx + 2 * halo_i)
        if true_lat_l.shape != shape or true_lon_l.shape != shape:
            raise ValueError(f"true_lat_l, true_lon_l must be {shape}")
        if len(beyond) != 4:
            raise ValueError("beyond must hold four counts: west, east, south, north")
        b = (C.c_int * 4)(*[int(v) for v in beyond])
        fn = getattr(self.lib, f"sb_um_tile_coast_open_{_SFX[dt]}")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i), C.c_int(halo_j), C.c_int(win_i), C.c_int(win_j), b,
                     _p(true_lat_l), _p(true_lon_l), _CT[dt](maxdist), C.c_int(1 if incremental else 0)),
                  "sb_um_tile_coast_open")
        self._um_tile = (dt, nx, ny, halo_i, halo_j)

    def um_tile_ice_dev(self, dtype, landfrac_l, icefrac_l, cdist_l, stream=None):
        """Enqueue the coast and distance update of the interior of cdist_l for this ice frame (device frames, raw
        addresses, the precision the tile coast was opened with); no synchronisation."""
        fn = getattr(self.lib, f"sb_um_tile_ice_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, _p(landfrac_l), _p(icefrac_l), _p(cdist_l), C.c_void_p(stream) if stream else None),
                  "sb_um_tile_ice_dev")

    def um_tile_ice(self, landfrac_l, icefrac_l, cdist_l):
        """The tile's ice call on host frames (ny + 2*halo_j, nx + 2*halo_i) of the precision the tile coast was opened
        with: stages them, synchronises and writes the interior of cdist_l in place (its ghost cells are untouched; what
        the call before left in its interior must still be there).  Returns cdist_l."""
        if getattr(self, "_um_tile", None) is None:
            raise SeabreezeHipError("um_tile_ice without um_tile_coast_open")
        dt, nx, ny, hi, hj = self._um_tile
        shape = (ny + 2 * hj, nx + 2 * hi)
        landfrac_l = _host(landfrac_l, dt); icefrac_l = _host(icefrac_l, dt)
        if landfrac_l.shape != shape or icefrac_l.shape != shape:
            raise ValueError(f"landfrac_l and icefrac_l must be {shape}")
        if not isinstance(cdist_l, np.ndarray) or cdist_l.shape != shape or cdist_l.dtype != dt or not cdist_l.flags.c_contiguous:
            raise ValueError(f"cdist_l must be a C-contiguous {shape} array of the coast's dtype")
        self._chk(getattr(self.lib, f"sb_um_tile_ice_{_SFX[dt]}")(self.h, _p(landfrac_l), _p(icefrac_l), _p(cdist_l)),
                  "sb_um_tile_ice")
        return cdist_l

    def um_tile_ice_report(self):
        """um_ice_report's four fields for the tile coast: ice calls since the open / those after the first whose coast
        differed (-1 on the whole path) / workgroup tiles (4 rows x 64 columns of the interior) the last call marked / tiles
        of the interior.  Synchronises."""
        arr = (C.c_longlong * 4)()
        self._chk(self.lib.sb_um_tile_ice_report(self.h, arr), "sb_um_tile_ice_report")
        return dict(calls=arr[0], changed_calls=arr[1], tiles_marked=arr[2], tiles=arr[3])

    def um_tile_coast_close(self):
        self._chk(self.lib.sb_um_tile_coast_close(self.h), "sb_um_tile_coast_close")
        self._um_tile = None

    def get_edges_um_dev(self, dtype, nx, ny, halo_i, halo_j, landfrac_l, icefrac_l, coast, stream=None):
        """UM-layout get_edges on device arrays (raw addresses); enqueues without synchronising."""
        fn = getattr(self.lib, f"sb_get_edges_um_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i), C.c_int(halo_j), _p(landfrac_l), _p(icefrac_l),
                     _p(coast), C.c_void_p(stream) if stream else None), "sb_get_edges_um_dev")

    def get_dist_um_dev(self, dtype, nx, ny, halo_i, halo_j, coast_l, landfrac, true_lat, true_lon, cdist,
                        maxdist=180.0, stream=None):
        """UM-layout get_dist on device arrays (raw addresses, coordinates included); enqueues without synchronising."""
        dt = np.dtype(dtype)
        fn = getattr(self.lib, f"sb_get_dist_um_{_SFX[dt]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i), C.c_int(halo_j), _p(coast_l), _p(landfrac),
                     _p(true_lat), _p(true_lon), _CT[dt](maxdist), _p(cdist), C.c_void_p(stream) if stream else None),
                  "sb_get_dist_um_dev")

    def get_dist_um_win_dev(self, dtype, nx, ny, halo_i, halo_j, win_i, win_j, coast_l, landfrac, true_lat, true_lon,
                            cdist, maxdist=180.0, stream=None):
        """get_dist_um_win on device arrays (raw addresses, coordinates included); enqueues without synchronising."""
        dt = np.dtype(dtype)
        fn = getattr(self.lib, f"sb_get_dist_um_win_{_SFX[dt]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i), C.c_int(halo_j), C.c_int(win_i), C.c_int(win_j),
                     _p(coast_l), _p(landfrac), _p(true_lat), _p(true_lon), _CT[dt](maxdist), _p(cdist),
                     C.c_void_p(stream) if stream else None), "sb_get_dist_um_win_dev")

    def tile_get_edges_um_dev(self, dtype, nx, ny, halo_i, halo_j, ext_i, ext_j, sides, landfrac_l, icefrac_l, coast_l,
                              stream=None):
        """tile_get_edges_um on device frames (raw addresses); enqueues without synchronising."""
        fn = getattr(self.lib, f"sb_tile_get_edges_um_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i), C.c_int(halo_j), C.c_int(ext_i), C.c_int(ext_j),
                     C.c_int(sides), _p(landfrac_l), _p(icefrac_l), _p(coast_l), C.c_void_p(stream) if stream else None),
                  "sb_tile_get_edges_um_dev")

    def tile_get_dist_um_dev(self, dtype, nx, ny, halo_i, halo_j, win_i, win_j, sides, coast_l, landfrac_l, true_lat_l,
                             true_lon_l, cdist_l, maxdist=180.0, stream=None):
        """tile_get_dist_um on device frames (raw addresses, coordinates included); enqueues without synchronising."""
        dt = np.dtype(dtype)
        fn = getattr(self.lib, f"sb_tile_get_dist_um_{_SFX[dt]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo_i), C.c_int(halo_j), C.c_int(win_i), C.c_int(win_j),
                     C.c_int(sides), _p(coast_l), _p(landfrac_l), _p(true_lat_l), _p(true_lon_l), _CT[dt](maxdist),
                     _p(cdist_l), C.c_void_p(stream) if stream else None), "sb_tile_get_dist_um_dev")

    def sigma_moments_dev(self, dtype, nx, ny, halo, sigma, moments5, stream=None):
        """Band-local sigma moments -> 5 doubles at device address moments5."""
        fn = getattr(self.lib, f"sb_sigma_moments_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, C.c_int(nx), C.c_int(ny), C.c_int(halo), _p(sigma), _p(moments5),
                     C.c_void_p(stream) if stream else None), "sb_sigma_moments_dev")

    def device_upload(self, dst, src):
        """Host array -> device address `dst` on the context's own stream (sb_device_upload); synchronises that stream."""
        src = np.ascontiguousarray(src)
        self._chk(self.lib.sb_device_upload(self.h, _p(dst), _p(src), C.c_size_t(src.nbytes)), "sb_device_upload")

    def device_download(self, dst, src):
        """Device address `src` -> the C-contiguous host array `dst` on the context's own stream (sb_device_download);
        synchronises that stream."""
        if not isinstance(dst, np.ndarray) or not dst.flags.c_contiguous:
            raise ValueError("dst must be a C-contiguous numpy array")
        self._chk(self.lib.sb_device_download(self.h, _p(dst), _p(src), C.c_size_t(dst.nbytes)), "sb_device_download")
        return dst

    def use_gathered_moments(self, gathered, nparts: int):
        """Following diag calls merge `nparts` gathered moments (device address) instead of scanning sigma."""
        self._chk(self.lib.sb_use_gathered_moments(self.h, _p(gathered) if gathered else None, C.c_int(nparts)),
                  "sb_use_gathered_moments")


    # ------------------------------------------------------------------ latitude-band communication (RCCL)
    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        assert len(unique_id) == 128
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._chk(self.lib.sb_comm_init(self.h, buf, C.c_int(rank), C.c_int(nranks)), "sb_comm_init")

    def comm_finalize(self):
        self._chk(self.lib.sb_comm_finalize(self.h), "sb_comm_finalize")

    def swap_bounds_dev(self, dtype, field, nx, ny, halo, stream=None):
        """Ghost-cell fill of a device field (nx+2h, ny+2h): N-S rows over RCCL, poles and E-W locally."""
        fn = getattr(self.lib, f"sb_swap_bounds_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, _p(field), C.c_int(nx), C.c_int(ny), C.c_int(halo),
                     C.c_void_p(stream) if stream else None), "sb_swap_bounds_dev")

    def fill_ghosts_dev(self, dtype, field, nx, ny, halo, south, north, stream=None):
        """The local part of swap_bounds: E-W wrap of every row, pole replication where south / north is set."""
        fn = getattr(self.lib, f"sb_fill_ghosts_{_SFX[np.dtype(dtype)]}_dev")
        self._chk(fn(self.h, _p(field), C.c_int(nx), C.c_int(ny), C.c_int(halo), C.c_int(1 if south else 0),
                     C.c_int(1 if north else 0), C.c_void_p(stream) if stream else None), "sb_fill_ghosts_dev")

    def band_seabreeze_diag_dev(self, dtype, timestep, tn, nx, ny, nz, halo, p, u, v, theta, mask, z, sigma,
                                ws, wd, thc, sb_con, stream=None, tunables: Tunables | None = None):
        """One step of a latitude band incl. its communication (moments all-gather, theta ghost rows)."""
        dt = np.dtype(dtype)
        fn = getattr(self.lib, f"sb_band_seabreeze_diag_{_SFX[dt]}_dev")
        rc = fn(self.h, _CT[dt](timestep), C.c_int(tn), C.c_int(nx), C.c_int(ny), C.c_int(nz), C.c_int(halo),
                _p(p), _p(u), _p(v), _p(theta), _p(mask), _p(z), _p(sigma), _p(ws), _p(wd), _p(thc), _p(sb_con),
                C.byref(tunables) if tunables is not None else None, C.c_void_p(stream) if stream else None)
        self._chk(rc, "sb_band_seabreeze_diag_dev")

    def allgather_moments_dev(self, mine5, gathered, stream=None):
        self._chk(self.lib.sb_allgather_moments_dev(self.h, _p(mine5), _p(gathered),
                                                    C.c_void_p(stream) if stream else None),
                  "sb_allgather_moments_dev")


def comm_unique_id() -> bytes:
    """128-byte RCCL unique id (call on rank 0, broadcast to every rank, pass to Context.comm_init)."""
    lib = load_library()
    buf = (C.c_ubyte * 128)()
    rc = lib.sb_comm_get_unique_id(buf)
    if rc != 0:
        raise SeabreezeHipError(f"sb_comm_get_unique_id failed ({rc}): {lib.sb_last_error(None).decode()}")
    return bytes(buf)


def dist_window(lon, lat, maxdist=180.0) -> int:
    lib = load_library()
    lon = np.ascontiguousarray(lon)
    dt = np.dtype(lon.dtype)
    lat = _host(lat, dt)
    k = C.c_int(0)
    rc = getattr(lib, f"sb_dist_window_{_SFX[dt]}")(C.c_int(lon.size), C.c_int(lat.size), _p(lon), _p(lat),
                                                   _CT[dt](maxdist), C.byref(k))
    if rc != 0:
        raise SeabreezeHipError(f"sb_dist_window failed ({rc}): {lib.sb_last_error(None).decode()}")
    return k.value


def contrast_regimes(hist):
    """Band cells per contrast regime from a search_radius histogram of nhist >= 129 bins: radius <= 16 (the strip
    kernel), 17..32 (the wide strip / tile kernels), 33..127 (in reach of the table contrast), beyond 127 (the global path
    whatever is switched on), and without a window.  Counts only: which switches to set is the caller's decision."""
    h = np.asarray(hist)
    if h.ndim != 1 or h.size < 129:
        raise ValueError("contrast_regimes needs a histogram of at least 129 bins (radii up to 127 told apart)")
    return dict(strip=int(h[1:17].sum()), wide=int(h[17:33].sum()), table=int(h[33:128].sum()), beyond=int(h[128:].sum()),
                none=int(h[0]))


def get_threads() -> int:
    lib = load_library()
    n = C.c_int(0)
    lib.sb_get_threads(C.byref(n))
    return n.value
