/*
 * seabreeze_hip.h -- C ABI of libseabreeze_hip.so, the MI355X (gfx950) implementation
 * of the sea-breeze trigger diagnostic's hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / C++ types.
 * The Fortran host modules (fortran/ *.f90, ISO_C_BINDING) and the f2py-surface Python
 * module (python_wrapper/) bind exactly these entry points; INTEGRATION.md shows the
 * reference-side stubs.  Paths cited as "ref:" are relative to the reference tree
 * (antarcticrainforest/seabreeze_param).
 *
 * Conventions
 *   - Arrays are Fortran order, longitude fastest: f(lon, lat[, lev]); contiguous.
 *   - Two precisions: _f32 (default REAL) and _f64 (REAL under -fdefault-real-8),
 *     mirroring how the reference picks its working precision at compile time.
 *   - Entry points without a suffix take HOST pointers (drop-in semantics: the caller
 *     owns every array, ref: SURVEY.md §8(b) "Ownership"); the library stages them
 *     through device buffers it owns.  `_dev` entry points take DEVICE pointers and
 *     enqueue on `stream` (a hipStream_t passed as void*; NULL = the context's own
 *     stream) without synchronising -- this is what a GPU-resident host model and
 *     bench.py use.  NULL is the context's own non-blocking stream, never the legacy
 *     default stream: a caller that passes NULL orders its work against the calls
 *     through the context (sb_device_upload / _download, sb_synchronize).
 *     "Without synchronising" holds for the steady state, the second and later call
 *     of one geometry and one set of switches on one context.  A call WAITS FOR THE
 *     DEVICE where the grow-only workspace has to grow -- the first call of a
 *     context, of a larger grid or ghost width, of an option that brings planes of
 *     its own: the smaller buffer is freed, and hipFree waits --, and the first band
 *     step of a context creates its second stream.  sb_get_dist_*_dev and
 *     sb_band_get_dist_*_dev wait for the device when they are handed other
 *     coordinates than the call before (the tables are made anew from a host vector
 *     that may still be on its way), and once for the stream that uploaded the tables
 *     when the same coordinates come back on ANOTHER stream.  Everything a call
 *     enqueues -- kernels, the zeroing of its flag and plan buffers, copies -- is
 *     ordered on `stream`; a band step's second stream forks from it and joins it
 *     inside the call (tests/test_enqueue_only_gpu.py).
 *   - Every function returns SB_OK (0) or an sb_status; sb_last_error() gives text.
 *     The reference has no error reporting on this path (generic + wrapper) and an
 *     `error` out-argument in the UM copy (ref: UM/vn10.7/sea_breeze_diag.F90:102,
 *     198-202); the Fortran modules map a non-zero status to `error stop` / `error`.
 *   - There is NO CPU fallback: without a usable gfx950 device sb_create fails with
 *     SB_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef SEABREEZE_HIP_H
#define SEABREEZE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sb_ctx sb_ctx;

typedef enum sb_status {
    SB_OK = 0,
    SB_ERR_ARG = 1,        /* bad dimension / NULL pointer / unsupported combination   */
    SB_ERR_HIP = 2,        /* a HIP runtime call failed                                */
    SB_ERR_NO_DEVICE = 3,  /* no gfx950 device visible                                 */
    SB_ERR_ALLOC = 4,      /* device workspace allocation failed                       */
    SB_ERR_COMM = 5        /* RCCL halo exchange failed / not initialised              */
} sb_status;

/* Window / neighbour index rule at the domain edge. */
typedef enum sb_boundary {
    /* lat clamp, lon `max(1, modulo(jj, nlons))` -- reproduces the f2py kernels
       verbatim, including the lon quirk (ref: python_wrapper/seabreezediag/
       seabreeze_diag_python.f90:201-202, sobel.f90:67-68) */
    SB_BND_WRAPPER = 0,
    /* lat clamp, true periodic lon: the single-domain reading of the generic code's
       unguarded window (ref: generic/sea_breeze_diag.f90:198-200)                    */
    SB_BND_GLOBAL = 1,
    /* raw reads into `halo` ghost cells supplied by the caller around theta, mask, z
       and sigma (UM-style bounds 1-h:n+h, ref: UM/vn10.7/sea_breeze_diag.F90:94-99,
       241-243); the ghost cells are what swap_bounds fills                            */
    SB_BND_HALO = 2
} sb_boundary;

/* Tunables of the trigger in SI units (ref: generic/sea_breeze_diag.f90:127-138). */
typedef struct sb_tunables {
    double target_plev_pa;   /* 70000.  */
    double thresh_wind;      /* 11.     */
    double thresh_winddir;   /* 90.     */
    double thresh_windch;    /* 5.      */
    double thresh_thc;       /* 0.75    */
    double target_time_s;    /* 21600.  */
    double maxdist_km;       /* 180.    */
} sb_tunables;

/* -------------------------------------------------------------------------------- */
/* context                                                                          */
/* -------------------------------------------------------------------------------- */
int  sb_create(sb_ctx **ctx, int device);            /* device < 0: current device   */
int  sb_destroy(sb_ctx *ctx);
const char *sb_last_error(const sb_ctx *ctx);        /* ctx may be NULL               */
const char *sb_version(void);
void sb_default_tunables(sb_tunables *t);
/* Expected largest search radius of the land/sea window: up to 16 the marching-strip contrast
   kernel runs (LDS halo 16); beyond it, in single precision, the 96-column strip kernel (radii up to 31 from LDS),
   in double precision the tile kernel with a halo of 24 or 32 cells.  Correctness never depends on it -- cells that
   need more take a global-memory path --, and t0 is formed by one sequence of operations in every kernel; the window
   means are exact fixed-point sums in the strip kernels and rounded sums in the tile kernel and on the global path,
   so thc may differ between kernels in its last bits (fp64: a few ulp; the tests hold 1e-7 against the reference). */
int  sb_set_search_radius_hint(sb_ctx *ctx, int radius);
/* Single-domain host-model calls let the strip contrast kernel merge k_scan's statistics and compact
   k_wind's segment lists itself (on, the default) or leave that to a kernel of its own between k_scan and
   the contrast kernel (off).  A measurement and test knob: results never depend on it.                  */
int  sb_set_fold(sb_ctx *ctx, int on);
/* The strip contrast kernel's plan -- which blocks each workgroup marches over, in which order, and where their
   coastal-band cells lie -- follows from the band plane (|mask| <= maxdist) alone.  It is kept in device memory from
   call to call; k_scan compares every word of the plane it writes with the word the call before left, and the first
   difference makes the kernel plan afresh (on, the default).  Off: it plans every call.  A measurement and test
   knob: results never depend on it.                                                                       */
int  sb_set_plan_cache(sb_ctx *ctx, int on);
/* Search radii beyond 16 (radius hints of 17 .. 32): in single precision the 96-column marching-strip kernel answers
   windows of up to 31 cells from LDS (on, the default); off: the tile kernel, as in double precision.  A measurement and
   test knob: results agree to single-precision rounding of the window means.                                      */
int  sb_set_wide_strip(sb_ctx *ctx, int on);
/* A band step (sb_band_seabreeze_diag_*_dev, or a diag call with gathered moments in use) on the strip kernel runs
   k_scan and k_wind ahead of the join with the communication stream and lets the contrast kernel apply the update
   (0, the default), or k_scan | join | contrast kernel, k_wind -- the three kernels of a single-domain call, one
   launch less, but less work to cover the communication with (1).  A measurement knob: results never depend on it.  */
int  sb_set_band_order(sb_ctx *ctx, int contrast_first);
/* k_wind's column walk in double precision with the generic flavour's first-minimum rule on a whole call: two cells per
   lane and two pressure levels per 16-byte load where nx and the ghost width are even and p lies on a 16-byte boundary
   (on, the default), or one cell and one level per load everywhere, as every other call walks (off).  The level found
   is the same bit for bit.  A measurement and test knob: results never depend on it.                             */
int  sb_set_wind_pairs(sb_ctx *ctx, int on);
/* *ran = 1: the k_wind of the last diag call on this context was the paired instance, 0: it was not.  The host decides
   that when it enqueues the call: no synchronisation.                                                           */
int  sb_last_wind_pairs(sb_ctx *ctx, int *ran);
/* The kernels that run one persistent workgroup per compute unit (k_scan, the contrast kernel; k_wind four per unit)
   take n workgroups instead (1 .. the device's compute units; 0: back to the default).  A test knob -- with a few
   workgroups a small grid exercises what only grids far beyond the BASELINE sizes reach otherwise: shares of the
   strip kernel's march that span several rounds and hold more query steps than a stored plan does.  Results never
   depend on it.                                                                                                  */
int  sb_set_workgroups(sb_ctx *ctx, int n);
/* Opt-in, off by default: the caller states that sigma (the sub-grid orography deviation, an ancillary that a
   host model reads once; ref: generic/sea_breeze_diag.f90:159-166 recomputes its mean and deviation every
   call) does not change between calls.  The first complete diag / band step after the switch forms the
   statistics as usual; later calls that pass the same array (address, shape, ghost width, precision) reuse its
   sigmoid scalars: k_scan stops reading sigma (one of its three planes) and a band step drops the moments
   all-gather and the merge.  Results are those of the default path as long as the statement holds; any other
   sigma array, or switching the option again, forms the statistics anew.                                  */
int  sb_set_static_sigma(sb_ctx *ctx, int on);
/* Opt-in, off by default: the land-sea contrast from device-wide summed-area tables, at a cost per band cell that does not
   depend on the radius of its window -- for grids on which band cells lie further from the other class than the LDS
   kernels reach (radius hint 32 at the most), where every such cell otherwise takes the global-memory path: regional
   grids of a few km, whose 180 km band is 45 (4 km) to 120 (1.5 km) cells wide.  Every call builds three tables over the
   whole ghost-celled frame -- prefix sums of t0 in 64-bit fixed point (2^-36 K, rounded once), of the same over
   land-side cells and of the land-side count: 20 bytes per frame cell of grow-only workspace, allocated by the first
   call that uses them -- and answers every band cell from them: the radius by bisection on the count table, the two
   window sums exactly.  Reach: radii up to 127; domain: |t0| < 2048 K (beyond, or NaN, the windows that hold the cell
   are garbage, not a fault).  Cells beyond the reach, cells whose window is wider than the longitude circle and cells
   that find one class only as far as they may search take the global-memory path as ever and are counted as ever
   (sb_last_counters).  thc agrees with the other kernels to the rounding of the window means (fp64: within the 1e-7
   the tests hold against the reference; the fixed-point rounding moves sb_con by 2.1e-10 at the most).
   Takes effect for WHOLE SINGLE-DOMAIN calls of the host-model flavour -- sb_seabreeze_diag_*[_dev],
   sb_seabreeze_diag_um_*[_dev] -- with SB_BND_GLOBAL or SB_BND_HALO: six launches (k_scan, k_prep, two table passes, the
   query, k_wind).  Alone it changes nothing -- exactly what runs without it -- for the f2py flavour (sb_diag_*,
   sb_diag_stream_*; SB_BND_WRAPPER), for band steps (sb_band_seabreeze_diag_*) and while gathered moments are in use: the
   first has a switch of its own beside this one, sb_set_table_contrast_f2py, the other two sb_set_table_contrast_bands.  It is never
   chosen automatically, whatever the radius hint.  sb_profile_end reports the row pass under [2] and the column pass
   and the query together under [3] for such calls.                                                                 */
int  sb_set_table_contrast(sb_ctx *ctx, int on);
/* Opt-in, off by default, beside the table contrast above: the tables for the calls of a multi-band run too.  Takes effect
   only while sb_set_table_contrast is on, for the host-model flavour with SB_BND_HALO, and only for
     - band steps, sb_band_seabreeze_diag_*[_dev].  Ahead of the join with the communication stream, as without it:
       k_scan (publishes the band's moments), k_prep (every call: no stored plan is trusted), k_wind, which leaves its
       winds in scratch planes.  Behind it: k_merge_moments (the scalars of the gathered moments; dropped where
       sb_set_static_sigma lets them stand), the two table passes over the band's whole ghost-celled frame, and the
       query, which applies thresholds and state update itself: 3 + 4 launches.  theta gets the whole swap_bounds on the
       communication stream -- neighbour rows, pole replication, east-west wrap: one fill kernel -- as the tile kernel's
       band step does;
     - diag calls while gathered moments are in use (sb_use_gathered_moments: bands driven from outside, ghost cells
       filled by the caller): the same seven kernels in one sequence.  sb_profile_end reports the row pass under [2],
       the column pass and the query together under [3]; k_merge_moments is not timed.
   With it off, or sb_set_table_contrast off, such calls enqueue exactly what they enqueue without it; whole
   single-domain calls never depend on it.
   Ghost cells: the tables know no wrap and no clamp, a window is answered from them while it lies within the frame.  The
   caller's contract is halo >= the largest radius, with the ghost cells of mask, z and sigma filled as a band step
   expects them anyway; a band cell whose window needs more than the ghost width takes the global-memory path, bounded
   by the frame and counted as ever (sb_last_counters) -- where the frame shows one class only the result is NaN, as for
   every contrast kernel of a band.
   Ignored for these calls: sb_set_band_order (k_wind always runs ahead of the join) and sb_set_table_window_cache (no
   window is kept; the stored windows of a whole call are dropped, as after any other call on the context).
   Results are those of the whole-grid table call on the same cells.  It is never chosen automatically.               */
int  sb_set_table_contrast_bands(sb_ctx *ctx, int on);
/* Opt-in, off by default, beside the table contrast above: the tables for the f2py flavour too.  Takes effect only while
   sb_set_table_contrast is on, for WHOLE calls of that flavour -- sb_diag_*[_dev] and every sb_diag_stream_step_* -- which
   run under SB_BND_WRAPPER without ghost cells: six launches (k_scan, k_prep, the row pass, the column pass, the query,
   k_wind) where the flavour runs five.  The row pass forms t0 itself and writes the t0 plane of `output` (rows
   1 .. nlats - 1, the same bits as k_t0 writes; row nlats stays untouched), so no k_t0 is launched; sb_profile_end
   reports the row pass under [2], the column pass and the query together under [3].
   The wrapper's index rule -- latitude clamped, column max(1, modulo(jj, nlons)) -- never reads the last column: an
   offset that lands there, the centre of a last-column cell included, reads column 1.  The tables are therefore built
   over the EFFECTIVE row, whose last column holds column 1's value and land-side bit, and a window is a truly periodic
   one over that row: radii up to 127 while 2 r + 1 <= nlons.  Cells beyond the reach, cells whose window is wider than
   the circle and one-class cells take the global-memory path, which knows the rule, and are counted as ever
   (sb_last_counters).  Results agree with the default path of the flavour as the host-model table call agrees with its.
   sb_set_table_window_cache takes effect for these calls wherever this switch does (a streamed run on a standing mask).
   With it off, or sb_set_table_contrast off, the f2py flavour enqueues exactly what it enqueues without it.  Ignored:
   by the host-model flavour, by band steps and while gathered moments are in use.  It is never chosen automatically.   */
int  sb_set_table_contrast_f2py(sb_ctx *ctx, int on);
/* Opt-in, off by default, for the table contrast above: keep every band cell's window while the coast stands.  The radius
   of a cell's window and the land-side cells in it follow from the land-side plane (mask >= 0) and the geometry alone, and
   mask -- the signed coast distance -- changes only when the host model's ice mask does.  A table call that searches
   ("fills") leaves radius and count of every band cell in one more plane; the calls after it take them from there and
   neither build nor read the count table: the two passes move 16 instead of 20 bytes per frame cell, the query one word
   per band cell instead of a bisection.  Cells the tables do not answer are marked and take the global-memory path every
   call, counted as ever.
   Dropped: by content, on the device -- k_scan compares every word of the band plane and of the land-side plane with
   what the call before left, and the first difference makes this call search again; nothing is stated by the caller, and
   the host-pointer entry points are served like the device-pointer ones.  And by the host whenever the planes k_scan
   compared with are not those of the stored windows: after any other diag call or band step on this context (the f2py
   flavour and sb_diag_stream_* unless they run as table calls themselves -- sb_set_table_contrast_f2py --, a band step, a
   call with this switch or the table contrast off, another grid, boundary rule or ghost width), after a failed launch,
   a reallocated workspace, and when this switch is set.  No synchronisation, no
   further launch: six launches, as without it.
   Results are those of the table path bit for bit, counters included, whether a call fills or not.
   Workspace: 4 bytes per interior cell, grow-only, allocated with the tables while the switch is on.
   Takes effect exactly where sb_set_table_contrast does, and for the f2py flavour where sb_set_table_contrast_f2py does;
   silently ignored wherever those are ignored and while they are off.
   It is never chosen automatically.                                                                                  */
int  sb_set_table_window_cache(sb_ctx *ctx, int on);
/* [0] band cells of the last diag call that were answered from a stored window, [1] band cells of that call whose window
   was searched (found or not); both 0 when that call did not run with the window cache in effect.  [2] calls whose
   kernels searched, [3] calls that ran with the cache in effect, both since sb_set_table_window_cache(ctx, 1) last.
   A call that failed counts as a call without the cache.  Synchronises the device, as sb_last_counters does (a diag
   call may have been enqueued on a stream of the caller's).                                                         */
int  sb_table_cache_report(sb_ctx *ctx, long long rep[4]);
/* Opt-in guard for missing and non-finite temperatures.  Every contrast kernel but the global-memory search assumes
   |t0| < 2048 K (64-bit fixed point in the strip kernels and the tables, fp64 prefix sums about a per-tile offset in the
   tile kernel): a NaN, an Inf or the 2.0e20 missing value in theta or z leaves a finite, wrong thc in the windows that hold
   the cell, where the reference lets it flow into the window means (generic/sea_breeze_diag.f90:198-216: NaN, +-Inf or
   about 2e20 / n in thc, NaN or 0 in sb_con).  With the guard on, a call
     - marks every cell of the ghost-celled frame with !(|theta| + 0.0060956 |z| < 2048) as bad, ahead of its first kernel
       (one pass over theta and z: two reads per frame cell);
     - behind the contrast kernel dilates the bad cells by that kernel's reach -- 16 cells (k_strip), 31 (k_strip32), 127
       (the tables), under the call's boundary rule; for the tile kernel, whose floating-point sums do not cancel, every
       tile whose staged rectangle holds a bad cell -- and computes the band cells so tainted again as the reference
       does: plain sums of t0 per class in double precision over the window the global-memory search finds;
     - then runs k_wind as ever.  Band cells that are not tainted keep the bits the contrast kernel left: their windows do
       not hold the cell, and the wrapped fixed-point sums cancel whatever bits it turned into.
   Four launches more (sb_last_step_report[0] counts them), all unconditional, no host synchronisation; without a bad cell
   three of them leave at once.  Radii, counters, marks, stored plans and stored windows follow from mask alone: the
   fields of sb_last_counters, sb_last_step_report[1..3] and sb_profile_end mean what they mean without the guard (its
   launches lie outside every timed pair).  Workspace: two bit planes of the frame, grow-only, allocated while the switch is on.
   Takes effect for WHOLE calls in which the contrast kernel runs ahead of a final k_wind: sb_seabreeze_diag_*[_dev] and
   sb_seabreeze_diag_um_*[_dev] (fold on or off; strip, 96-column strip or tile kernel; with sb_set_table_contrast, with
   or without sb_set_table_window_cache) and the f2py flavour, sb_diag_*[_dev] and sb_diag_stream_step_* (with or without
   sb_set_table_contrast_f2py).  Silently IGNORED where the contrast kernel applies the update itself -- a band step
   (sb_band_seabreeze_diag_*) and a call with gathered moments in use: those enqueue exactly what they enqueue without it,
   unless sb_set_nonfinite_guard_bands (below), a switch of its own, is on beside this one.
   Off by default; with the switch off a call enqueues exactly what it enqueued before the guard existed.
   Cost, measured on one MI355X at 2560 x 1920 x 56 in double precision: 54 us per call without a bad cell
   (165 against 111 us), about 0.5 ms more as soon as one cell has to be computed again (one thread per cell: latency).
   NOT covered: a non-finite sigma.  It poisons the statistics of the whole field, and the reference then returns NaN
   everywhere; nothing here looks at sigma.                                                                             */
int  sb_set_nonfinite_guard(sb_ctx *ctx, int on);
/* Opt-in, off by default, beside the guard above: the guard for the calls of a multi-band run too.  Takes effect only
   while sb_set_nonfinite_guard is on, for the host-model flavour, and only for
     - band steps, sb_band_seabreeze_diag_*[_dev], on every contrast kernel a band step can get (k_strip, k_strip32, the
       tile kernel, the tables under sb_set_table_contrast_bands);
     - sb_seabreeze_diag_*[_dev] and sb_seabreeze_diag_um_*[_dev] while gathered moments are in use
       (sb_use_gathered_moments), under any boundary rule, with sb_set_band_order 0 or 1.
   In those calls the contrast kernel applies thresholds and state update itself and writes over ws / wd, the state of the
   step before, so nothing behind it could form sb_con again.  The taint follows from theta, z, the band plane and the
   kernel's reach alone: k_guard_bits and the two taint passes therefore run directly AHEAD of the contrast kernel (for the
   tables between the column pass and the query), the latitude pass puts ws / wd of every tainted band cell aside, and
   the repair directly behind the contrast kernel computes those cells again and applies the update again from what was
   put aside: thc and sb_con are written over, ws / wd come out as the contrast kernel left them.  Under
   sb_set_band_order(ctx, 1) -- the contrast ahead of a final k_wind -- the guard runs as in a whole call.  Four launches
   more, as there; the reaches are the whole call's (16 / 31 / 127 / by tile).
   Ghost cells of theta: the guard reads the whole frame.  A band step on a strip kernel with nx > 98 otherwise exchanges
   the neighbour rows only and leaves theta's east-west ghost columns and polar ghost rows unfilled; while this switch
   is in effect theta gets the whole swap_bounds on the communication stream, as the tile kernel's and the tables' band
   steps get it anyway -- ONE FILL LAUNCH MORE for those steps (sb_last_step_report[0] counts it).  A call with gathered
   moments has its ghost cells filled by the caller.
   sb_guard_report and sb_last_step_report[0] mean for a served band step what they mean for a whole call; a band step
   counts once in [3].  Setting this switch resets [2] and [3], as setting the other does, and drops the strip kernel's
   stored plan (the next step plans its march afresh).  A profiled call with gathered moments times the three passes ahead
   of the tables' query within pair [3].
   Workspace: two planes of (nx, ny) elements beside the guard's bit planes, grow-only, allocated while the switch is on.
   With either switch off such calls enqueue exactly what they enqueue without it; whole single-domain calls never depend
   on it.  IGNORED: by the f2py flavour with gathered moments (sb_diag_* while sb_use_gathered_moments is in use), which
   enqueues what it enqueues without it.  Cost: DESIGN.md 2.4e.  It is never chosen automatically.                       */
int  sb_set_nonfinite_guard_bands(sb_ctx *ctx, int on);
/* [0] bad cells of the ghost-celled frame the last diag call found, [1] band cells that call computed again, [2] calls
   that found a bad cell, [3] calls that ran with the guard in effect, both since sb_set_nonfinite_guard was last called.
   All four are 0 after a call the guard did not serve.  Synchronises the device, as sb_last_counters does.            */
int  sb_guard_report(sb_ctx *ctx, long long rep[4]);
/* What the last diag call or band step enqueued on this rank: [0] kernel launches, [1] RCCL operations (sends,
   receives, all-gathers), [2] RCCL groups, [3] device-to-device copies.  No synchronisation.               */
int  sb_last_step_report(sb_ctx *ctx, int report[4]);
/* Counters of the last diag call: [0] band cells, [1] cells that left the LDS path,
   [2] cells whose search found only one class (result NaN; the reference loops
   forever there, ref: generic/sea_breeze_diag.f90:191-214), [3] max radius used.
   Synchronises the context's stream.                                                */
int  sb_last_counters(sb_ctx *ctx, long long counters[4]);
int  sb_synchronize(sb_ctx *ctx);
/* Per-kernel timing with HIP events on the stream the kernels run on.  Between sb_profile_begin and
   sb_profile_end the first `max_calls` diag calls record a pair of events around each of their
   launches; sb_profile_end synchronises and returns the average duration in ms of
   [0] k_scan [1] k_wind [2] k_t0 (f2py flavour only; 0 where a call does not launch it) [3] k_thc3
   [4] k_prep.  An event interval also holds the gap to the previous launch (about 5 us).          */
int  sb_profile_begin(sb_ctx *ctx, int max_calls);
int  sb_profile_end(sb_ctx *ctx, double avg_ms[5], int *ncalls);

/* -------------------------------------------------------------------------------- */
/* seabreeze_diag -- host-model flavour                                              */
/* replaces: subroutine seabreeze_diag(timestep, timestep_number, p, u, v, theta,   */
/*           mask, z, sigma, windspeed, winddir, thc, sb_con)                        */
/*           ref: generic/sea_breeze_diag.f90:55-271                                 */
/* p,u,v: (nx,ny,nz).  theta,mask,z,sigma: (nx+2*halo, ny+2*halo), interior at       */
/* offset `halo` (halo must be 0 unless bnd == SB_BND_HALO).                         */
/* windspeed,winddir,thc,sb_con: (nx,ny), updated in place.                          */
/* tun == NULL selects the reference's compile-time constants.                       */
/* -------------------------------------------------------------------------------- */
int sb_seabreeze_diag_f64(sb_ctx *ctx, double timestep_s, int timestep_number,
                          int nx, int ny, int nz, int halo, int bnd,
                          const double *p, const double *u, const double *v,
                          const double *theta, const double *mask, const double *z,
                          const double *sigma, double *windspeed, double *winddir,
                          double *thc, double *sb_con, const sb_tunables *tun);
int sb_seabreeze_diag_f32(sb_ctx *ctx, float timestep_s, int timestep_number,
                          int nx, int ny, int nz, int halo, int bnd,
                          const float *p, const float *u, const float *v,
                          const float *theta, const float *mask, const float *z,
                          const float *sigma, float *windspeed, float *winddir,
                          float *thc, float *sb_con, const sb_tunables *tun);
int sb_seabreeze_diag_f64_dev(sb_ctx *ctx, double timestep_s, int timestep_number,
                          int nx, int ny, int nz, int halo, int bnd,
                          const double *p, const double *u, const double *v,
                          const double *theta, const double *mask, const double *z,
                          const double *sigma, double *windspeed, double *winddir,
                          double *thc, double *sb_con, const sb_tunables *tun,
                          void *stream);
int sb_seabreeze_diag_f32_dev(sb_ctx *ctx, float timestep_s, int timestep_number,
                          int nx, int ny, int nz, int halo, int bnd,
                          const float *p, const float *u, const float *v,
                          const float *theta, const float *mask, const float *z,
                          const float *sigma, float *windspeed, float *winddir,
                          float *thc, float *sb_con, const sb_tunables *tun,
                          void *stream);

/* -------------------------------------------------------------------------------- */
/* seabreeze_diag -- UM vn10.7 field layout                                          */
/* replaces: subroutine seabreeze_diag(timestep, timestep_number, p, u, v, theta, z, */
/*           sigma, mask, windspeed, winddir, thc, sb_con, error)                    */
/*           ref: UM/vn10.7/sea_breeze_diag.F90:55-56 (argument order), :66-117      */
/*           (bounds), :198-202 (error), :210-211 (theta <- t0), :265-274 (level)    */
/* p, u, v, sb_con on pdims and windspeed, winddir, thc on tdims: (nx,ny[,nz]), no    */
/* ghost cells.  theta, z, sigma on tdims_s: (nx+2*halo_s, ny+2*halo_s).  mask (the   */
/* signed coast distance) on tdims_l: (nx+2*halo_l, ny+2*halo_l), halo_l >= halo_s.   */
/* The window reads both t0 and mask, so it can use halo_s ghost cells; a cell whose  */
/* window would need more yields NaN and is counted (sb_last_counters [2]).           */
/* *error = 1 and nothing done when ny < 1 or nz < 1 (UM :198-202), else 0.           */
/* flags: SB_UM_THETA_TO_T0 -- theta comes back as t0 = theta - gmma*z*sigmoid(sigma), */
/*        ghost cells included (UM :210-211; the arithmetic does not depend on it);    */
/*        SB_UM_LEVEL_WALK -- the UM copy's level rule: upwards from level 1 while     */
/*        |p - 70000| does not grow (ties move on), stop at the first increase         */
/*        (:265-274), instead of the generic file's first minimum over all levels.     */
/* The UM file cannot be compiled outside the UM: this entry point    */
/* follows its text; parity is pinned only through the generic/wrapper arithmetic.     */
/* -------------------------------------------------------------------------------- */
#define SB_UM_THETA_TO_T0 1
#define SB_UM_LEVEL_WALK  2
int sb_seabreeze_diag_um_f64(sb_ctx *ctx, double timestep_s, int timestep_number, int nx, int ny, int nz,
                             int halo_s, int halo_l, const double *p, const double *u, const double *v,
                             double *theta, const double *z, const double *sigma, const double *mask,
                             double *windspeed, double *winddir, double *thc, double *sb_con, int flags,
                             int *error);
int sb_seabreeze_diag_um_f32(sb_ctx *ctx, float timestep_s, int timestep_number, int nx, int ny, int nz,
                             int halo_s, int halo_l, const float *p, const float *u, const float *v,
                             float *theta, const float *z, const float *sigma, const float *mask,
                             float *windspeed, float *winddir, float *thc, float *sb_con, int flags,
                             int *error);
int sb_seabreeze_diag_um_f64_dev(sb_ctx *ctx, double timestep_s, int timestep_number, int nx, int ny, int nz,
                             int halo_s, int halo_l, const double *p, const double *u, const double *v,
                             double *theta, const double *z, const double *sigma, const double *mask,
                             double *windspeed, double *winddir, double *thc, double *sb_con, int flags,
                             int *error, void *stream);
int sb_seabreeze_diag_um_f32_dev(sb_ctx *ctx, float timestep_s, int timestep_number, int nx, int ny, int nz,
                             int halo_s, int halo_l, const float *p, const float *u, const float *v,
                             float *theta, const float *z, const float *sigma, const float *mask,
                             float *windspeed, float *winddir, float *thc, float *sb_con, int flags,
                             int *error, void *stream);

/* -------------------------------------------------------------------------------- */
/* diag -- f2py-surface flavour (whole global grid, 1-D p, packed output)            */
/* replaces: subroutine diag(timestep_number, p, z, std, theta, v, u, cdist,         */
/*           windspeed, winddir, thc, target_plev, thresh_wind, thresh_winddir,      */
/*           thresh_windch, thresh_thc, target_time, maxdist, timestep, nps, nlons,  */
/*           nlats, output)                                                          */
/*           ref: python_wrapper/seabreezediag/seabreeze_diag_python.f90:49-285      */
/* Units as at that surface: target_plev hPa, target_time h, timestep min; unlike    */
/* the reference they are NOT overwritten in place (:146-148).  Rows 1..nlats-1 are  */
/* processed, row nlats of `output` is left untouched (:165).  windspeed, winddir,   */
/* thc are updated in place like the reference's dummies.                            */
/* output: (nlons,nlats,4) = sb_con, t0, windspeed, winddir (:277-280).              */
/* -------------------------------------------------------------------------------- */
int sb_diag_f64(sb_ctx *ctx, int timestep_number, const double *p, const double *z,
                const double *std, const double *theta, const double *v, const double *u,
                const double *cdist, double *windspeed, double *winddir, double *thc,
                double target_plev, double thresh_wind, double thresh_winddir,
                double thresh_windch, double thresh_thc, double target_time,
                double maxdist, double timestep, int nps, int nlons, int nlats,
                double *output);
int sb_diag_f32(sb_ctx *ctx, int timestep_number, const float *p, const float *z,
                const float *std, const float *theta, const float *v, const float *u,
                const float *cdist, float *windspeed, float *winddir, float *thc,
                float target_plev, float thresh_wind, float thresh_winddir,
                float thresh_windch, float thresh_thc, float target_time,
                float maxdist, float timestep, int nps, int nlons, int nlats,
                float *output);
int sb_diag_f64_dev(sb_ctx *ctx, int timestep_number, const double *p, const double *z,
                const double *std, const double *theta, const double *v, const double *u,
                const double *cdist, double *windspeed, double *winddir, double *thc,
                double target_plev, double thresh_wind, double thresh_winddir,
                double thresh_windch, double thresh_thc, double target_time,
                double maxdist, double timestep, int nps, int nlons, int nlats,
                double *output, void *stream);
int sb_diag_f32_dev(sb_ctx *ctx, int timestep_number, const float *p, const float *z,
                const float *std, const float *theta, const float *v, const float *u,
                const float *cdist, float *windspeed, float *winddir, float *thc,
                float target_plev, float thresh_wind, float thresh_winddir,
                float thresh_windch, float thresh_thc, float target_time,
                float maxdist, float timestep, int nps, int nlons, int nlats,
                float *output, void *stream);

/* -------------------------------------------------------------------------------- */
/* diag, streamed: many timesteps on one grid                */
/* replaces: the per-timestep loop of the reference's Python driver,                 */
/*           ref: python_wrapper/seabreezediag/__init__.py:222-245 -- every step it   */
/*           hands diag the same z, std, cdist and the state of the step before.      */
/* sb_diag_stream_begin uploads those six planes once; sb_diag_stream_step takes one  */
/* step's p(nps), theta(nlons,nlats), v, u (nlons,nlats,nps) -- host pointers, units  */
/* and tunables as sb_diag_* -- uploads theta and the one u, v plane p selects through */
/* pinned double-buffered staging and enqueues the step; it hands back the sb_con     */
/* plane of the PREVIOUS step (rows 1..nlats-1 of sb_con_prev, as double, what the    */
/* reference's driver accumulates; *have_prev = 0 on the first step), so that staging  */
/* step i+1 overlaps the device work of step i.  sb_diag_stream_end waits, returns the */
/* last step's sb_con, the last step's four output planes and the final state (any of  */
/* them may be NULL).  Results are those of sb_diag_* called step by step.             */
/* sb_diag_stream_stats: steps so far and where the host spent its time, in seconds:   */
/* [0] host copies (staging, sb_con out) [1] enqueueing [2] waiting for the device.    */
/* -------------------------------------------------------------------------------- */
int sb_diag_stream_begin_f32(sb_ctx *ctx, int nlons, int nlats, const float *z, const float *std,
                             const float *cdist, const float *windspeed, const float *winddir, const float *thc);
int sb_diag_stream_begin_f64(sb_ctx *ctx, int nlons, int nlats, const double *z, const double *std,
                             const double *cdist, const double *windspeed, const double *winddir, const double *thc);
int sb_diag_stream_step_f32(sb_ctx *ctx, int timestep_number, const float *p, int nps, const float *theta,
                            const float *v, const float *u, float target_plev, float thresh_wind,
                            float thresh_winddir, float thresh_windch, float thresh_thc, float target_time,
                            float maxdist, float timestep, double *sb_con_prev, int *have_prev);
int sb_diag_stream_step_f64(sb_ctx *ctx, int timestep_number, const double *p, int nps, const double *theta,
                            const double *v, const double *u, double target_plev, double thresh_wind,
                            double thresh_winddir, double thresh_windch, double thresh_thc, double target_time,
                            double maxdist, double timestep, double *sb_con_prev, int *have_prev);
int sb_diag_stream_end_f32(sb_ctx *ctx, double *sb_con_last, float *output4, float *windspeed, float *winddir,
                           float *thc);
int sb_diag_stream_end_f64(sb_ctx *ctx, double *sb_con_last, double *output4, double *windspeed, double *winddir,
                           double *thc);
int sb_diag_stream_stats(sb_ctx *ctx, long *steps, double seconds[3]);

/* -------------------------------------------------------------------------------- */
/* diag, streamed, with sea ice that moves: the coast follows on the device (opt-in)  */
/* replaces: get_edges(lsm, ci[ts]) -> get_dist(coast, lsm, lon, lat) of every step of */
/*           the reference's driver, ref: python_wrapper/seabreezediag/__init__.py:    */
/*           222-245 (the ice plane is part of the land class, ref: sobel.f90:51).     */
/* A stream that never calls these behaves and costs as before.                        */
/* sb_diag_stream_coast: once, between sb_diag_stream_begin and the first step.  lsm   */
/* (nlons,nlats), lon(nlons), lat(nlats) are host pointers; lsm is uploaded and kept,   */
/* the window half-width k follows from maxdist_km as in sb_get_dist_* with kwin < 0   */
/* (same refusals: k > SB_DIST_MAX_WINDOW, the latitude nearest 70 degrees in the last */
/* row), and the search radius hint becomes k + 1.  The stream gets a coast bit plane  */
/* of its own.  incremental = 0: every ice call computes the whole grid (k_edges and   */
/* the whole-grid distance launch: the A/B and fallback path); grids narrower than the */
/* window (2k + 1 > nlons, k <= 31) take that path whatever is asked.                  */
/* sb_diag_stream_ice: ci(nlons,nlats), a host pointer, is staged through pinned       */
/* memory like a step's planes, and the update of the stream's resident cdist plane is */
/* enqueued on the context's stream, in order between the steps: rule 0 (lsm + ci >    */
/* 0.4) and the wrapper's neighbour indexing as sb_get_edges_*(rule 0, SB_BND_WRAPPER), */
/* the sign from lsm as the driver's get_dist(coast, lsm, ...).  No synchronisation,   */
/* no download, no comparison on the host.  The cdist handed to sb_diag_stream_begin   */
/* is replaced by the first ice call, which computes everything.  Later calls compare  */
/* the new coast with the stored one in 64-cell words; a changed word at columns       */
/* x0 .. x0+63 of row y marks the (target row, 256-column tile) pairs of rows y-k ..   */
/* y+k (clamped) and columns x0-k .. x0+63+k (circular; the whole row where 2k + 64 >= */
/* nlons), and the distance kernel computes the marked tiles again.  That is exact: a  */
/* target reads coast cells of its own window only, the tiles hold whole waves, and an  */
/* unmarked tile's windows hold no changed cell, so the resident plane equals, bit for */
/* bit, sb_get_edges_* + sb_get_dist_*(kwin = -1) of the same inputs after every call. */
/* sb_diag_stream_ice_report (synchronises): [0] ice calls of this stream [1] those     */
/* after the first whose coast differed (-1 on the whole-grid path: nothing is          */
/* compared there) [2] tiles the last call marked [3] tiles of the grid.                */
/* sb_diag_stream_get_cdist (synchronises): the resident distance plane, for            */
/* inspection and tests.                                                                */
/* sb_diag_stream_ice_time (waits for the last ice call): the HIP-event time in ms of   */
/* its device work -- the plane's upload, the clear of the marks, the kernels -- between */
/* two events every ice call records on the context's stream (the stream is the         */
/* context's own, so a caller cannot place events there): for measurements.             */
/* -------------------------------------------------------------------------------- */
int sb_diag_stream_coast_f32(sb_ctx *ctx, const float *lsm, const float *lon, const float *lat, float maxdist_km,
                             int incremental);
int sb_diag_stream_coast_f64(sb_ctx *ctx, const double *lsm, const double *lon, const double *lat, double maxdist_km,
                             int incremental);
int sb_diag_stream_ice_f32(sb_ctx *ctx, const float *ci);
int sb_diag_stream_ice_f64(sb_ctx *ctx, const double *ci);
int sb_diag_stream_ice_report(sb_ctx *ctx, long long rep[4]);
int sb_diag_stream_ice_time(sb_ctx *ctx, double *ms);
int sb_diag_stream_get_cdist_f32(sb_ctx *ctx, float *cdist);
int sb_diag_stream_get_cdist_f64(sb_ctx *ctx, double *cdist);

/* -------------------------------------------------------------------------------- */
/* sigmoid                                                                           */
/* replaces: subroutine sigmoid(ary, sm)  ref: generic/sea_breeze_diag.f90:457-481,  */
/*           seabreeze_diag_python.f90:287-311                                       */
/* -------------------------------------------------------------------------------- */
int sb_sigmoid_f64(sb_ctx *ctx, int nlons, int nlats, const double *ary, double *sm);
int sb_sigmoid_f32(sb_ctx *ctx, int nlons, int nlats, const float *ary, float *sm);
int sb_sigmoid_f64_dev(sb_ctx *ctx, int nlons, int nlats, const double *ary, double *sm, void *stream);
int sb_sigmoid_f32_dev(sb_ctx *ctx, int nlons, int nlats, const float *ary, float *sm, void *stream);

/* Latitude-band decomposition: the sigmoid needs GLOBAL statistics of sigma
   (ref: generic/sea_breeze_diag.f90:466-479).  Each band computes its own moments
   {count, mean, sum of squared deviations, min, max} (5 doubles, device memory), the
   host model all-gathers them (RCCL), and every following diag call on this context
   merges the gathered array (rank order, bit-identical on all ranks) instead of
   scanning its local sigma.  sb_use_gathered_moments(ctx, NULL, 0) switches back.     */
int sb_sigma_moments_f64_dev(sb_ctx *ctx, int nx, int ny, int halo, const double *sigma,
                             double *moments5, void *stream);
int sb_sigma_moments_f32_dev(sb_ctx *ctx, int nx, int ny, int halo, const float *sigma,
                             double *moments5, void *stream);
int sb_use_gathered_moments(sb_ctx *ctx, const double *gathered_dev, int nparts);

/* -------------------------------------------------------------------------------- */
/* get_edges -- coastline by binary 3x3 Sobel                                        */
/* replaces: get_edges(lsm, ci, nlons, nlats, coast)  ref: sobel.f90:19-89 (rule 0)  */
/*           get_edges(mask, icefrac, landfrac, halo_size)                           */
/*                                    ref: generic/sea_breeze_diag.f90:273-373 (rule 1) */
/* rule 0: land <=> lsm+ci > 0.4; rule 1: ice-aware two-branch mask (:325-337).      */
/* -------------------------------------------------------------------------------- */
int sb_get_edges_f64(sb_ctx *ctx, int nlons, int nlats, const double *lsm, const double *ci,
                     int rule, int bnd, double *coast);
int sb_get_edges_f32(sb_ctx *ctx, int nlons, int nlats, const float *lsm, const float *ci,
                     int rule, int bnd, float *coast);
int sb_get_edges_f64_dev(sb_ctx *ctx, int nlons, int nlats, const double *lsm, const double *ci,
                     int rule, int bnd, double *coast, void *stream);
int sb_get_edges_f32_dev(sb_ctx *ctx, int nlons, int nlats, const float *lsm, const float *ci,
                     int rule, int bnd, float *coast, void *stream);

/* -------------------------------------------------------------------------------- */
/* get_dist -- signed great-circle distance (km) to the nearest coast cell           */
/* replaces: get_dist(coast, mask, lon, lat, nlons, nlats, maxdist, cdist)           */
/*                                   ref: sobel.f90:91-193                           */
/*           get_dist(coast, landfrac, lon, lat, maxdist, cdist, halo_size)          */
/*                                   ref: generic/sea_breeze_diag.f90:375-455        */
/* kwin < 0: window half-width from the 70-degree grid spacing (sobel.f90:129-137);  */
/* kwin >= 0: fixed +-kwin cells (the generic/UM halo width, generic :422,425).      */
/* lon, lat: HOST pointers in every variant (tiny vectors; the window size is        */
/* derived from them on the host).                                                   */
/* Reach: kwin, or the half-width derived for kwin < 0, may be 0 ..                  */
/* SB_DIST_MAX_WINDOW cells (113 at 0.0135 degrees and maxdist = 180 km, the grids   */
/* sb_set_table_contrast is for); a wider window is refused with SB_ERR_ARG.  Any    */
/* nlons >= 1, also grids narrower than the window.                                  */
/* Single precision on km-scale grids: the coordinates are rounded to 24 bits before */
/* they are subtracted, as in the reference's own single-precision build.  At 0.0135 */
/* degrees spacing near 70 N that field differs from the double-precision one by     */
/* 5.6e-4 relative.  It is reproduced as it is, not more accurately: use the _f64    */
/* entry points for such grids.                                                      */
/* -------------------------------------------------------------------------------- */
#define SB_DIST_MAX_WINDOW 255
int sb_get_dist_f64(sb_ctx *ctx, int nlons, int nlats, const double *coast, const double *mask,
                    const double *lon, const double *lat, double maxdist, int kwin, double *cdist);
int sb_get_dist_f32(sb_ctx *ctx, int nlons, int nlats, const float *coast, const float *mask,
                    const float *lon, const float *lat, float maxdist, int kwin, float *cdist);
int sb_get_dist_f64_dev(sb_ctx *ctx, int nlons, int nlats, const double *coast, const double *mask,
                    const double *lon, const double *lat, double maxdist, int kwin, double *cdist,
                    void *stream);
int sb_get_dist_f32_dev(sb_ctx *ctx, int nlons, int nlats, const float *coast, const float *mask,
                    const float *lon, const float *lat, float maxdist, int kwin, float *cdist,
                    void *stream);
/* The half-width sb_get_dist would pick for kwin < 0. */
int sb_dist_window_f64(int nlons, int nlats, const double *lon, const double *lat, double maxdist, int *k);
int sb_dist_window_f32(int nlons, int nlats, const float *lon, const float *lat, float maxdist, int *k);

/* -------------------------------------------------------------------------------- */
/* get_edges, get_dist -- one latitude band of a multi-GPU run                       */
/* The coast setup of sb_get_edges_*(..., rule, SB_BND_GLOBAL) and                    */
/* sb_get_dist_*(..., kwin) for a rank that holds only its own rows, in the layout of */
/* the band step (sb_band_seabreeze_diag_*): every field is (nx+2*halo, ny+2*halo)    */
/* with the interior at (halo, halo); ny counts the band's own rows; south / north    */
/* != 0: the band touches that pole (meaning and row orientation as in                */
/* sb_fill_ghosts_*_dev).  lon has nx entries, lat ny+2*halo: one per frame row.      */
/* Read: on a cut side the north-south ghost rows next to the interior -- 1 row of    */
/* lsm and ci for the Sobel, kwin rows of coast (and their lat entries) for the       */
/* distance -- filled beforehand by sb_swap_bounds_* or the caller's own exchange.    */
/* Never read: the ghost rows on a pole side and their lat entries (the Sobel clamps  */
/* to the edge row, the window ends there, as on the globe), and the east-west ghost  */
/* columns (longitude is periodic by index arithmetic).  mask is read in the interior */
/* only.  Written: the interior of coast / cdist; their ghost cells are left to the   */
/* caller's swap_bounds.  Ghost rows are sources only, never computed as targets.     */
/* Result: the interior equals, bit for bit, rows r0 .. r1-1 of the whole-grid call   */
/* on the grid of which the frame's rows are rows r0-halo .. r1+halo-1, on the same   */
/* device and in the same precision: the Sobel's clamp at a pole row, the sweep-order */
/* reset and the sign included.  Both land rules; SB_BND_WRAPPER's column quirk is    */
/* not served.  south and north both set with halo = 0 is the whole grid.             */
/* SB_ERR_ARG: kwin < 0 (the derived half-width needs the global latitudes: use       */
/* sb_dist_window_* on those), kwin > SB_DIST_MAX_WINDOW, kwin > halo with a cut      */
/* side, halo < 1 with a cut side (edges), coast overlapping cdist.                   */
/* The _dev forms take device pointers for the fields and HOST pointers for lon, lat, */
/* and enqueue without synchronising; the coordinate tables are keyed on the content  */
/* of lon and of the lat entries that are read, as sb_get_dist_*_dev keeps them.      */
/* -------------------------------------------------------------------------------- */
int sb_band_get_edges_f64(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                          const double *lsm, const double *ci, int rule, double *coast);
int sb_band_get_edges_f32(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                          const float *lsm, const float *ci, int rule, float *coast);
int sb_band_get_edges_f64_dev(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                          const double *lsm, const double *ci, int rule, double *coast, void *stream);
int sb_band_get_edges_f32_dev(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                          const float *lsm, const float *ci, int rule, float *coast, void *stream);
int sb_band_get_dist_f64(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                         const double *coast, const double *mask, const double *lon, const double *lat,
                         double maxdist, int kwin, double *cdist);
int sb_band_get_dist_f32(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                         const float *coast, const float *mask, const float *lon, const float *lat,
                         float maxdist, int kwin, float *cdist);
int sb_band_get_dist_f64_dev(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                         const double *coast, const double *mask, const double *lon, const double *lat,
                         double maxdist, int kwin, double *cdist, void *stream);
int sb_band_get_dist_f32_dev(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                         const float *coast, const float *mask, const float *lon, const float *lat,
                         float maxdist, int kwin, float *cdist, void *stream);

/* -------------------------------------------------------------------------------- */
/* A band whose coast moves with the sea ice -- the coast distance of one latitude    */
/* band, kept up to date on the device without any exchange of coast                  */
/* Where the sea ice moves, a coupled run needs the band's cdist again at every       */
/* timestep.  sb_band_get_edges_* + sb_band_get_dist_* cost four ghost exchanges      */
/* (lsm, ci, coast, cdist) and the whole band.  Here the band keeps its coast as a    */
/* bit plane over its SOURCE rows (its own and kwin ghost rows on each cut side) and  */
/* forms the bits of the ghost source rows itself from kwin + 1 ghost rows of lsm and */
/* ci -- integer logic on land flags: exactly what the neighbour would have sent.  An */
/* ice call compares the new coast with the stored one in 64-cell words and computes  */
/* again only the (own row, 256-column tile) pairs a changed word can reach.  Per     */
/* timestep: one exchange going in (ci's ghost rows), one going out (cdist's).        */
/*                                                                                    */
/* sb_band_coast_open_*: geometry as sb_band_get_dist_*; lon (nx) and lat (ny+2*halo, */
/* one per frame row; entries beyond a pole are never read) are HOST pointers and are */
/* copied.  Allocates the context's band planes and may synchronise.  rule: the land  */
/* rule of sb_get_edges_* (0 or 1); the boundary is SB_BND_GLOBAL's.  incremental = 0:*/
/* every ice call computes the whole band (also taken where the grid is narrower than */
/* the window, 2*kwin + 1 > nx, kwin < 32).  SB_ERR_ARG: sb_band_get_dist's refusals  */
/* (kwin < 0, kwin > SB_DIST_MAX_WINDOW, bad sizes, NULL), kwin + 1 > halo with a cut */
/* side (the Sobel of the kwin-th ghost row reads the next one), rule outside 0..1,   */
/* already open.  south and north both set with halo = 0 is the whole grid of a       */
/* single-GPU host model.                                                             */
/*                                                                                    */
/* sb_band_ice_*_dev: lsm, ci, cdist are DEVICE frames in the band step's layout, in  */
/* the precision the coast was opened with (else SB_ERR_ARG; NULL, not open: same).   */
/* lsm and ci are read on the source rows and one row beyond them on cut sides; lsm   */
/* also gives the sign, read in the interior only.  Only the interior of cdist is     */
/* written: all of it by the first call, the marked tiles by later ones.  Enqueues on */
/* `stream` (NULL: the context's own) a clear of the marks, the delta kernel and the  */
/* distance kernel; no synchronisation, no download, no host compare (but: another    */
/* get_dist call on the context in between replaces the coordinate tables, and the    */
/* next ice call uploads them again).  Sets the search-radius hint to kwin + 1.       */
/* The caller's side of the contract:                                                 */
/*   * the content of lsm stands between calls (a changed lsm: close and reopen);     */
/*   * the interior of cdist is left alone between calls;                             */
/*   * every cut-side ghost row of lsm and ci is a real row of the globe, filled by   */
/*     sb_swap_bounds_* or the caller's exchange (no band thinner than halo);         */
/*   * the ghost cells of cdist are the caller's swap_bounds, as ever.                */
/* Result: after every call the interior of cdist equals, bit for bit,                */
/* sb_band_get_edges_* followed by sb_band_get_dist_*(kwin) of the same inputs -- by  */
/* their contract the rows of the whole-grid calls.  A band step after an ice call    */
/* needs nothing new: it finds the changed planes by content.                         */
/*                                                                                    */
/* sb_band_ice_report (synchronises the device): [0] ice calls since the open [1]     */
/* those after the first whose coast differed (-1 on the whole path) [2] (own row,    */
/* tile) pairs the last call marked (the first call: all) [3] pairs of the band.      */
/* sb_band_coast_close (synchronises the device) frees the planes.                    */
/* -------------------------------------------------------------------------------- */
int sb_band_coast_open_f64(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                           const double *lon, const double *lat, double maxdist, int kwin, int rule,
                           int incremental);
int sb_band_coast_open_f32(sb_ctx *ctx, int nx, int ny, int halo, int south, int north,
                           const float *lon, const float *lat, float maxdist, int kwin, int rule,
                           int incremental);
int sb_band_ice_f64_dev(sb_ctx *ctx, const double *lsm, const double *ci, double *cdist, void *stream);
int sb_band_ice_f32_dev(sb_ctx *ctx, const float *lsm, const float *ci, float *cdist, void *stream);
int sb_band_ice_report(sb_ctx *ctx, long long rep[4]);
int sb_band_coast_close(sb_ctx *ctx);

/* -------------------------------------------------------------------------------- */
/* search_radius -- every band cell's window radius, from mask alone                  */
/* no counterpart in the reference: the radius is the final nn of its expanding       */
/*           window, ref: generic/sea_breeze_diag.f90:188-214                         */
/* A setup product like get_dist: it changes when mask does (the ice mask), not per   */
/* step.  It tells, before any diag call, what sb_last_counters [0], [2], [3] would   */
/* say after one -- and that per cell: the ghost width a band run needs, which        */
/* contrast kernel the radii call for, where a window never finds a second class.     */
/* mask: (nx+2*halo, ny+2*halo), interior at (halo, halo); halo must be 0 unless      */
/* bnd == SB_BND_HALO.  Cells are classified as a diag call classifies them, in the   */
/* working precision: a band cell is one with !(|mask| > maxdist) (NaN: a band cell), */
/* land side is mask >= 0 (-0.0: land, NaN: sea side); with SB_BND_WRAPPER the last   */
/* row holds no band cell.  radius (nx, ny) int32, interior layout, may be NULL:      */
/*   0   not a band cell;                                                             */
/*   nn  the smallest nn >= 1 for which the cells (x+dx, y+dy), |dx|, |dy| <= nn,      */
/*       that exist under the boundary rule hold both classes (longitude periodic,    */
/*       latitude clamped; SB_BND_WRAPPER: offsets -1 and nx-1 both read column 0,    */
/*       the centre of a cell in the last column included; SB_BND_HALO: the frame);   */
/*   -1  no such nn up to the diag call's own cap -- nx+ny, and for SB_BND_HALO the    */
/*       frame's reach (ghost width plus distance to the nearest interior edge) if     */
/*       smaller: the cells a diag call returns NaN for and counts as one-class.       */
/* summary[4], may be NULL: [0] band cells, [1] those with a radius, [2] those with   */
/* -1, [3] the largest radius (0: none).  hist, optional (NULL or nhist == 0, else     */
/* nhist >= 2): hist[0] the -1 cells, hist[k] band cells of radius k for               */
/* 1 <= k < nhist-1, hist[nhist-1] those of radius >= nhist-1.                         */
/* The band forms take the band step's frame (sb_band_seabreeze_diag_*,               */
/* sb_band_get_dist_*): south / north as in sb_fill_ghosts_*; on cut sides the ghost  */
/* rows of mask are read as the caller filled them and bound the reach; ghost rows    */
/* beyond a pole and the east-west ghost columns are never read (clamp; periodic by   */
/* index).  With halo >= the whole grid's summary[3] a band's interior equals its     */
/* rows of the whole-grid SB_BND_GLOBAL plane.                                        */
/* No side effects on diag state: the call has a grow-only workspace of its own and   */
/* leaves planes, plans, lists, stored windows, counters and reports of the context   */
/* alone; a diag call after it enqueues and returns what it would have without it.    */
/* Host forms stage, synchronise and return the results.  The _dev forms take device  */
/* pointers for mask, radius, summary and hist, zero summary and hist themselves on   */
/* the stream, enqueue three kernels there and do not synchronise.                    */
/* SB_ERR_ARG: NULL mask; radius, summary and hist all NULL; bad sizes (rows wider     */
/* than 65535 cells included); halo != 0 with another rule than SB_BND_HALO;           */
/* nhist == 1.                                                                        */
/* -------------------------------------------------------------------------------- */
int sb_search_radius_f64(sb_ctx *ctx, int nx, int ny, int halo, int bnd, const double *mask, double maxdist,
                         int *radius, long long summary[4], long long *hist, int nhist);
int sb_search_radius_f32(sb_ctx *ctx, int nx, int ny, int halo, int bnd, const float *mask, float maxdist,
                         int *radius, long long summary[4], long long *hist, int nhist);
int sb_search_radius_f64_dev(sb_ctx *ctx, int nx, int ny, int halo, int bnd, const double *mask, double maxdist,
                         int *radius, long long summary[4], long long *hist, int nhist, void *stream);
int sb_search_radius_f32_dev(sb_ctx *ctx, int nx, int ny, int halo, int bnd, const float *mask, float maxdist,
                         int *radius, long long summary[4], long long *hist, int nhist, void *stream);
int sb_band_search_radius_f64(sb_ctx *ctx, int nx, int ny, int halo, int south, int north, const double *mask,
                         double maxdist, int *radius, long long summary[4], long long *hist, int nhist);
int sb_band_search_radius_f32(sb_ctx *ctx, int nx, int ny, int halo, int south, int north, const float *mask,
                         float maxdist, int *radius, long long summary[4], long long *hist, int nhist);
int sb_band_search_radius_f64_dev(sb_ctx *ctx, int nx, int ny, int halo, int south, int north, const double *mask,
                         double maxdist, int *radius, long long summary[4], long long *hist, int nhist, void *stream);
int sb_band_search_radius_f32_dev(sb_ctx *ctx, int nx, int ny, int halo, int south, int north, const float *mask,
                         float maxdist, int *radius, long long summary[4], long long *hist, int nhist, void *stream);

/* -------------------------------------------------------------------------------- */
/* get_edges -- UM vn10.7 layout (tdims_l), for curvilinear / rotated-pole grids      */
/* replaces: get_edges(mask, icefrac, landfrac)                                      */
/*           ref: UM/vn10.7/sea_breeze_diag.F90:328-446 (get_edges)                  */
/* landfrac, icefrac, coast: (nx+2*halo_i, ny+2*halo_j), interior at offset           */
/* (halo_i, halo_j); halo_i, halo_j >= 1.  The ghost cells of landfrac and icefrac    */
/* are filled by the caller (what the UM's swap_bounds of the mask amounts to,        */
/* :408-410).  The ice-aware rule (rule 1 of sb_get_edges_*, :390-403) is applied to  */
/* the interior and the one-cell ring round it, the Sobel is sb_get_edges_*'s         */
/* (:416-435), 0/1 goes into the interior of coast; its ghost cells are NOT touched   */
/* (the UM's closing swap_bounds, :440-442, is the caller's).                         */
/* -------------------------------------------------------------------------------- */
int sb_get_edges_um_f64(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                        const double *landfrac, const double *icefrac, double *coast);
int sb_get_edges_um_f32(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                        const float *landfrac, const float *icefrac, float *coast);
int sb_get_edges_um_f64_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                        const double *landfrac, const double *icefrac, double *coast, void *stream);
int sb_get_edges_um_f32_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                        const float *landfrac, const float *icefrac, float *coast, void *stream);

/* -------------------------------------------------------------------------------- */
/* get_dist -- UM vn10.7 layout, 2-D per-cell coordinates                             */
/* replaces: get_dist(landfrac, coast)                                               */
/*           ref: UM/vn10.7/sea_breeze_diag.F90:448-601 (get_dist)                   */
/* coast, cdist: (nx+2*halo_i, ny+2*halo_j); landfrac, true_lat, true_lon: interior   */
/* (nx, ny) fields, coordinates in degrees (trignometric_mod's true_latitude,         */
/* true_longitude, :523-524).  Window: +-halo_i columns x +-halo_j rows (:515-516),   */
/* 0 <= halo_i, halo_j <= 31 (else SB_ERR_ARG).  Sources (coast > 0) and targets are  */
/* interior cells only: the UM's scatter reaches into the halo but swap_bounds        */
/* discards those writes (:584-598), so there is no wrap and no clamp, and on a       */
/* multi-rank run every rank sees its own coast cells only (sb_tile_get_dist_um_*     */
/* below gives a rank its cells of the whole-domain field).  Only the interior of     */
/* cdist is written; its ghost cells are left to the caller's swap_bounds /           */
/* sb_fill_ghosts_*.  cdist == coast (in place, as the UM overwrites coast) works.    */
/* Arithmetic in the working precision with the UM's constants R = 6370.9989,         */
/* pi = 3.1415926, r2d = 180/pi, d2r = pi/180 (:509-512): the source longitude         */
/* l1 = d2r*(lon - 360) where lon > 180 (:552-556), the target's                      */
/* l2 = d2r*(r2d*lam1 - 360) where r2d*lam1 > 180, lam1 = d2r*lon (:560-564),         */
/* c = 2R atan2(sqrt(a), sqrt(1-a)) + 0.5, signed by landfrac > 0 (:565-574), and the  */
/* sweep-order reset |cdist| > 2*maxdist -> 12000 (:578; rows outer, columns inner)   */
/* applied to the minimum over sources swept at or before the target.  12000: no     */
/* coast cell in the window.  maxdist is a parameter of 180 km in the UM.             */
/* The _dev forms take device pointers for all five fields and enqueue without        */
/* synchronising; nothing is derived from the coordinates on the host.                */
/* The UM file cannot be compiled outside the UM: these entry points follow its text. */
/* -------------------------------------------------------------------------------- */
int sb_get_dist_um_f64(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                       const double *coast, const double *landfrac,
                       const double *true_lat, const double *true_lon,
                       double maxdist, double *cdist);
int sb_get_dist_um_f32(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                       const float *coast, const float *landfrac,
                       const float *true_lat, const float *true_lon,
                       float maxdist, float *cdist);
int sb_get_dist_um_f64_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                       const double *coast, const double *landfrac,
                       const double *true_lat, const double *true_lon,
                       double maxdist, double *cdist, void *stream);
int sb_get_dist_um_f32_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j,
                       const float *coast, const float *landfrac,
                       const float *true_lat, const float *true_lon,
                       float maxdist, float *cdist, void *stream);

/* -------------------------------------------------------------------------------- */
/* get_dist -- UM vn10.7 layout, the window stated apart from the ghost width         */
/* The field of sb_get_dist_um_* for a window of +-win_i columns x +-win_j rows,      */
/* 0 <= win_i, win_j <= SB_DIST_UM_MAX_WINDOW (113 cells at 0.0135 degrees and        */
/* maxdist = 180 km: the signed distance sb_set_table_contrast consumes on km-scale   */
/* rotated grids); a negative or wider window is refused with SB_ERR_ARG.  halo_i,    */
/* halo_j >= 0 describe the layout only: coast and cdist are                          */
/* (nx+2*halo_i, ny+2*halo_j) with the interior at (halo_i, halo_j), and the window   */
/* may be wider or narrower than the ghost width.  Everything else is                 */
/* sb_get_dist_um_*'s rule: interior sources and targets only (no wrap, no clamp),    */
/* the UM's constants and both longitude corrections, the sweep-order reset on the    */
/* minimum over sources swept at or before the target, 12000 where the window holds   */
/* no coast, only the interior of cdist written, cdist == coast allowed; the _dev     */
/* forms enqueue without synchronising and derive nothing on the host.                */
/* With win_i == halo_i <= 31 and win_j == halo_j <= 31 the call is                   */
/* sb_get_dist_um_*'s, bit for bit.  Any other window goes to a kernel that, in       */
/* double precision, takes sin((phi_s - phi_t)/2) on the difference as the UM writes  */
/* it: at km-scale spacing the fields of the two kernels differ by up to 1e-12        */
/* relative, the wide one being the closer to the UM's own arithmetic.                */
/* -------------------------------------------------------------------------------- */
#define SB_DIST_UM_MAX_WINDOW 255
int sb_get_dist_um_win_f64(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j,
                       const double *coast, const double *landfrac,
                       const double *true_lat, const double *true_lon,
                       double maxdist, double *cdist);
int sb_get_dist_um_win_f32(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j,
                       const float *coast, const float *landfrac,
                       const float *true_lat, const float *true_lon,
                       float maxdist, float *cdist);
int sb_get_dist_um_win_f64_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j,
                       const double *coast, const double *landfrac,
                       const double *true_lat, const double *true_lon,
                       double maxdist, double *cdist, void *stream);
int sb_get_dist_um_win_f32_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j,
                       const float *coast, const float *landfrac,
                       const float *true_lat, const float *true_lon,
                       float maxdist, float *cdist, void *stream);

/* -------------------------------------------------------------------------------- */
/* get_edges, get_dist -- UM layout, one tile of a 2-D domain decomposition           */
/* The UM runs on a 2-D decomposition: every rank holds a rectangular tile on tdims_l */
/* with ghost cells that swap_bounds fills.  sb_get_edges_um_* / sb_get_dist_um_win_* */
/* follow the UM's text -- interior sources only -- so on such a run their field      */
/* depends on how the domain was cut.  The tile calls give a rank its cells of the    */
/* WHOLE-DOMAIN field from its own frame alone; the library exchanges nothing.        */
/* Every field -- landfrac_l, icefrac_l, coast_l, cdist_l and the two coordinate      */
/* frames true_lat_l, true_lon_l (degrees) -- is (nx+2*halo_i, ny+2*halo_j) with the  */
/* tile's interior at (halo_i, halo_j).  The caller fills the ghost cells of the      */
/* inputs once with its own swap_bounds (the coordinates are static).  sides: a sum   */
/* of SB_TILE_* bits.  A side whose bit is set ends at the domain's edge: nothing     */
/* beyond it is a source and nothing beyond it is written, which is what the          */
/* whole-domain calls do at their rim.  A side whose bit is clear is a cut: the ghost */
/* cells beyond it are a neighbour's cells.  (Where the domain ends inside the reach  */
/* of a cut side -- a neighbour narrower than ext or the window -- the ghost cells    */
/* beyond the domain are the caller's: coast_l must hold 0 there.)                    */
/*                                                                                    */
/* sb_tile_get_edges_um_*: the ice-aware rule and the Sobel of sb_get_edges_um_*;     */
/* 0/1 goes into the interior of coast_l and into the ghost cells within ext_i        */
/* columns / ext_j rows of it on every cut side, so a rank forms the coast of the     */
/* ghost cells its distance window reads (ext = win) instead of receiving it.  Every  */
/* other cell of coast_l is left untouched.  A cut side needs halo >= ext + 1 (the    */
/* Sobel reads the ring one cell beyond the last cell it writes), an edge side        */
/* halo >= 1, the ring sb_get_edges_um_* reads too.  coast_l must not overlap         */
/* landfrac_l or icefrac_l.                                                           */
/*                                                                                    */
/* sb_tile_get_dist_um_*: sb_get_dist_um_win_*(win_i, win_j)'s rule with one change:  */
/* sources are the coast cells (coast_l > 0) of the interior AND of the ghost cells    */
/* within win_i columns / win_j rows on every cut side, their coordinates read from   */
/* the coordinate frames.  Targets are interior cells only; only the interior of      */
/* cdist_l is written; the sign is landfrac_l > 0 of the interior.  cdist_l == coast_l */
/* works (the coast bit plane is formed in a launch of its own).  A cut side needs    */
/* halo >= win; the window is 0 .. SB_DIST_UM_MAX_WINDOW each way.  The arithmetic is */
/* always that of the wide kernel of sb_get_dist_um_win_*: both sines taken on the    */
/* difference as written.  Whether a source is swept at or before a target is decided */
/* on row and column differences, so the sweep-order reset survives the cut.          */
/*                                                                                    */
/* Result: the interior of cdist_l equals, bit for bit, the tile's cells of           */
/* sb_get_edges_um_* followed by sb_get_dist_um_win_*(win_i, win_j) on the domain of  */
/* which the frame is a cut-out -- same device, same precision -- wherever that call  */
/* takes its wide kernel: any window that differs from its layout halo or exceeds 31. */
/* Against a whole-domain call with win == halo <= 31 (sb_get_dist_um_*'s kernel) the  */
/* fields differ by the two kernels' documented difference: up to 1e-12 relative in   */
/* double, 2e-6 in single precision.  All four bits set is the whole domain.          */
/* SB_ERR_ARG, with nothing enqueued and nothing written: bad sizes, sides outside    */
/* 0 .. 15, ext or win negative or beyond 255, a halo too small as stated above, NULL, */
/* coast_l overlapping an input of the edges call.                                    */
/* The _dev forms take device pointers for every field and enqueue on `stream` (NULL: */
/* the context's own): one kernel (edges), two (distance).  They do not synchronise,  */
/* download or derive anything on the host.  A tile that follows moving sea ice:      */
/* sb_um_tile_coast_open_* / sb_um_tile_ice_* below.  Not served: the exchange itself.*/
/* -------------------------------------------------------------------------------- */
#define SB_TILE_WEST 1   /* the tile's first column is the domain's first column */
#define SB_TILE_EAST 2   /* the tile's last column is the domain's last column */
#define SB_TILE_SOUTH 4  /* the tile's first row is the domain's first row */
#define SB_TILE_NORTH 8  /* the tile's last row is the domain's last row */
int sb_tile_get_edges_um_f64(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int ext_i, int ext_j, int sides,
                       const double *landfrac_l, const double *icefrac_l, double *coast_l);
int sb_tile_get_edges_um_f32(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int ext_i, int ext_j, int sides,
                       const float *landfrac_l, const float *icefrac_l, float *coast_l);
int sb_tile_get_edges_um_f64_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int ext_i, int ext_j, int sides,
                       const double *landfrac_l, const double *icefrac_l, double *coast_l, void *stream);
int sb_tile_get_edges_um_f32_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int ext_i, int ext_j, int sides,
                       const float *landfrac_l, const float *icefrac_l, float *coast_l, void *stream);
int sb_tile_get_dist_um_f64(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j, int sides,
                       const double *coast_l, const double *landfrac_l,
                       const double *true_lat_l, const double *true_lon_l,
                       double maxdist, double *cdist_l);
int sb_tile_get_dist_um_f32(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j, int sides,
                       const float *coast_l, const float *landfrac_l,
                       const float *true_lat_l, const float *true_lon_l,
                       float maxdist, float *cdist_l);
int sb_tile_get_dist_um_f64_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j, int sides,
                       const double *coast_l, const double *landfrac_l,
                       const double *true_lat_l, const double *true_lon_l,
                       double maxdist, double *cdist_l, void *stream);
int sb_tile_get_dist_um_f32_dev(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j, int sides,
                       const float *coast_l, const float *landfrac_l,
                       const float *true_lat_l, const float *true_lon_l,
                       float maxdist, float *cdist_l, void *stream);

/* -------------------------------------------------------------------------------- */
/* a UM-layout coast that moves with the sea ice -- get_edges_um + get_dist_um_win,   */
/* kept up to date on the device, incrementally                                       */
/* The UM copy rebuilds its land mask from icefrac inside the timestep routine and    */
/* runs get_edges and get_dist on it (ref: UM/vn10.7/sea_breeze_diag.F90:384-445): the*/
/* coast moves with the ice at every model step.  sb_get_edges_um_* +                 */
/* sb_get_dist_um_win_* per step cost the whole interior, whatever changed.  Here the */
/* context keeps the interior's coast as a bit plane of its own; an ice call compares */
/* the new coast with the stored one in 64-cell words and computes again only the     */
/* workgroups of the distance kernels (4 rows x 64 columns) a changed word can reach  */
/* through the window.                                                                */
/*                                                                                    */
/* sb_um_coast_open_*: geometry as sb_get_dist_um_win_*: landfrac_l, icefrac_l and    */
/* cdist_l of the ice calls are (nx+2*halo_i, ny+2*halo_j) frames with the interior   */
/* at (halo_i, halo_j); halo_i, halo_j >= 1 (the Sobel reads the one-cell ring, as in */
/* sb_get_edges_um_*); the window is +-win_i x +-win_j, each 0 ..                     */
/* SB_DIST_UM_MAX_WINDOW, stated apart from the ghost width.  true_lat, true_lon      */
/* (nx, ny), degrees, are HOST pointers and are copied to the device.  Allocates the  */
/* context's UM planes and may synchronise.  incremental = 0: every ice call computes */
/* the whole interior with sb_get_edges_um's and sb_get_dist_um_win's kernels (for    */
/* A/B runs, and for runs in which every tile changes).  SB_ERR_ARG: bad sizes, a     */
/* halo below 1, a window outside 0 .. 255, NULL, already open.  The UM state is      */
/* independent of the stream's (sb_diag_stream_coast), the band's                     */
/* (sb_band_coast_open_*) and a UM tile's (sb_um_tile_coast_open_*) moving coasts:    */
/* one context may hold all four.  On a decomposed run the interior-only rule makes   */
/* this field depend on the cut: a rank of such a run opens the tile coast instead.   */
/*                                                                                    */
/* The rule is the UM's ice-aware land rule (:390-403) and sb_get_dist_um_win_*'s     */
/* distance rule in every respect: interior sources and targets only, no wrap, no     */
/* clamp, both longitude corrections, the sweep-order reset, 12000 where the window   */
/* holds no coast.  The sign comes from landfrac_l > 0, read in the interior of the   */
/* frame (sb_get_dist_um_* takes an interior (nx, ny) landfrac: the same values, read */
/* here through the frame's pitch and offset).                                        */
/*                                                                                    */
/* sb_um_ice_*_dev: landfrac_l, icefrac_l, cdist_l are DEVICE frames in the precision */
/* the coast was opened with (else SB_ERR_ARG; NULL, not open: same).  Enqueues on    */
/* `stream` (NULL: the context's own) one clear of [marks | changed-word counter],    */
/* the delta kernel and the distance kernel; no synchronisation, no download, no host */
/* compare.  Only the interior of cdist_l is written: all of it by the first call,    */
/* the marked workgroups by later ones.  The caller's side of the contract:           */
/*   * the content of landfrac_l stands between calls (a changed landfrac: close and  */
/*     reopen);                                                                       */
/*   * the interior of cdist_l is left alone between calls;                           */
/*   * the one-cell ring of landfrac_l and icefrac_l is filled (swap_bounds);         */
/*   * the ghost cells of cdist_l are the caller's swap_bounds, as ever.              */
/* sb_um_ice_f64 / _f32 take HOST frames: they stage all three (cdist_l too: what the */
/* call before left in its interior stands where nothing is marked), synchronise and  */
/* return the interior of cdist_l; its ghost cells are untouched.                     */
/* Result: after every call the interior of cdist_l equals, bit for bit,              */
/* sb_get_edges_um_* followed by sb_get_dist_um_win_*(win_i, win_j) of the same       */
/* inputs -- sb_get_dist_um_*'s field where win == halo <= 31.  A                     */
/* sb_seabreeze_diag_um_* call after an ice call needs nothing new: it finds the      */
/* changed band planes by content.  The coast bit plane is the context's own, not the */
/* scratch plane other get_dist calls overwrite: any other coast call on the context  */
/* between two ice calls leaves the next ice call exact.                              */
/*                                                                                    */
/* sb_um_ice_report (synchronises the device): [0] ice calls since the open [1]       */
/* those after the first whose coast differed (-1 on the whole path) [2] workgroup    */
/* tiles the last call marked (the first call: all) [3] tiles of the grid,            */
/* ceil(ny/4) * ceil(nx/64).  sb_um_coast_close (synchronises the device) frees the   */
/* planes.                                                                            */
/* -------------------------------------------------------------------------------- */
int sb_um_coast_open_f64(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j,
                         const double *true_lat, const double *true_lon, double maxdist, int incremental);
int sb_um_coast_open_f32(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j,
                         const float *true_lat, const float *true_lon, float maxdist, int incremental);
int sb_um_ice_f64_dev(sb_ctx *ctx, const double *landfrac_l, const double *icefrac_l, double *cdist_l, void *stream);
int sb_um_ice_f32_dev(sb_ctx *ctx, const float *landfrac_l, const float *icefrac_l, float *cdist_l, void *stream);
int sb_um_ice_f64(sb_ctx *ctx, const double *landfrac_l, const double *icefrac_l, double *cdist_l);
int sb_um_ice_f32(sb_ctx *ctx, const float *landfrac_l, const float *icefrac_l, float *cdist_l);
int sb_um_ice_report(sb_ctx *ctx, long long rep[4]);
int sb_um_coast_close(sb_ctx *ctx);

/* -------------------------------------------------------------------------------- */
/* one tile of the UM's 2-D decomposition whose coast moves with the sea ice --       */
/* sb_tile_get_edges_um + sb_tile_get_dist_um, kept up to date on the device,         */
/* incrementally                                                                      */
/* The UM runs decomposed and rebuilds its mask from icefrac at every timestep.       */
/* sb_um_ice_* follows the ice but keeps the interior-only rule, so its field depends */
/* on the cut; the tile setup calls above give the whole-domain field but cost the    */
/* whole tile per call.  Here the context keeps the coast of the tile's SOURCE        */
/* rectangle as a bit plane of its own; an ice call compares the new coast with the   */
/* stored one in 64-cell words and computes again only the workgroups of the tile     */
/* distance kernel (4 rows x 64 columns of the interior) a changed word can reach     */
/* through the window -- a changed word of a neighbour's ghost cells included.        */
/*                                                                                    */
/* sb_um_tile_coast_open_*: every field of the ice calls is the rank's frame,         */
/* (nx+2*halo_i, ny+2*halo_j) with the interior at (halo_i, halo_j), as in the tile   */
/* calls.  beyond[4]: the number of DOMAIN cells beyond the tile's west, east, south  */
/* and north side; 0 says that side is the domain's edge, any value >= the window     */
/* that the window never sees the domain's end.  Sources are the coast cells of       */
/* [-eW, nx+eE) x [-eS, ny+eN) in interior coordinates with e* = min(win, beyond*):   */
/* the tile calls' reach with the domain's end stated, so a neighbour narrower than   */
/* the window needs nothing of the caller.  Every side needs halo >= e* + 1 (the      */
/* Sobel of the outermost source cell reads one cell further; on an edge side that is */
/* the one-cell ring sb_get_edges_um_* reads).  Ghost cells beyond the domain hold    */
/* what the whole-domain frame's ring holds there: the caller's, as at the            */
/* whole-domain call's rim.  true_lat_l, true_lon_l (degrees) are HOST frames and are */
/* copied to the device.  Allocates the context's tile planes and may synchronise.    */
/* incremental = 0: every ice call computes the whole tile with the tile setup calls' */
/* kernels (for A/B runs, and for runs in which every workgroup changes).  The state  */
/* stands beside sb_um_coast_open_*'s: one context may hold both, and the stream's    */
/* and the band's moving coasts as well.                                              */
/*                                                                                    */
/* sb_um_tile_ice_*_dev: landfrac_l, icefrac_l, cdist_l are DEVICE frames in the      */
/* precision the coast was opened with.  Enqueues on `stream` (NULL: the context's    */
/* own) one clear of [marks | changed-word counter], the delta kernel and the         */
/* distance kernel; no synchronisation, no download, no host compare.  Only the       */
/* interior of cdist_l is written: all of it by the first call, the marked workgroups */
/* by later ones.  The caller's side of the contract:                                 */
/*   * the content of landfrac_l (ghost cells within e* + 1 included) and the         */
/*     coordinates stand while the coast is open;                                     */
/*   * swap_bounds refreshes the ghost cells of icefrac_l within e* + 1 of the        */
/*     interior before every ice call;                                                */
/*   * the interior of cdist_l is left alone between calls;                           */
/*   * the ghost cells of cdist_l are the caller's swap_bounds, as ever.              */
/* sb_um_tile_ice_f64 / _f32 take HOST frames: they stage all three (cdist_l too),    */
/* synchronise and return the interior of cdist_l; its ghost cells are untouched.     */
/* Result: after every call the interior of cdist_l equals, bit for bit, the tile's   */
/* cells of sb_get_edges_um_* followed by sb_get_dist_um_win_*(win_i, win_j) on the   */
/* domain of which the frame is a cut-out -- same device, same precision -- wherever  */
/* that call takes its wide kernel (any window that differs from its layout halo or   */
/* exceeds 31); against its other kernel the documented 1e-12 / 2e-6 applies, as for  */
/* the tile calls.  The arithmetic is always the wide kernel's.  The coast bit plane  */
/* is the context's own: any other coast call on the context between two ice calls    */
/* leaves the next ice call exact.                                                    */
/* SB_ERR_ARG, with nothing enqueued, nothing written and the state untouched: bad    */
/* sizes, a window outside 0 .. 255, a negative beyond, a halo below e* + 1 on any    */
/* side, NULL, already open (open); not open, the other precision, NULL (ice calls,   */
/* report, close).                                                                    */
/*                                                                                    */
/* sb_um_tile_ice_report (synchronises the device): sb_um_ice_report's four fields -- */
/* [0] ice calls since the open [1] those after the first whose coast differed (-1 on */
/* the whole path) [2] workgroup tiles the last call marked (the first call: all)     */
/* [3] tiles of the interior, ceil(ny/4) * ceil(nx/64).  sb_um_tile_coast_close       */
/* (synchronises the device) frees the planes.                                        */
/* -------------------------------------------------------------------------------- */
int sb_um_tile_coast_open_f64(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j, const int beyond[4],
                              const double *true_lat_l, const double *true_lon_l, double maxdist, int incremental);
int sb_um_tile_coast_open_f32(sb_ctx *ctx, int nx, int ny, int halo_i, int halo_j, int win_i, int win_j, const int beyond[4],
                              const float *true_lat_l, const float *true_lon_l, float maxdist, int incremental);
int sb_um_tile_ice_f64_dev(sb_ctx *ctx, const double *landfrac_l, const double *icefrac_l, double *cdist_l, void *stream);
int sb_um_tile_ice_f32_dev(sb_ctx *ctx, const float *landfrac_l, const float *icefrac_l, float *cdist_l, void *stream);
int sb_um_tile_ice_f64(sb_ctx *ctx, const double *landfrac_l, const double *icefrac_l, double *cdist_l);
int sb_um_tile_ice_f32(sb_ctx *ctx, const float *landfrac_l, const float *icefrac_l, float *cdist_l);
int sb_um_tile_ice_report(sb_ctx *ctx, long long rep[4]);
int sb_um_tile_coast_close(sb_ctx *ctx);

/* -------------------------------------------------------------------------------- */
/* swap_bounds -- ghost-cell fill of one latitude band of a multi-GPU run            */
/* replaces: subroutine swap_bounds(field, halo_size)                                */
/*           ref: generic/halo_exchange_mod.f90:12-17 (an empty stub; the UM copy    */
/*           calls a real one, ref: UM/vn10.7/sea_breeze_diag.F90:408-410)            */
/* One process per GPU owns `ny` rows x full longitude circles inside a frame of     */
/* `halo` ghost cells: field is (nx+2*halo, ny+2*halo) in DEVICE memory.  North and   */
/* south ghost rows are exchanged with the band neighbours (ranks rank-1 / rank+1)    */
/* by ncclSend/ncclRecv in one group over RCCL (xGMI); bands at rank 0 / nranks-1     */
/* replicate their pole-side edge row; E-W ghost columns are the periodic wrap.       */
/* Without sb_comm_init the context is a single band owning the globe (local fill).  */
/* librccl.so is opened on demand by sb_comm_get_unique_id / sb_comm_init.           */
/*   rank 0:    sb_comm_get_unique_id(id);  -- hand the 128 bytes to every rank       */
/*   every rank: sb_comm_init(ctx, id, rank, nranks);                                 */
/* sb_allgather_moments_dev: the 5-double sigma moments of every band, in rank order, */
/* for sb_use_gathered_moments (ncclAllGather).                                       */
/* -------------------------------------------------------------------------------- */
int sb_comm_get_unique_id(unsigned char id[128]);
int sb_comm_init(sb_ctx *ctx, const unsigned char id[128], int rank, int nranks);
int sb_comm_finalize(sb_ctx *ctx);
int sb_swap_bounds_f64_dev(sb_ctx *ctx, double *field, int nx, int ny, int halo, void *stream);
int sb_swap_bounds_f32_dev(sb_ctx *ctx, float *field, int nx, int ny, int halo, void *stream);
int sb_allgather_moments_dev(sb_ctx *ctx, const double *mine5, double *gathered, void *stream);
/* The local part of sb_swap_bounds_*_dev on its own, for a host model that moves the north-south ghost rows with its
   own message passing (ref: generic/halo_exchange_mod.f90:12-17, where swap_bounds stands for "various routines about
   communications across processors"): the east-west ghost columns of every row -- ghost rows included -- become the
   periodic wrap, and a band that touches a pole (south / north != 0) replicates its edge row into the ghost rows on
   that side first.  No communicator is needed or used.                                                          */
int sb_fill_ghosts_f64_dev(sb_ctx *ctx, double *field, int nx, int ny, int halo, int south, int north, void *stream);
int sb_fill_ghosts_f32_dev(sb_ctx *ctx, float *field, int nx, int ny, int halo, int south, int north, void *stream);
/* One seabreeze_diag step of a latitude band, device pointers, as sb_seabreeze_diag_*_dev with
   bnd = SB_BND_HALO -- plus the band's communication: the sigma moments are reduced over all
   bands and theta's ghost cells are filled (swap_bounds) inside the call, on the context's
   second stream, while the kernels that need neither (k_scan, k_wind) run on `stream`.
   mask, z, sigma must already carry their ghost cells (static: exchange them once).       */
int sb_band_seabreeze_diag_f64_dev(sb_ctx *ctx, double timestep_s, int timestep_number, int nx, int ny, int nz,
                                   int halo, const double *p, const double *u, const double *v, double *theta,
                                   const double *mask, const double *z, const double *sigma, double *windspeed,
                                   double *winddir, double *thc, double *sb_con, const sb_tunables *tun,
                                   void *stream);
int sb_band_seabreeze_diag_f32_dev(sb_ctx *ctx, float timestep_s, int timestep_number, int nx, int ny, int nz,
                                   int halo, const float *p, const float *u, const float *v, float *theta,
                                   const float *mask, const float *z, const float *sigma, float *windspeed,
                                   float *winddir, float *thc, float *sb_con, const sb_tunables *tun,
                                   void *stream);

/* Host-pointer forms of the two for host models whose fields live in host memory (what the Fortran
   modules fortran/halo_exchange_mod.f90 and fortran/sea_breeze_diag_mod.F90 bind): the arrays are staged
   through device buffers of the context, the exchange runs over RCCL between the devices, the results come
   back.  sb_swap_bounds_* replaces swap_bounds(field, halo_size), ref: generic/halo_exchange_mod.f90:12-17
   and its call sites generic/sea_breeze_diag.f90:342,371; theta's ghost cells are filled on return from
   sb_band_seabreeze_diag_*.                                                                          */
int sb_swap_bounds_f64(sb_ctx *ctx, double *field, int nx, int ny, int halo);
int sb_swap_bounds_f32(sb_ctx *ctx, float *field, int nx, int ny, int halo);
int sb_band_seabreeze_diag_f64(sb_ctx *ctx, double timestep_s, int timestep_number, int nx, int ny, int nz,
                               int halo, const double *p, const double *u, const double *v, double *theta,
                               const double *mask, const double *z, const double *sigma, double *windspeed,
                               double *winddir, double *thc, double *sb_con, const sb_tunables *tun);
int sb_band_seabreeze_diag_f32(sb_ctx *ctx, float timestep_s, int timestep_number, int nx, int ny, int nz,
                               int halo, const float *p, const float *u, const float *v, float *theta,
                               const float *mask, const float *z, const float *sigma, float *windspeed,
                               float *winddir, float *thc, float *sb_con, const sb_tunables *tun);
/* rank of this context's band and the number of bands; nranks = 0 without a communicator */
int sb_comm_rank(sb_ctx *ctx, int *rank, int *nranks);

/* -------------------------------------------------------------------------------- */
/* device memory for host models that keep their fields resident between calls      */
/* (Fortran: type(c_ptr) handles passed to the _dev entry points); upload and         */
/* download synchronise.                                                              */
/* -------------------------------------------------------------------------------- */
int sb_device_malloc(sb_ctx *ctx, size_t nbytes, void **dptr);
int sb_device_free(sb_ctx *ctx, void *dptr);
int sb_device_upload(sb_ctx *ctx, void *dst_dev, const void *src_host, size_t nbytes);
int sb_device_download(sb_ctx *ctx, void *dst_host, const void *src_dev, size_t nbytes);

/* -------------------------------------------------------------------------------- */
/* get_threads  ref: sobel.f90:195-206 (OpenMP thread count there; here the number   */
/* of visible HIP devices -- the unit of parallelism a caller can spread bands over) */
/* -------------------------------------------------------------------------------- */
int sb_get_threads(int *nt);

#ifdef __cplusplus
}
#endif
#endif /* SEABREEZE_HIP_H */
