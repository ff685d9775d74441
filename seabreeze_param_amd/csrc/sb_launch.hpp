// sb_launch.hpp -- host-side launcher declarations shared by the kernel files and the C ABI.
#pragma once
#include "sb_device.hpp"
#include "sb_diag_plan.hpp"
#include "sb_dist_plan.hpp"
#include "sb_ice_plan.hpp"

#define SB_STATS_MAX_BLOCKS 2048
#define SB_DIST_TY 4                // rows per k_dist tile
#define SB_PROF_EVENTS (2 * SB_PROF_KERNELS)
#ifndef SB_WIND_UN
#define SB_WIND_UN 8                // levels of a p column in flight per lane of k_wind
#endif
#ifndef SB_WIND_WGS_PER_CU
#define SB_WIND_WGS_PER_CU 4        // persistent 256-thread workgroups of k_wind per compute unit (= its waves per SIMD:
                                    // the gather is bound by the memory system from two workgroups per CU upwards,
                                    // tools/probe_gather.hip, and 128 registers keep the update code free of spills)
#endif
#ifndef SB_WIND_UN_F32
#define SB_WIND_UN_F32 14           // ... and the two constants in single precision: a load brings half the bytes, so a wave
#endif                              // keeps more of them in flight and the update's registers (57) allow eight waves per SIMD.
#ifndef SB_WIND_WGS_PER_CU_F32      // Measured on one box (k_wind, 5120x3840x56 fp32): 8 loads x 4 workgroups 138.6 us,
#define SB_WIND_WGS_PER_CU_F32 8    // 16 x 4 131.8, 16 x 6 126.4, 8 x 8 120.3, 14 x 7 119.1, 19 x 8 117.6, 28 x 8 118.1,
#endif                              // 14 x 8 114.3-118.1; 2560x1920x56 fp32: 50.1 -> 39.7 us
#ifndef SB_WIND_UN_PAIR
#define SB_WIND_UN_PAIR 7           // 16-byte loads (two cells x two levels each) in flight per lane of k_wind's paired walk.
#endif                              // Measured (k_wind, 2560x1920x56 fp64, tools/wind_pairs_ab.py): 4 loads 63.3-63.9 us, 7 loads
                                    // 61.1-61.4, 14 loads 72.8-73.6 (128 registers, spills); the one-cell walk 71.7-72.6

// The device-wide summed-area tables of sb_set_table_contrast (sb_table_kernels.hip) over the (nxh, nyh) frame: inclusive
// 2-D prefix sums of t0 in fixed point with SB_TAB_FB fractional bits (A), of the same over land-side cells (L) and of
// the land-side count (C); S*: per block of SB_TAB_RB rows and per column the block's sum of the row-prefixed values,
// which the row pass leaves for the column pass.  Unsigned: the sums wrap, the differences a query forms do not.
//   Format.  A window of (2R+1)^2 values below 2^11 K must fit 63 bits: (2R+1)^2 2^(11+F) < 2^63.  A value is rounded
// once, by at most 2^-(F+1) K, so a window mean and hence thc moves by at most 2 2^-(F+1) K, which sb_con amplifies by at
// most 11/0.75 (scale_wind <= thr_wind / 1, d scale_thc / d thc <= 1 / thr_thc); the double-precision tests allow
// 1e-7 max(|ref|, 1e-2), so that bound must stay below 1e-9.  F = 36: reach R = 127 (255^2 = 65025 < 2^16), bound
// 2^-36 11/0.75 = 2.1e-10, and every single-precision value of magnitude >= 2^-12 is exact.  One format for both precisions.
#define SB_TAB_FB 36
#define SB_TAB_REACH 127
#define SB_TAB_RB 16                // rows per workgroup of the row pass = rows of a block of S
static_assert((2 * SB_TAB_REACH + 1) * (2 * SB_TAB_REACH + 1) < (1 << (63 - 11 - SB_TAB_FB)), "a window at the reach must fit 63 bits");
static_assert((2 * SB_TAB_REACH + 3) * (2 * SB_TAB_REACH + 3) >= (1 << (63 - 11 - SB_TAB_FB)), "the reach is the largest the format holds");
#include "sb_table_cache.hpp"
// With sb_set_table_window_cache in effect (W != nullptr) a call whose planes stand builds A, L, SA and SL alone and takes
// every band cell's window from W (sb_table_cache.hpp); the three kernels agree on that by one predicate over the same words:
// force (the host's half) || *gen == call_id (k_scan of this call found a plane changed).  rep: device words of
// sb_table_cache_report: [0] calls that searched (the row pass counts them); from SB_TAB_REP_HDR on two words per wave of
// the query, the band cells of this call it answered from W and those it searched (every wave writes its own, the host
// adds them up).
#define SB_TAB_REP_HDR 2
#define SB_TAB_QUERY_WAVES_PER_CU 16    // the query's grid: 4 workgroups of 4 waves per compute unit
struct SbTables {
    unsigned long long *A, *L, *SA, *SL;
    unsigned *C, *SC;
    unsigned *W;                    // nx * ny words, or nullptr: the cache is not in effect, C is built and searched every call
    unsigned *rep;
    const int *gen;                 // DiagJob::plan_gen
    int call_id, force, rep_reset;  // rep_reset: the first such call since the switch was turned on, rep[0] starts over
};
__device__ __forceinline__ bool sb_tab_fill(const SbTables &tb) { return !tb.W || tb.force || *tb.gen == tb.call_id; }

// The guard for missing and non-finite temperatures (sb_set_nonfinite_guard; sb_guard_kernels.hip, SbGuardPlan): two bit
// planes of the (nxh, nyh) frame in the layout of bandbits -- bad cells, later the tainted band cells; the longitude pass'
// result -- and the device words of sb_guard_report: [0] bad frame cells of this call, [1] band cells it computed again,
// [2] calls that found a bad cell since the switch was set; the workgroups' ticket and their partial counts.
#define SB_GUARD_MAX_WGS 2048
#define SB_GUARD_REP_TICKET 4
#define SB_GUARD_REP_PART 8
#define SB_GUARD_REP_WORDS (SB_GUARD_REP_PART + SB_GUARD_MAX_WGS)
struct SbGuard {
    uint64_t *bad, *taint;
    unsigned *rep;
    int rep_reset;                  // the first such call since the switch was set: rep[2] starts over
    void *stash_ws, *stash_wd;      // sb_set_nonfinite_guard_bands: (nx, ny) of T, ws / wd of the tainted band cells as they were
                                    // ahead of a contrast kernel that applies the update itself; else nullptr
};

// Everything of the context a diag launch needs besides the job itself.
struct SbLaunchCtx {
    hipStream_t stream;             // every kernel of the call is enqueued here
    hipEvent_t *prof;               // SB_PROF_EVENTS timing events of this call, or nullptr
    unsigned *prof_mask;            // bit k set: kernel k was launched (and its event pair recorded) in this call
    Moments *partials;              // per-workgroup reduction partials
    void *stats;                    // sigmoid scalars (4 x T)
    const Moments *gathered;        // per-band sigma moments to merge instead of scanning sigma, or nullptr
    int ngathered;
    Moments *moments_out;           // band step: this band's sigma moments go here (k_scan's last workgroup merges them) ...
    hipEvent_t moments_event;       // ... and this event is recorded behind k_scan, or nullptr
    int *stats_ticket;              // ... with this device word (zero between launches) as the workgroups' ticket
    int ncu;                        // compute units (k_scan and the contrast kernel run one workgroup per CU)
    int wind_pairs;                 // sb_set_wind_pairs: k_wind may take its paired walk where the call is eligible
    int *wind_pairs_ran;            // ... and launch_wind notes here whether it did (host memory), or nullptr
    SbTables tables;                // a call whose plan builds the device-wide tables (SbDiagPlan::table)
    SbGuardPlan guard;              // where the guard's launches go between the plan's steps (on == false: nowhere) ...
    SbGuard guard_ws;               // ... and their workspace
};

template <typename T>
hipError_t sb_launch_stats(const T *ary, int nx, int ny, int ld, size_t off0, Moments *partials, T *stats,
                           Moments *moments_out, int *ticket, hipStream_t st);   // moments_out: publish moments, not scalars;
                                                                                // ticket: a device word that is zero between launches
template <typename T>
hipError_t sb_launch_sigmoid_apply(const T *ary, T *sm, size_t n, const T *stats, hipStream_t st);
// workgroups of k_scan for nseg 64-cell segments: 16 waves x one trip of 2 segments each, so that a small domain (a band of
// a multi-GPU run) is spread over all CUs and its waves make few dependent trips -- k_scan is latency, not bytes, there;
// at most one 1024-thread workgroup per CU, two trips of loads in flight (two workgroups per CU, 8 waves per SIMD, measured
// slower in round 4: k_scan 25.0 -> 28.7 us at 2560x1920 fp64, 60.1 -> 65.0 at 5120x3840 fp32)
inline int sb_scan_workgroups(unsigned nseg, int ncu) {
    const int nblk = (int)((nseg + 31) / 32);
    return nblk < 1 ? 1 : nblk > ncu ? ncu : nblk;
}
// enqueues the steps of `plan` (sb_diag_plan.hpp), each with the job in the step's mode
template <typename T>
hipError_t sb_launch_diag(const DiagJob<T> &job, const SbDiagPlan &plan, const SbLaunchCtx &lc);
// tile size of the tile contrast kernel (k_thc3) for an LDS halo of H = 24 or 32 cells
void sb_thc_tile_shape(int H, int *tx, int *ty);
// the tile contrast kernel (halos of 24 and 32 cells): reads the list of active tiles and the sigmoid scalars k_prep left
template <typename T>
hipError_t sb_launch_thc(const DiagJob<T> &job, int H, int ncu, hipStream_t st);

// the marching-strip contrast kernel (sb_strip_kernel.hip): LDS halo of 16 cells, ranks k_scan's flags itself
template <typename T>
hipError_t sb_launch_strip(const DiagJob<T> &job, int ncu, hipStream_t st);
// its block grid (strips x 16-row blocks) for nx x rows interior cells; false: the grid is too large for it
bool sb_strip_shape(int nx, int rows, int *ntx, int *nty);
// the marching-strip kernel for search radii up to 31 (sb_strip32_kernel.hip): single precision only (hipErrorInvalidValue
// for double); its flags carry TWO virtual blocks above and below every strip
template <typename T>
hipError_t sb_launch_strip32(const DiagJob<T> &job, int ncu, hipStream_t st);
template <>
hipError_t sb_launch_strip32<float>(const DiagJob<float> &job, int ncu, hipStream_t st);
template <>
hipError_t sb_launch_strip32<double>(const DiagJob<double> &job, int ncu, hipStream_t st);
bool sb_strip32_shape(int nx, int rows, int *ntx, int *nty);
// what the three contrast kernels answer for a domain of nx x rows interior cells: the plan's input
inline SbShapes sb_contrast_shapes(int nx, int rows) {
    SbShapes s;
    s.strip_fits = sb_strip_shape(nx, rows, &s.strip_ntx, &s.strip_nty);
    s.strip32_fits = sb_strip32_shape(nx, rows, &s.strip32_ntx, &s.strip32_nty);
    sb_thc_tile_shape(24, &s.tile_w, &s.tile_rows24);
    sb_thc_tile_shape(32, &s.tile_w, &s.tile_rows32);
    return s;
}

// the device-wide tables (sb_table_kernels.hip): the row pass (t0 -> fixed point -> prefix along longitude, block sums for
// the column pass), the column pass (prefix along latitude, in place), the query (one wave per listed segment -> thc)
template <typename T>
hipError_t sb_launch_table_rows(const DiagJob<T> &job, const SbTables &tb, hipStream_t st);
hipError_t sb_launch_table_cols(const Geo &g, const SbTables &tb, hipStream_t st);
template <typename T>
hipError_t sb_launch_table_query(const DiagJob<T> &job, const SbTables &tb, int ncu, hipStream_t st);

// the guard (sb_guard_kernels.hip): the bad-bit plane and the count, ahead of the call's first kernel; behind the contrast
// kernel the two taint passes and the repair of the tainted band cells in job.thc (three launches).  Where the contrast
// kernel applies the update itself (SbGuardPlan::taint_before, ::update) all but the repair run ahead of it, the latitude
// pass stashes ws / wd, and the repair applies the update again (job.nws / job.nwd: this call's winds)
template <typename T>
hipError_t sb_launch_guard_bits(const DiagJob<T> &job, const SbGuard &gd, int ncu, hipStream_t st);
template <typename T>
hipError_t sb_launch_guard_taint(const DiagJob<T> &job, const SbGuardPlan &gp, const SbGuard &gd, int ncu, hipStream_t st);
template <typename T>
hipError_t sb_launch_guard_repair(const DiagJob<T> &job, const SbGuardPlan &gp, const SbGuard &gd, int ncu, hipStream_t st);

// theta <- theta - (gmma*z)*sigmoid(sigma) over n cells, with the scalars the last diag call left in `stats`
template <typename T>
hipError_t sb_launch_theta_to_t0(T *theta, const T *z, const T *sigma, size_t n, const T *stats, hipStream_t st);

template <typename T>
hipError_t sb_launch_edges(const T *lsm, const T *ci, T *coast, int nx, int ny, int rule, int bnd, hipStream_t st);
// phi: d2r*lat (ny), lamf: folded d2r*lon (nx), both device pointers
template <typename T>
hipError_t sb_launch_dist(const T *coast, const T *mask, const T *phi, const T *lamf,
                          const T *shl, const T *chl,         // sin, cos of half the folded longitudes (k_dist_bits, fp64)
                          T *cdist, int nx, int ny,
                          int k, T maxdist, uint64_t *bits,   // bits: ny*ceil(nx/64) words of workspace
                          int cuts,                           // SB_CUT_* (sb_dist_plan.hpp); the kernel: sb_dist_kernel(nx, k)
                          hipStream_t st);

// A stream whose sea ice moves (sb_diag_stream_ice_*; sb_ice_kernels.hip, sb_ice_plan.hpp): the f2py flavour's coast of
// lsm and ci as bits, compared with and written into the stream's bit plane (ny * ceil(nx/64) words); every (row, tile) a
// changed word can reach gets a 1 in marks (ny * ceil(nx/256) bytes, cleared by the caller); rep[0] += changed words,
// rep[1] += 1 with the first of them unless `first` ...
template <typename T>
hipError_t sb_launch_edge_bits_delta(const T *lsm, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx, int ny,
                                     int k, int first, hipStream_t st);
// ... and sb_launch_dist's kernel over that bit plane, computing the marked tiles of cdist alone
template <typename T>
hipError_t sb_launch_dist_dirty(const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl, T *cdist, int nx, int ny,
                                int k, T maxdist, const uint64_t *bits, int cuts, const unsigned char *marks, hipStream_t st);

// One latitude band in the band step's frame (pitch nx + 2h, interior at (h, h); south / north: the band touches that
// pole).  Edges: lsm, ci, coast are the frames; SB_BND_GLOBAL's rule, raw reads of the first ghost row at a cut side.
template <typename T>
hipError_t sb_launch_edges_band(const T *lsm, const T *ci, T *coast, int nx, int ny, int h, int south, int north, int rule,
                                hipStream_t st);
// Distance: coast, mask, cdist point at (column 0, source row 0) of fields of pitch ld; nys source rows (phi and bits
// have as many), of which r0 .. r1-1 are the targets.
template <typename T>
hipError_t sb_launch_dist_band(const T *coast, const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl, T *cdist,
                               int nx, int nys, int r0, int r1, int ld, int k, T maxdist, uint64_t *bits, int cuts, hipStream_t st);

// A band whose sea ice moves (sb_band_ice_*; sb_ice_kernels.hip, sb_ice_plan.hpp).  lsm, ci: the frames (first cell); br:
// sb_band_rows of the band and k; a cut side needs k + 1 <= h (else hipErrorInvalidValue).  The coast of the band's SOURCE
// rows under SB_BND_GLOBAL's rule as bits, compared with and written into the band's bit plane (br.nys * ceil(nx/64)
// words); every (own row, tile) a changed word can reach gets a 1 in marks (ny * ceil(nx/256) bytes, cleared by the
// caller); rep as sb_launch_edge_bits_delta ...
template <typename T>
hipError_t sb_launch_edge_bits_delta_band(const T *lsm, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx,
                                          int h, SbBandRows br, int south, int north, int rule, int k, int first, hipStream_t st);
// ... or, on the whole path, as a coast plane of pitch nx + 2h that starts at (column 0, source row 0) ...
template <typename T>
hipError_t sb_launch_edges_band_src(const T *lsm, const T *ci, T *coast, int nx, int h, SbBandRows br, int south, int north,
                                    int rule, int k, hipStream_t st);
// ... and sb_launch_dist_band's kernel over that bit plane, computing the marked tiles of the band's own rows alone
template <typename T>
hipError_t sb_launch_dist_band_dirty(const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl, T *cdist, int nx,
                                     int nys, int r0, int r1, int ld, int k, T maxdist, const uint64_t *bits, int cuts,
                                     const unsigned char *marks, hipStream_t st);

// the UM vn10.7 copy's coast setup on the tdims_l layout (sb_um_coast_kernels.hip): lf, ci, coast are
// (nx + 2hi) x (ny + 2hj) with hi, hj >= 1; coast's interior is written, its ghost cells are not
template <typename T>
hipError_t sb_launch_edges_um(const T *lf, const T *ci, T *coast, int nx, int ny, int hi, int hj, hipStream_t st);
// coast, cdist: (nx + 2hi) x (ny + 2hj), hi, hj >= 0, cdist may be coast; landfrac, tlat, tlon: nx x ny (degrees);
// bits: ny * ceil(nx/64) words of workspace.  The window is +-wi x +-wj (0 .. SB_DIST_UM_MAX_WINDOW), stated apart from
// the layout's ghost width: k_dist_um where wi == hi <= 31 and wj == hj <= 31, k_dist_um_wide otherwise
template <typename T>
hipError_t sb_launch_dist_um_win(const T *coast, const T *landfrac, const T *tlat, const T *tlon, T *cdist, int nx, int ny,
                                 int hi, int hj, int wi, int wj, T maxdist, uint64_t *bits, hipStream_t st);

// One tile of a 2-D decomposition (sb_tile_get_edges_um_*, sb_tile_get_dist_um_*; sb_um_coast_kernels.hip).  Every field is
// the tile's (nx + 2hi) x (ny + 2hj) frame (first cell); sides: SB_TILE_* bits, a set bit = that side is the domain's edge.
// Edges: 0/1 into the interior and ei ghost columns / ej ghost rows on every cut side; hipErrorInvalidValue unless the halo
// holds one cell more than is written on every side.  Distance: sources are the coast cells of the interior and of wi ghost
// columns / wj ghost rows on every cut side (hipErrorInvalidValue unless the halo holds them), targets the interior; cdist_l
// may be coast_l; bits: sb_dist_um_tile_bits_bytes of workspace.  k_dist_um_wide's arithmetic whatever the window.
template <typename T>
hipError_t sb_launch_edges_um_tile(const T *lf, const T *ci, T *coast, int nx, int ny, int hi, int hj, int ei, int ej, int sides,
                                   hipStream_t st);
size_t sb_dist_um_tile_bits_bytes(int nx, int ny, int wi, int wj, int sides);
template <typename T>
hipError_t sb_launch_dist_um_tile(const T *coast_l, const T *landfrac_l, const T *tlat_l, const T *tlon_l, T *cdist_l, int nx,
                                  int ny, int hi, int hj, int wi, int wj, int sides, T maxdist, uint64_t *bits, hipStream_t st);

// A UM-layout coast that moves with the sea ice (sb_um_ice_*; sb_ice_kernels.hip, sb_ice_plan.hpp).  lf, ci: the
// (nx + 2hi) x (ny + 2hj) frames (first cell), hi, hj >= 1 (else hipErrorInvalidValue).  The interior's coast under the UM's
// rule as bits, compared with and written into the context's UM bit plane (ny * ceil(nx/64) words); every workgroup of the
// UM distance kernels (4-row group x 64-column tile) a changed word can reach through the +-wi x +-wj window gets a 1 in
// marks (ceil(ny/4) * ceil(nx/64) bytes, cleared by the caller); rep as sb_launch_edge_bits_delta ...
template <typename T>
hipError_t sb_launch_edge_bits_delta_um(const T *lf, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx,
                                        int ny, int hi, int hj, int wi, int wj, int first, hipStream_t st);
// ... and sb_launch_dist_um_win's kernel over that bit plane, computing the marked workgroups of cdist's interior alone;
// landfrac_l is the frame (first cell), read in its interior
template <typename T>
hipError_t sb_launch_dist_um_dirty(const T *landfrac_l, const T *tlat, const T *tlon, T *cdist, int nx, int ny, int hi, int hj,
                                   int wi, int wj, T maxdist, const uint64_t *bits, const unsigned char *marks, hipStream_t st);

// One tile of the UM layout's 2-D decomposition whose coast moves with the sea ice (sb_um_tile_ice_*; sb_ice_kernels.hip,
// sb_um_coast_kernels.hip, sb_ice_plan.hpp).  Every field is the tile's (nx + 2hi) x (ny + 2hj) frame (first cell); r: the
// source rectangle (sb_um_tile_ice_sources: e* = min(window, cells of the domain beyond that side));
// hipErrorInvalidValue unless e* <= the window and the halo holds e* + 1 cells on every side.  bits: (ny+eS+eN) *
// ceil((nx+eW+eE)/64) words, the rectangle's plane; marks, rep: as sb_launch_edge_bits_delta_um, over the interior.
template <typename T>
hipError_t sb_launch_edge_bits_delta_um_tile(const T *lf, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx,
                                             int ny, int hi, int hj, int wi, int wj, SbTileReach r, int first, hipStream_t st);
// ... and k_dist_um_tile over that bit plane, computing the marked workgroups of cdist_l's interior alone
template <typename T>
hipError_t sb_launch_dist_um_tile_dirty(const T *landfrac_l, const T *tlat_l, const T *tlon_l, T *cdist_l, int nx, int ny, int hi,
                                        int hj, int wi, int wj, SbTileReach r, T maxdist, const uint64_t *bits,
                                        const unsigned char *marks, hipStream_t st);
// the whole path: sb_launch_edges_um_tile / sb_launch_dist_um_tile with the reach stated per side instead of by `sides`
template <typename T>
hipError_t sb_launch_edges_um_tile_reach(const T *lf, const T *ci, T *coast, int nx, int ny, int hi, int hj, SbTileReach r,
                                         hipStream_t st);
template <typename T>
hipError_t sb_launch_dist_um_tile_reach(const T *coast_l, const T *landfrac_l, const T *tlat_l, const T *tlon_l, T *cdist_l, int nx,
                                        int ny, int hi, int hj, int wi, int wj, SbTileReach r, T maxdist, uint64_t *bits,
                                        hipStream_t st);

// search_radius (sb_radius_kernels.hip): the radius of every band cell's window from mask alone.  The kernels work in
// WINDOW coordinates: a row as the windows see it has W cells -- the nx cells of the circle (SB_BND_GLOBAL, a band;
// SB_BND_WRAPPER with column nx-1 standing for column 0, the rule's quirk), or the nx + 2h cells of a plain
// SB_BND_HALO frame, which does not wrap.
struct SbRadiusGeo {
    int nx, ny, h, ld;      // interior cells, ghost width, row pitch of mask (nx + 2h)
    int bnd, band, rows;    // BND_*, GEO_BAND_* (0: no band), band rows (ny, or ny - 1 for the wrapper rule)
    int W, nw;              // cells and 64-bit words of a row in window coordinates
    int coff, ioff;         // frame column of window column 0; window column of interior column 0
    int periodic;           // window columns wrap round the row
    int Y0, Y1;             // frame rows a window may read: [Y0, Y1) (not the ghost rows beyond a pole)
};
inline SbRadiusGeo sb_radius_geo(int nx, int ny, int h, int bnd, int band) {
    SbRadiusGeo g;
    g.nx = nx; g.ny = ny; g.h = h; g.ld = nx + 2 * h;
    g.bnd = bnd; g.band = bnd == BND_HALO ? band : 0; g.rows = bnd == BND_WRAPPER ? ny - 1 : ny;
    const bool plain = bnd == BND_HALO && !(g.band & GEO_BAND_EW);
    g.W = plain ? nx + 2 * h : nx; g.nw = (g.W + 63) / 64;
    g.coff = plain ? 0 : h; g.ioff = plain ? h : 0;
    g.periodic = plain ? 0 : 1;
    g.Y0 = (g.band & GEO_BAND_SOUTH) ? h : 0;
    g.Y1 = (g.band & GEO_BAND_NORTH) ? h + ny : ny + 2 * h;
    return g;
}
// the workspace: [64 bytes: "a land-side cell exists", "a sea-side cell exists" | per row, which words of the land-side plane
// hold a land-side cell, which a sea-side cell | land-side plane | band plane | one 16-bit distance per cell], all over the
// ny + 2h frame rows in window coordinates
#define SB_RADIUS_WS_HDR 64
#define SB_RADIUS_MAX_W 65535        // a row distance is kept in 16 bits and 65535 stands for "none": wider rows are refused
#define SB_RADIUS_MAX_SEGS 0x7fffffffLL    // the passes number the frame's segments (rows x words per row) in 32 bits
inline size_t sb_radius_ws_bytes(const SbRadiusGeo &g) {
    const size_t nyh = (size_t)g.ny + 2 * (size_t)g.h, plane = nyh * g.nw * sizeof(uint64_t);
    const size_t sums = nyh * ((g.nw + 63) / 64) * sizeof(uint64_t);
    return SB_RADIUS_WS_HDR + 2 * sums + 2 * plane + ((nyh * g.W * sizeof(uint16_t) + 7) & ~(size_t)7);
}
// zeroes summary / hist (device pointers, any of them and radius may be null) on the stream and enqueues the three passes
template <typename T>
hipError_t sb_launch_search_radius(const T *mask, T maxdist, const SbRadiusGeo &g, void *ws, int *radius, long long *summary,
                                   long long *hist, int nhist, hipStream_t st);

// local part of swap_bounds: E-W periodic ghost columns, pole-side ghost rows replicate the edge row
template <typename T>
hipError_t sb_launch_fill_ghosts(T *field, int nx, int ny, int h, int south, int north, hipStream_t st);
