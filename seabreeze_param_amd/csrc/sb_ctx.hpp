// sb_ctx.hpp -- the context behind the C ABI and what every unit of it shares (host-only, internal):
// sb_capi.hip, sb_capi_diag.hip, sb_capi_stream.hip, sb_capi_coast.hip, sb_capi_band.hip.
#pragma once
#include "../../include/seabreeze_hip.h"
#include "sb_launch.hpp"
#include "sb_ice_plan.hpp"

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

inline thread_local std::string g_err;   // errors raised without a context

// device workspace that grows (ensure) and frees itself with whatever owns it
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// What every coast that moves with the sea ice keeps on the device (a stream's, a band's, the UM layout's, a UM tile's): its own coast
// bit plane (the context's `coastbits` and `umbits` are scratch of other get_dist calls), [marks | rep] and, on the whole
// path, a coast plane.  ice_open .. ice_free below work on it; what is specific to a layout stays with the layout.
struct IceTrack {
    DevBuf bits, marks, coast;
    size_t mark_bytes = 0;              // bytes of the mark plane, rounded up to a word; rep (4 words) follows
    int incremental = 1;
    long long calls = 0;                // ice calls since ice_open; the caller counts a call once it is enqueued
};

class HostPool;                     // sb_capi_stream.hip

// words of sb_ctx::ticket: [0] k_scan's spare word, [1] k_stats' / a band step's ticket
enum { SB_TICKET_WORDS = 2 };

// Streaming form of the f2py-flavour diag (sb_diag_stream_*): what stays on the device between steps, and the
// pinned staging buffers of the per-step transfers.
struct DiagStream {
    bool active = false;
    HostPool *pool = nullptr;                  // created by the first sb_diag_stream_begin, joined by sb_destroy
    int nlons = 0, nlats = 0, esz = 0;
    DevBuf z, sd, cdist, ws, wd, thc, p1, theta, v, u, out;
    void *pin_in[2] = {nullptr, nullptr};      // theta | v plane | u plane | p level, two slots
    void *pin_out[2] = {nullptr, nullptr};     // sb_con plane of a step, two slots
    size_t pin_in_cap = 0, pin_out_cap = 0;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    long steps = 0;
    double host_copy_s = 0.0, enqueue_s = 0.0, wait_s = 0.0;   // where the host spent its time (sb_diag_stream_stats)
    // a coast that moves with the sea ice (sb_diag_stream_coast / _ice): the land mask and the step's ice plane, the
    // stream's planes of it (it); the pinned staging of the ice plane; what sb_diag_stream_coast derived
    bool ice_ready = false;                    // sb_diag_stream_coast since the last sb_diag_stream_begin
    DevBuf lsm, ice;
    IceTrack it;
    void *pin_ice[2] = {nullptr, nullptr};
    size_t pin_ice_cap = 0;
    hipEvent_t ev_ice[2] = {nullptr, nullptr};
    hipEvent_t ev_ice_t[2] = {nullptr, nullptr};   // round the device work of the last ice call (sb_diag_stream_ice_time)
    std::vector<unsigned char> ice_lonlat;     // lon(nlons) | lat(nlats): every ice call keys the coordinate tables with them
    int ice_k = 0;
    double ice_maxdist = 0.0;
};

// A band whose coast moves with the sea ice (sb_band_coast_open / sb_band_ice_*_dev): the geometry it was opened for, its
// planes (it: the bit plane and, on the whole path, the coast plane cover the band's source rows; one mark byte per (own
// row, tile)); lon and the source rows' latitudes, with which every ice call keys the coordinate tables.
struct BandCoast {
    bool open = false;
    int esz = 0, nx = 0, ny = 0, halo = 0, south = 0, north = 0, k = 0, rule = 0;
    double maxdist = 0.0;
    IceTrack it;
    std::vector<unsigned char> lonlat;         // lon(nx) | lat(nys)
};

// A UM-layout coast that moves with the sea ice (sb_um_coast_open / sb_um_ice_*): the geometry it was opened for, the
// coordinates on the device (tlat | tlon, interior fields), its planes (it: the bit plane covers the interior, one mark
// byte per workgroup of the UM distance kernels, the whole path's coast is a frame) and, on the whole path, an interior
// copy of landfrac.  Independent of the stream's and the band's moving coasts.
struct UmCoast {
    bool open = false;
    int esz = 0, nx = 0, ny = 0, hi = 0, hj = 0, wi = 0, wj = 0;
    double maxdist = 0.0;
    DevBuf coords, lf;
    IceTrack it;
};

// One tile of the UM layout's 2-D decomposition whose coast moves with the sea ice (sb_um_tile_coast_open /
// sb_um_tile_ice_*): the geometry it was opened for (beyond: the domain cells beyond the west, east, south and north
// side), the coordinate FRAMES on the device (tlat | tlon), its planes (it: the bit plane covers the source rectangle of
// sb_um_tile_ice_plan, one mark byte per workgroup of k_dist_um_tile over the interior, the whole path's coast is a
// frame).  Independent of the other three moving coasts.
struct UmTileCoast {
    bool open = false;
    int esz = 0, nx = 0, ny = 0, hi = 0, hj = 0, wi = 0, wj = 0, beyond[4] = {0, 0, 0, 0};
    double maxdist = 0.0;
    DevBuf coords;
    IceTrack it;
};

struct sb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int radius_hint = 16;
    int ncu = 256;              // persistent workgroups of the one-per-CU kernels: the device's compute units (sb_set_workgroups)
    int ncu_dev = 256;          // compute units of the device
    // opt-in: sigma does not change between calls (sb_set_static_sigma): its statistics are kept from the first
    // complete call on the same array and k_scan stops reading it
    int static_sigma = 0;
    bool stats_valid = false;
    int host_depth = 0;                 // > 0 inside a host-pointer entry point: staged copies have no identity
    int no_fold = 0;                    // sb_set_fold(ctx, 0): k_prep stays a kernel of its own
    int no_plan_cache = 0;              // sb_set_plan_cache(ctx, 0): the strip kernel plans its march afresh every call
    int no_wide_strip = 0;              // sb_set_wide_strip(ctx, 0): radii beyond 16 take the tile kernel in single precision too
    int band_late_wind = 0;             // sb_set_band_order(ctx, 1): a band step runs the contrast before k_wind (measurement)
    int no_wind_pairs = 0;              // sb_set_wind_pairs(ctx, 0): k_wind walks one cell per lane everywhere
    int last_wind_pairs = 0;            // the last call's k_wind was the paired instance (sb_last_wind_pairs)
    // the opt-in switches of the table contrast, its window cache and the guard (the six setters at the end of sb_capi.hip): which
    // calls each of them serves is sb_apply_switches' to say (sb_diag_plan.hpp)
    SbSwitches sw{};
    // the window cache: what the host knows about whose planes W belongs to (sb_table_cache.hpp); the report's host half
    // (sb_table_cache_report)
    SbTabCache tabc;
    bool tab_rep_reset = true;          // no call has run with the cache in effect since the switch was turned on
    bool tab_last = false;              // the last diag call ran with the cache in effect
    long long tab_calls = 0;            // such calls since the switch was turned on
    int tab_waves = 0;                  // waves of the last such call's query: the slots of the report it wrote
    // the guard for missing / non-finite temperatures (sb_guard_kernels.hip): the report's host half (sb_guard_report)
    bool guard_rep_reset = true;        // no call has run with the guard in effect since the switch was set
    bool guard_last = false;            // the last diag call ran with the guard in effect
    long long guard_calls = 0;          // such calls since the switch was set
    const void *stats_sigma = nullptr;
    int stats_dims[4] = {0, 0, 0, 0};   // nx, ny, halo, sizeof(T)
    int stats_ngathered = 0;            // bands whose moments the kept scalars were merged from (0: this domain's own)
    // what the last diag / band step enqueued (sb_last_step_report)
    int rep_launches = 0, rep_rccl = 0, rep_groups = 0, rep_copies = 0;
    // workspace (grow-only)
    DevBuf t0, bandbits, clsbits, tiles, vecs, nws, nwd, coastbits, tile_list, seg_list, stamps, jobcopy, plan;
    DevBuf umbits;                      // the coast bit plane of sb_get_dist_um_*
    DevBuf tabA, tabL, tabC, tabS;      // the device-wide summed-area tables (SbTables), allocated by the first call that builds them
    DevBuf tabW, tabRep;                // the stored windows and the report's device words, allocated with them while the cache is on
    DevBuf guardA, guardB, guardRep;    // the guard's two bit planes and its device words (SbGuard), allocated while the switch is on
    DevBuf guardWs, guardWd;            // sb_set_nonfinite_guard_bands: ws / wd of the tainted band cells ahead of the contrast kernel's update
    // search_radius: its planes, flags and row distances; the host forms' copies of mask and of the results.  No diag call
    // reads or writes them, and search_radius touches nothing else of the context.
    DevBuf rad_ws, rad_mask, rad_out;
    // the strip kernel's plan (sb_strip_kernel.hip): [64 bytes: number of the last call whose band plane changed |
    // ncu x SB_PLAN_STRIDE]; plan_key: the geometry it was made for; call_seq numbers the diag calls
    int plan_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const void *plan_bits = nullptr;
    int call_seq = 0, plan_use = 0;
    bool segs_built = false;            // the last complete call's strip kernel compacted k_wind's segment lists
    int tiles_n = 0, tiles_strip = -1, flag_parity = 0;   // two alternating [tile flags | counters] buffers in `tiles`
    int *last_flags = nullptr;          // the buffer the last diag call used
    Moments *partials = nullptr;
    unsigned int *ticket = nullptr;
    void *stats = nullptr;      // 4 x double
    int *counters = nullptr;    // 2 ints
    int *seg_count = nullptr;   // SB_SEG_PARTS ints: entries in each sub-list of segments (k_prep -> k_wind)
    // get_dist's coordinate tables (device: `vecs`): the coordinates they were made from, the host copy the upload reads,
    // and what the host found out about the coordinates' order
    std::vector<unsigned char> dist_key, dist_hv;
    SbDistTraits dist_traits;           // what the host found out about the coordinates' order (sb_dist_plan.hpp)
    hipStream_t dist_upload_stream = nullptr;   // the stream the tables were uploaded on, until another stream has waited for it
    // staging buffers for the host-pointer entry points
    std::vector<DevBuf> stage;
    // geometry of the last diag call (for sb_last_counters)
    Geo last_g{};
    int last_tiles = 0;
    bool have_last = false;
    // optional per-kernel HIP-event timing (sb_profile_begin / sb_profile_end)
    const Moments *gathered = nullptr;   // device array of per-band sigma moments (multi-GPU), or null: sb_use_gathered_moments
    int ngathered = 0;                   // alone writes the pair, plain_call reads it
    std::vector<hipEvent_t> prof_ev;
    std::vector<unsigned> prof_mask;    // per profiled call: which kernels were launched
    int prof_calls = 0, prof_max = 0;
    // latitude-band communicator (RCCL, loaded on demand by sb_comm_init)
    hipStream_t aux_stream = nullptr;   // communication of a band step runs here
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_mom = nullptr;
    DevBuf band_mom;                    // [5 own moments | 5 x nranks gathered]
    void *rccl_lib = nullptr;
    void *comm = nullptr;
    int rank = 0, nranks = 1;
    DiagStream ds;
    BandCoast bc;
    UmCoast um;
    UmTileCoast umt;
};

// What a band step means to the diag code underneath travels as an argument: band_diag_dev builds one value per phase,
// every other call takes plain_call's.
struct SbBandCall {
    int phases = 3;                     // 1: k_scan .. k_wind, 2: the contrast kernel and what follows it, 3: a whole call
    int geo = 0;                        // GEO_BAND_*: which ghost cells of theta follow from its interior and are not read (strip kernels)
    Moments *moments_out = nullptr;     // phase 1: where k_scan leaves this band's sigma moments
    const Moments *gathered = nullptr;  // the per-band sigma moments to merge instead of scanning sigma, or null
    int ngathered = 0;
};
inline SbBandCall plain_call(const sb_ctx *c) {
    SbBandCall b;
    if (c) { b.gathered = c->gathered; b.ngathered = c->ngathered; }    // as sb_use_gathered_moments left them
    return b;
}

inline int fail(sb_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_err = msg;
    return code;
}

inline int hipfail(sb_ctx *c, hipError_t e, const char *what) {
    return fail(c, SB_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(c, call)                                         \
    do {                                                        \
        hipError_t e__ = (call);                                \
        if (e__ != hipSuccess) return hipfail((c), e__, #call); \
    } while (0)

// the stream of a `_dev` call: the caller's, or the context's own
inline hipStream_t stream_of(const sb_ctx *c, void *stream) { return stream ? (hipStream_t)stream : c->stream; }

inline int ensure(sb_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return SB_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(c, SB_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    b.cap = bytes;
    return SB_OK;
}

// ---- the planes of a coast that moves with the sea ice (IceTrack) ----
// sizes in; the empty coast in the bit plane -- the first ice call differs from it -- and a cleared rep, enqueued on st
inline int ice_open(sb_ctx *c, IceTrack &t, size_t bitbytes, SbIceMarks m, size_t coastbytes, int incremental, hipStream_t st) {
    const size_t markbytes = ((size_t)m.rows * m.tiles + 3) & ~(size_t)3;
    int rc;
    if ((rc = ensure(c, t.bits, bitbytes)) || (rc = ensure(c, t.marks, markbytes + 4 * sizeof(unsigned)))) return rc;
    if (coastbytes && (rc = ensure(c, t.coast, coastbytes))) return rc;
    HIPCHK(c, hipMemsetAsync(t.bits.p, 0, bitbytes, st));
    HIPCHK(c, hipMemsetAsync((char *)t.marks.p + markbytes, 0, 4 * sizeof(unsigned), st));
    t.mark_bytes = markbytes;
    t.incremental = incremental ? 1 : 0;
    t.calls = 0;
    return SB_OK;
}

// what a call on the delta path hands its kernels
struct IceCall {
    unsigned char *marks;
    unsigned *rep;
    int first;
};

// the first call computes everything: every byte marked by the host; rep[0] cleared either way
inline int ice_begin(sb_ctx *c, const IceTrack &t, hipStream_t st, IceCall &call) {
    call.marks = (unsigned char *)t.marks.p;
    call.rep = (unsigned *)(call.marks + t.mark_bytes);
    call.first = t.calls == 0 ? 1 : 0;
    if (call.first) {
        HIPCHK(c, hipMemsetAsync(call.marks, 1, t.mark_bytes, st));
        HIPCHK(c, hipMemsetAsync(call.rep, 0, sizeof(unsigned), st));
    } else
        HIPCHK(c, hipMemsetAsync(call.marks, 0, t.mark_bytes + sizeof(unsigned), st));
    return SB_OK;
}

// rep[4] of sb_*_ice_report: calls, calls whose coast differed (-1 on the whole path), bytes marked by the last call, bytes
// of the plane.  device_wide: the ice calls ran on whichever stream the caller named; else on the context's own.
inline int ice_report(sb_ctx *c, const IceTrack &t, SbIceMarks m, bool whole, bool device_wide, long long rep[4]) {
    const long long tiles = (long long)m.rows * m.tiles;
    rep[0] = t.calls; rep[1] = 0; rep[2] = 0; rep[3] = tiles;
    HIPCHK(c, device_wide ? hipDeviceSynchronize() : hipStreamSynchronize(c->stream));
    if (whole) {
        // every call computes every tile and compares nothing
        rep[1] = -1;
        rep[2] = t.calls ? tiles : 0;
        return SB_OK;
    }
    if (t.calls == 0) return SB_OK;
    std::vector<unsigned char> host(t.mark_bytes + 2 * sizeof(unsigned));
    HIPCHK(c, hipMemcpy(host.data(), t.marks.p, host.size(), hipMemcpyDeviceToHost));
    for (long long i = 0; i < tiles; ++i) rep[2] += host[(size_t)i] ? 1 : 0;
    unsigned words[2];
    std::memcpy(words, host.data() + t.mark_bytes, sizeof(words));
    rep[1] = words[1];
    return SB_OK;
}

inline void ice_free(IceTrack &t) {
    for (DevBuf *d : {&t.bits, &t.marks, &t.coast})
        if (d->p) { (void)hipFree(d->p); d->p = nullptr; d->cap = 0; }
    t.calls = 0;
}

template <typename T>
Geo make_geo(int nx, int ny, int h, int bnd, int rows) {
    Geo g;
    g.nx = nx; g.ny = ny; g.h = h;
    g.nxh = nx + 2 * h; g.nyh = ny + 2 * h;
    g.nw = (g.nxh + 63) / 64;
    g.bnd = bnd; g.rows = rows;
    g.band = 0;
    return g;
}

inline int check_dims(sb_ctx *c, int nx, int ny, int nz, int halo, int bnd) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || nz < 1) return fail(c, SB_ERR_ARG, "nx, ny, nz must be >= 1");
    if (bnd < 0 || bnd > 2) return fail(c, SB_ERR_ARG, "unknown boundary rule");
    if (halo < 0 || (halo > 0 && bnd != SB_BND_HALO)) return fail(c, SB_ERR_ARG, "halo > 0 needs SB_BND_HALO");
    if ((double)(nx + 2 * halo) * (double)(ny + 2 * halo) > 2.0e9) return fail(c, SB_ERR_ARG, "grid too large");
    return SB_OK;
}

inline int check_arrays(sb_ctx *c, std::initializer_list<const void *> arrays) {
    for (const void *a : arrays)
        if (!a) return fail(c, SB_ERR_ARG, "null array pointer");
    return SB_OK;
}

// the one argument check of a diag call's `_dev` and host-pointer forms
inline int check_diag(sb_ctx *c, int nx, int ny, int nz, int halo, int bnd, std::initializer_list<const void *> arrays) {
    const int rc = check_dims(c, nx, ny, nz, halo, bnd);
    return rc ? rc : check_arrays(c, arrays);
}

// the level of a 1-D pressure column nearest the target (hPa), exactly as the kernel picks it: the first minimum of
// |p - target| in the working precision, the target converted like ref: seabreeze_diag_python.f90:148
template <typename T>
int pick_level(const T *p, int nps, T target_plev) {
    const T tp = target_plev * T(100.);
    int lev = 0;
    T best = std::fabs(p[0] - tp);
    for (int k = 1; k < nps; ++k) {
        const T a = std::fabs(p[k] - tp);
        if (a < best) { best = a; lev = k; }
    }
    return lev;
}

// ---- host staging helpers ----------------------------------------------------------
struct Stager {
    sb_ctx *c;
    size_t next = 0;
    int rc = SB_OK;
    // the staged copy of sigma sits at the same device address whatever the caller passed: the static-sigma
    // option is honoured by the device-pointer entry points only
    explicit Stager(sb_ctx *ctx) : c(ctx) { if (c) { ++c->host_depth; c->stats_valid = false; } }
    ~Stager() { if (c) --c->host_depth; }
    Stager(const Stager &) = delete;
    Stager &operator=(const Stager &) = delete;
    template <typename T>
    T *in(const T *host, size_t n) {       // upload
        T *d = out<T>(n);
        if (rc || !d) return nullptr;
        hipError_t e = hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) rc = hipfail(c, e, "hipMemcpyAsync H2D");
        return d;
    }
    template <typename T>
    T *out(size_t n) {                     // device scratch only
        if (rc) return nullptr;
        if (next >= c->stage.size()) c->stage.resize(next + 1);
        DevBuf &b = c->stage[next++];
        rc = ensure(c, b, n * sizeof(T) > 0 ? n * sizeof(T) : 8);
        return rc ? nullptr : (T *)b.p;
    }
    template <typename T>
    void back(T *host, const T *dev, size_t n) {
        if (rc) return;
        hipError_t e = hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = hipfail(c, e, "hipMemcpyAsync D2H");
    }
    int finish() {
        if (rc) return rc;
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hipfail(c, e, "hipStreamSynchronize");
        return SB_OK;
    }
};

// ---- what one unit calls in another: defined once, emitted for float and double by the owning unit ----
// sb_capi_diag.hip (the band step and the stream call them)
template <typename T>
int seabreeze_diag_dev(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, int bnd, const T *p,
                       const T *u, const T *v, const T *theta, const T *mask, const T *z, const T *sigma, T *ws,
                       T *wd, T *thc, T *sb_con, const sb_tunables *tun, void *stream, const SbBandCall &call,
                       int mask_halo = -1, int level_rule = 0);
template <typename T>
int diag_dev(sb_ctx *c, int tn, const T *p, const T *z, const T *std_, const T *theta, const T *v, const T *u,
             const T *cdist, T *ws, T *wd, T *thc, T target_plev, T thresh_wind, T thresh_winddir, T thresh_windch,
             T thresh_thc, T target_time, T maxdist, T timestep, int nps, int nlons, int nlats, T *output,
             void *stream);
template <typename T>
SbPlanIn plan_input(const sb_ctx *c, const SbBandCall &call, int nx, int rows);
template <typename T>
bool reuse_stats(const sb_ctx *c, const SbBandCall &call, const T *sigma, int nx, int ny, int halo);
// sb_capi_coast.hip (the stream's moving coast calls them)
template <typename T>
int dist_window(int nx, int ny, const T *lon, const T *lat, T maxdist, int *k);
template <typename T>
int dist_tables(sb_ctx *c, int nx, int ny, const T *lon, const T *lat, hipStream_t st);
// sb_capi_stream.hip (sb_destroy calls it)
void stream_release(sb_ctx *c);
