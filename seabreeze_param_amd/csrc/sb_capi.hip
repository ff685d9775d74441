// sb_capi.hip -- the C ABI of libseabreeze_hip.so (see include/seabreeze_hip.h).
//
// Host-pointer entry points stage through device buffers owned by the context and
// synchronise before returning; `_dev` entry points only enqueue.  There is no CPU
// fallback anywhere in this file: no device => SB_ERR_NO_DEVICE.
#include "../../include/seabreeze_hip.h"
#include "sb_launch.hpp"
#include "sb_ice_plan.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;   // errors raised without a context

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

}  // namespace

// Streaming form of the f2py-flavour diag (sb_diag_stream_*): what stays on the device between steps, and the
// pinned staging buffers of the per-step transfers.
// A handful of host threads that live as long as the context streams timesteps: the per-step copies between the
// caller's pageable arrays and the pinned staging buffers (three planes in, one plane out with a conversion to double)
// are cut into ranges and run side by side.  (Round 2 started two threads per step with std::async and converted the
// output on the calling thread: 0.68 ms of host copies per 1024 x 768 step, the longest item of a streamed step.)
class HostPool {
  public:
    explicit HostPool(int n) {
        for (int i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); });
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> g(m_); quit_ = true; }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    // run fn(0) .. fn(n-1), the caller's thread included; returns when all are done
    void run(int n, const std::function<void(int)> &fn) {
        if (n <= 0) return;
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn; next_ = 0; total_ = n; done_ = 0;
            ++epoch_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(m_);
        done_cv_.wait(lk, [this] { return done_ == total_; });
        fn_ = nullptr;
    }
    int threads() const { return (int)workers_.size() + 1; }

  private:
    void work() {
        for (;;) {
            int i;
            const std::function<void(int)> *f;
            {
                std::lock_guard<std::mutex> g(m_);
                if (!fn_ || next_ >= total_) return;
                i = next_++;
                f = fn_;
            }
            (*f)(i);
            {
                std::lock_guard<std::mutex> g(m_);
                if (++done_ == total_) done_cv_.notify_all();
            }
        }
    }
    void loop() {
        unsigned long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return quit_ || epoch_ != seen; });
                if (quit_) return;
                seen = epoch_;
            }
            work();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(int)> *fn_ = nullptr;
    int next_ = 0, total_ = 0, done_ = 0;
    unsigned long epoch_ = 0;
    bool quit_ = false;
};

// words of sb_ctx::ticket: [0] k_scan's spare word, [1] k_stats' / a band step's ticket
enum { SB_TICKET_WORDS = 2 };

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
    // stream's own coast bit plane (the context's `coastbits` is scratch of other get_dist calls), [marks | rep] and, on
    // the whole-grid path, a coast plane; the pinned staging of the ice plane; what sb_diag_stream_coast derived
    bool ice_ready = false;                    // sb_diag_stream_coast since the last sb_diag_stream_begin
    DevBuf lsm, ice, icebits, icemarks, icecoast;
    void *pin_ice[2] = {nullptr, nullptr};
    size_t pin_ice_cap = 0;
    hipEvent_t ev_ice[2] = {nullptr, nullptr};
    hipEvent_t ev_ice_t[2] = {nullptr, nullptr};   // round the device work of the last ice call (sb_diag_stream_ice_time)
    std::vector<unsigned char> ice_lonlat;     // lon(nlons) | lat(nlats): every ice call keys the coordinate tables with them
    int ice_k = 0, ice_incremental = 1;
    double ice_maxdist = 0.0;
    size_t ice_mark_bytes = 0;                 // bytes of the mark plane, rounded up to a word; rep follows
    long long ice_calls = 0;
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
    // the opt-in switches of the table contrast, its window cache and the guard (the six setters at the end of this file): which
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
    const Moments *gathered = nullptr;   // device array of per-band sigma moments (multi-GPU), or null
    int ngathered = 0;
    std::vector<hipEvent_t> prof_ev;
    std::vector<unsigned> prof_mask;    // per profiled call: which kernels were launched
    int prof_calls = 0, prof_max = 0;
    // latitude-band communicator (RCCL, loaded on demand by sb_comm_init)
    hipStream_t aux_stream = nullptr;   // communication of a band step runs here
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_mom = nullptr;
    Moments *band_moments_out = nullptr;   // set around phase 1 of a band step: where k_scan leaves this band's moments
    int band_geo = 0;                   // set around a band step on a strip kernel: GEO_BAND_* (which ghost cells of theta follow from
                                        // its interior and are not read)
    DevBuf band_mom;                    // [5 own moments | 5 x nranks gathered]
    void *rccl_lib = nullptr;
    void *comm = nullptr;
    int rank = 0, nranks = 1;
    DiagStream ds;
};

namespace {

int fail(sb_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_err = msg;
    return code;
}

int hipfail(sb_ctx *c, hipError_t e, const char *what) {
    return fail(c, SB_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(c, call)                                         \
    do {                                                        \
        hipError_t e__ = (call);                                \
        if (e__ != hipSuccess) return hipfail((c), e__, #call); \
    } while (0)

int ensure(sb_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return SB_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(c, SB_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    b.cap = bytes;
    return SB_OK;
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

// the launch plan's input (sb_diag_plan.hpp) as far as the context and the domain give it: all the contrast kernel's choice needs
template <typename T>
static SbPlanIn plan_input(const sb_ctx *c, int nx, int rows) {
    SbPlanIn in{};
    in.esize = (int)sizeof(T); in.nx = nx; in.rows = rows; in.halo = sb_pick_halo(c->radius_hint);
    in.no_wide_strip = c->no_wide_strip != 0; in.no_fold = c->no_fold != 0; in.no_plan_cache = c->no_plan_cache != 0;
    in.band_late_wind = c->band_late_wind != 0; in.gathered = c->gathered != nullptr;
    in.shapes = sb_contrast_shapes(nx, rows);
    return in;
}

// sigma's statistics of an earlier complete call still stand (opt-in, same array, same shape)
template <typename T>
static bool reuse_stats(const sb_ctx *c, const T *sigma, int nx, int ny, int halo) {
    return c->static_sigma && c->host_depth == 0 && c->stats_valid && c->stats_sigma == (const void *)sigma && c->stats_dims[0] == nx &&
           c->stats_dims[1] == ny && c->stats_dims[2] == halo && c->stats_dims[3] == (int)sizeof(T) &&
           c->stats_ngathered == (c->gathered ? c->ngathered : 0);   // single-domain scalars are not a band run's
}

// Prepare workspace + job; enqueue the kernels of one diag call.
template <typename T>
int run_diag(sb_ctx *c, DiagJob<T> &job, hipStream_t st, int phases = 3) {
    const Geo &g = job.g;
    const size_t ncell = (size_t)g.nxh * g.nyh;
    const size_t nbits = (size_t)g.nyh * g.nw * sizeof(uint64_t);
    int rc;
    c->tab_last = false;                // (sb_table_cache_report: until this call has been enqueued with the cache in effect)
    c->guard_last = false;              // (sb_guard_report likewise)
    if ((rc = ensure(c, c->bandbits, nbits))) return rc;
    if ((rc = ensure(c, c->clsbits, nbits))) return rc;
    SbPlanIn in = plan_input<T>(c, g.nx, g.rows);
    const SbContrast k = sb_plan_contrast(in);
    const bool strip = k.strip != 0;
    const int tx = k.tx, ty = k.ty, vb = k.vb, ntile = k.ntile, nflag = k.nflag;
    // Two buffers of [per-tile flags | 2 slow-path counters], used by alternate calls: k_scan
    // raises flags in this call's buffer, k_wind clears the other one for the next call, so no
    // memset sits on the critical path and the last call's values stay readable.
    if (c->tiles.cap < (size_t)2 * nflag * sizeof(int) || c->tiles_n != nflag || c->tiles_strip != vb) {
        if ((rc = ensure(c, c->tiles, (size_t)2 * nflag * sizeof(int)))) return rc;
        // (in stream order, on the call's own stream: a plain hipMemset runs on the null stream, which the non-blocking
        // streams kernels are enqueued on do not wait for -- a late memset could wipe flags k_scan had already raised.  No
        // device-wide synchronisation: what ran before on this stream is ordered before the memset, and a reallocation
        // above has synchronised already)
        HIPCHK(c, hipMemsetAsync(c->tiles.p, 0, (size_t)2 * nflag * sizeof(int), st));
        c->tiles_n = nflag;
        c->tiles_strip = vb;
        c->flag_parity = 0;
    }
    int *flags_now = (int *)c->tiles.p + (size_t)c->flag_parity * nflag;
    int *flags_next = (int *)c->tiles.p + (size_t)(1 - c->flag_parity) * nflag;
    job.thc_ty = k.tyrows; job.thc_ntx = tx; job.thc_nty = ty; job.thc_txs = k.txw == 32 ? 5 : 6;
    job.strip = k.strip;
    if (strip) { job.tile_sx = ty + 2 * vb; job.tile_sy = 1; job.tile_off = vb; }
    else { job.tile_sx = 1; job.tile_sy = tx; job.tile_off = 0; }
    job.bandbits = (uint64_t *)c->bandbits.p;
    job.clsbits = (uint64_t *)c->clsbits.p;
    job.stats = (const T *)c->stats;
    job.tile_nnmax = flags_now;
    job.counters = flags_now + (size_t)ntile;
    job.ticket = (int *)c->ticket;
    job.next_flags = flags_next;
    job.next_flags_n = nflag;
    // the lists k_prep compacts: active tiles (k_thc3) and segments that hold band cells (k_wind)
    // (padded: a k_thc3 workgroup loads its first two candidate entries before it knows how many there are)
    if ((rc = ensure(c, c->tile_list, ((size_t)ntile + (size_t)2 * c->ncu + 2) * sizeof(int)))) return rc;
    job.tile_pad = 2 * c->ncu;
    const size_t nseg = (size_t)g.nyh * g.nw;
    const size_t seg_cap = (nseg + SB_SEG_PARTS - 1) / SB_SEG_PARTS;
    if ((rc = ensure(c, c->seg_list, seg_cap * SB_SEG_PARTS * sizeof(SbSegEntry)))) return rc;
    job.tile_list = (int *)c->tile_list.p;
    job.seg_list = (SbSegEntry *)c->seg_list.p;
    job.seg_count = c->seg_count;
    job.seg_cap = (int)seg_cap;
    // the host-model flavour derives t0 inside k_thc3; the f2py flavour returns the t0 plane
    job.t0_fly = (job.flavour == SB_FLAVOUR_GENERIC) ? 1 : 0;
    // the t0 plane with its ghost cells: f2py flavour only (k_t0 -> k_thc3)
    if (!job.t0_fly) {
        if ((rc = ensure(c, c->t0, ncell * sizeof(T)))) return rc;
        job.t0 = (T *)c->t0.p;
    }
    if ((rc = ensure(c, c->jobcopy, sizeof(DiagJob<double>)))) return rc;
    job.self = (DiagJob<T> *)c->jobcopy.p;
    // which of the context's switches serve this call, and whether it is a table call that keeps its windows (its k_scan
    // watches the planes whatever the contrast kernel: without a strip kernel the header of the plan alone is allocated)
    static_assert((int)SB_CALL_BND_WRAPPER == (int)BND_WRAPPER && (int)SB_CALL_BND_GLOBAL == (int)BND_GLOBAL &&
                  (int)SB_CALL_BND_HALO == (int)BND_HALO, "SbCallBnd names sb_device.hpp's boundary rules");
    in.phases = phases;
    const bool cache = sb_apply_switches(c->sw, SbCall{job.flavour == SB_FLAVOUR_GENERIC, g.bnd, g.h != 0, g.band != 0}, in);
    if (strip || cache) {
        const size_t need = 64 + (strip ? (size_t)c->ncu * SB_PLAN_STRIDE : (size_t)0);
        if (c->plan.cap < need) {
            if ((rc = ensure(c, c->plan, need))) return rc;
            HIPCHK(c, hipMemsetAsync(c->plan.p, 0, need, st));   // no plan stored, no change seen (stream-ordered)
            c->plan_bits = nullptr;
        }
        if (phases & 1) {
            // a new call: its number, and whether the stored plan was made for this geometry, by this many workgroups,
            // from planes that live where this call's do
            if (c->call_seq == 0x7fffffff) {                 // (the numbers start over: nothing stored counts)
                HIPCHK(c, hipMemsetAsync(c->plan.p, 0, need, st));
                c->call_seq = 0;
                c->plan_bits = nullptr;
            }
            ++c->call_seq;
            if (strip) {
                const int key[8] = {g.nx, g.ny, g.h, g.bnd, g.rows, c->ncu, tx, ty | (vb << 24)};     // (the two strip kernels' plans differ)
                c->plan_use = c->plan_bits == c->bandbits.p && std::memcmp(key, c->plan_key, sizeof(key)) == 0 ? 1 : 0;
                std::memcpy(c->plan_key, key, sizeof(key));
                c->plan_bits = c->bandbits.p;
            } else c->plan_bits = nullptr;                   // (as below: no strip kernel's plan follows from this call's planes)
        }
        job.plan = (char *)c->plan.p + 64;
        job.plan_gen = (int *)c->plan.p;
        job.call_id = c->call_seq;
        job.plan_use = strip && !c->no_plan_cache ? c->plan_use : 0;
    } else if (phases & 1) c->plan_bits = nullptr;           // (the tile kernel rewrites nothing of the plan, but k_scan does not watch the plane for it)
#ifdef SB_STAMPS
    if ((rc = ensure(c, c->stamps, (size_t)4096 * SB_NSTAMP * sizeof(long long)))) return rc;
    job.stamps = (long long *)c->stamps.p;
#endif
    SbLaunchCtx lc{};
    if (phases == 3 && c->prof_calls < c->prof_max) {
        lc.prof_mask = &c->prof_mask[(size_t)c->prof_calls];
        lc.prof = &c->prof_ev[(size_t)SB_PROF_EVENTS * c->prof_calls++];
    }
    lc.stream = st; lc.partials = c->partials; lc.stats = c->stats;
    lc.gathered = c->gathered; lc.ngathered = c->ngathered; lc.ncu = c->ncu;
    lc.wind_pairs = c->no_wind_pairs ? 0 : 1; lc.wind_pairs_ran = &c->last_wind_pairs;
    lc.moments_out = (phases == 1) ? c->band_moments_out : nullptr;   // (a band step: k_scan publishes this band's moments)
    lc.moments_event = (phases == 1 && c->nranks > 1) ? c->ev_mom : nullptr;   // (one rank: nobody waits for them)
    lc.stats_ticket = (int *)c->ticket + 1;
    // every decision about the kernels of this call: the plan's (the job's mode fields are the executor's to set)
    in.t0_fly = job.t0_fly != 0; in.moments_out = lc.moments_out != nullptr;
    in.reuse_stats = reuse_stats<T>(c, job.sigma, g.nx, g.ny, g.h);
    in.plan_use = c->plan_use != 0; in.segs_built = c->segs_built;
    in.scan_wgs = sb_scan_workgroups((unsigned)g.nyh * (unsigned)g.nw, c->ncu);
    const SbDiagPlan plan = sb_plan_diag(in);
    // the guard for missing and non-finite temperatures: a plan of its own beside that one, which it leaves as it is
    lc.guard = sb_plan_guard(in, plan);
    if (lc.guard.on) {
        if ((rc = ensure(c, c->guardA, nbits))) return rc;
        if ((rc = ensure(c, c->guardB, nbits))) return rc;
        if (!c->guardRep.p) {
            if ((rc = ensure(c, c->guardRep, SB_GUARD_REP_WORDS * sizeof(unsigned)))) return rc;
            HIPCHK(c, hipMemsetAsync(c->guardRep.p, 0, SB_GUARD_REP_WORDS * sizeof(unsigned), st));   // (the ticket: zero between launches)
        }
        lc.guard_ws.bad = (uint64_t *)c->guardA.p; lc.guard_ws.taint = (uint64_t *)c->guardB.p; lc.guard_ws.rep = (unsigned *)c->guardRep.p;
        lc.guard_ws.rep_reset = c->guard_rep_reset ? 1 : 0;
        if (lc.guard.taint_before >= 0) {                // the contrast kernel applies the update: ws / wd of the tainted cells are put aside
            if ((rc = ensure(c, c->guardWs, (size_t)g.nx * g.ny * sizeof(T)))) return rc;
            if ((rc = ensure(c, c->guardWd, (size_t)g.nx * g.ny * sizeof(T)))) return rc;
            lc.guard_ws.stash_ws = c->guardWs.p; lc.guard_ws.stash_wd = c->guardWd.p;
        }
    }
    if (plan.table) {
        // 20 bytes per frame cell, and the row pass' block sums: 20 bytes per column and block of SB_TAB_RB rows
        const size_t nsum = (size_t)((g.nyh + SB_TAB_RB - 1) / SB_TAB_RB) * g.nxh;
        if ((rc = ensure(c, c->tabA, ncell * sizeof(unsigned long long)))) return rc;
        if ((rc = ensure(c, c->tabL, ncell * sizeof(unsigned long long)))) return rc;
        if ((rc = ensure(c, c->tabC, ncell * sizeof(unsigned)))) return rc;
        if ((rc = ensure(c, c->tabS, nsum * (2 * sizeof(unsigned long long) + sizeof(unsigned))))) return rc;
        lc.tables.A = (unsigned long long *)c->tabA.p; lc.tables.L = (unsigned long long *)c->tabL.p; lc.tables.C = (unsigned *)c->tabC.p;
        lc.tables.SA = (unsigned long long *)c->tabS.p; lc.tables.SL = lc.tables.SA + nsum; lc.tables.SC = (unsigned *)(lc.tables.SL + nsum);
    }
    // the stored windows: 4 bytes per interior cell.  Whether this call searches: the host's half here, the device's in the
    // table kernels (sb_tab_fill) -- no synchronisation, no launch
    SbTabKey tkey{};
    if (plan.table && cache) {
        if ((rc = ensure(c, c->tabW, (size_t)g.nx * g.ny * sizeof(unsigned)))) return rc;
        if ((rc = ensure(c, c->tabRep, (SB_TAB_REP_HDR + (size_t)2 * SB_TAB_QUERY_WAVES_PER_CU * c->ncu_dev) * sizeof(unsigned)))) return rc;
        tkey = SbTabKey{g.nx, g.ny, g.h, g.bnd, g.rows, c->bandbits.p, c->clsbits.p, c->tabW.p, c->tabC.p};
        lc.tables.W = (unsigned *)c->tabW.p; lc.tables.rep = (unsigned *)c->tabRep.p;
        lc.tables.gen = job.plan_gen; lc.tables.call_id = job.call_id;
        lc.tables.force = sb_tab_cache_decide(c->tabc, tkey, job.call_id) != SB_TAB_STEADY ? 1 : 0;
        lc.tables.rep_reset = c->tab_rep_reset ? 1 : 0;
    }
    // this call's wind speed / direction at band cells, where k_wind runs ahead of the contrast (k_wind -> k_thc3)
    if (plan.wind_scratch) {
        if ((rc = ensure(c, c->nws, (size_t)g.nx * g.ny * sizeof(T)))) return rc;
        if ((rc = ensure(c, c->nwd, (size_t)g.nx * g.ny * sizeof(T)))) return rc;
        job.nws = (T *)c->nws.p; job.nwd = (T *)c->nwd.p;
    }
    if (phases == 3) c->rep_launches = c->rep_rccl = c->rep_groups = c->rep_copies = 0;   // a band step resets them itself
    {
        const hipError_t le = sb_launch_diag<T>(job, plan, lc);
        if (le != hipSuccess) {
            // nothing the host noted for later calls stands: the stored plan and the segment lists were not (all) made
            c->plan_bits = nullptr;
            c->segs_built = false;
            c->stats_valid = false;
            sb_tab_cache_launch_failed(c->tabc);
        }
        if (le == hipErrorInvalidValue) return fail(c, SB_ERR_ARG, "no contrast kernel instance for this halo / tile shape");
        if (le != hipSuccess) return hipfail(c, le, "sb_launch_diag");
    }
    c->rep_launches += plan.nsteps + (lc.guard.on ? lc.guard.nlaunch : 0);
    if (lc.guard.on) { c->guard_last = true; c->guard_rep_reset = false; ++c->guard_calls; }
    // W belongs to the planes of the last call that ran with the cache in effect: any other call that ran k_scan on them
    // (or a part of a band step) drops the key
    if (lc.tables.W) {
        sb_tab_cache_filled(c->tabc, tkey, job.call_id);
        c->tab_rep_reset = false;
        c->tab_waves = SB_TAB_QUERY_WAVES_PER_CU * c->ncu;
        ++c->tab_calls;
    } else sb_tab_cache_other_call(c->tabc);
    c->tab_last = lc.tables.W != nullptr;
    if (!(phases & 2)) return SB_OK;          // the flag buffers swap when the call is complete
    c->segs_built = plan.segs_built;
    if (c->static_sigma && c->host_depth == 0 && !in.reuse_stats) {
        c->stats_valid = true;
        c->stats_sigma = (const void *)job.sigma;
        c->stats_dims[0] = g.nx; c->stats_dims[1] = g.ny; c->stats_dims[2] = g.h; c->stats_dims[3] = (int)sizeof(T);
        c->stats_ngathered = c->gathered ? c->ngathered : 0;
    }
    c->last_flags = flags_now;
    c->flag_parity = 1 - c->flag_parity;
    c->last_g = g;
    c->last_tiles = ntile;
    c->have_last = true;
    return SB_OK;
}

template <typename T>
int check_dims(sb_ctx *c, int nx, int ny, int nz, int halo, int bnd) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || nz < 1) return fail(c, SB_ERR_ARG, "nx, ny, nz must be >= 1");
    if (bnd < 0 || bnd > 2) return fail(c, SB_ERR_ARG, "unknown boundary rule");
    if (halo < 0 || (halo > 0 && bnd != SB_BND_HALO)) return fail(c, SB_ERR_ARG, "halo > 0 needs SB_BND_HALO");
    if ((double)(nx + 2 * halo) * (double)(ny + 2 * halo) > 2.0e9) return fail(c, SB_ERR_ARG, "grid too large");
    return SB_OK;
}

template <typename T>
int seabreeze_diag_dev(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, int bnd, const T *p,
                       const T *u, const T *v, const T *theta, const T *mask, const T *z, const T *sigma, T *ws,
                       T *wd, T *thc, T *sb_con, const sb_tunables *tun, void *stream, int phases = 3,
                       int mask_halo = -1, int level_rule = 0) {
    int rc = check_dims<T>(c, nx, ny, nz, halo, bnd);
    if (rc) return rc;
    if (!p || !u || !v || !theta || !mask || !z || !sigma || !ws || !wd || !thc || !sb_con)
        return fail(c, SB_ERR_ARG, "null array pointer");
    sb_tunables d;
    sb_default_tunables(&d);
    if (tun) d = *tun;
    DiagJob<T> job{};
    job.g = make_geo<T>(nx, ny, halo, bnd, ny);
    if (bnd == SB_BND_HALO) job.g.band = c->band_geo;    // (a band step whose strip kernel reads no east-west / polar ghost cells of theta)
    job.nz = nz;
    job.flavour = SB_FLAVOUR_GENERIC;
    job.tn = tn;
    // modulo(real(timestep_number)*timestep, target_time) < 0.0001   ref: generic/sea_breeze_diag.f90:264
    const T period = (T)d.target_time_s;
    job.refresh = sb_modulo<T>((T)tn * timestep_s, period) < T(0.0001) ? 1 : 0;
    job.target_plev = (T)d.target_plev_pa; job.thr_wind = (T)d.thresh_wind; job.thr_dir = (T)d.thresh_winddir;
    job.thr_ch = (T)d.thresh_windch; job.thr_thc = (T)d.thresh_thc; job.maxdist = (T)d.maxdist_km;
    job.fill = T(0);                                              // ref :176
    job.p = p; job.u = u; job.v = v; job.theta = theta; job.mask = mask; job.z = z; job.sigma = sigma;
    // mask may sit in a wider ghost frame than theta, z and sigma (UM layout: tdims_l against tdims_s)
    const int hl = mask_halo < 0 ? halo : mask_halo;
    if (hl < halo) return fail(c, SB_ERR_ARG, "the ghost frame of mask must be at least as wide as that of theta, z, sigma");
    job.mask_ld = nx + 2 * hl;
    job.mask_off = (unsigned)((hl - halo) * job.mask_ld + (hl - halo));
    job.level_rule = level_rule;
    job.ws = ws; job.wd = wd; job.thc = thc; job.sb_con = sb_con; job.out = nullptr;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return run_diag<T>(c, job, st, phases);
}

template <typename T>
int sigma_moments_dev(sb_ctx *c, int nx, int ny, int halo, const T *sigma, double *moments5, void *stream);
template <typename T>
int swap_bounds_dev(sb_ctx *c, T *field, int nx, int ny, int halo, void *stream);
template <typename T>
int exchange_rows_dev(sb_ctx *c, T *field, int nx, int ny, int halo, void *stream);

// One model step of a latitude band: the communication (this band's sigma moments and their all-gather, theta's
// ghost rows) runs on the context's second stream while k_scan, k_prep and k_wind, which need neither, run
// on the caller's stream; the two join before k_thc3, which merges the gathered moments in its prologue.
template <typename T>
int band_diag_dev(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, const T *p, const T *u,
                  const T *v, T *theta, const T *mask, const T *z, const T *sigma, T *ws, T *wd, T *thc, T *sb_con,
                  const sb_tunables *tun, void *stream) {
    int rc = check_dims<T>(c, nx, ny, nz, halo, SB_BND_HALO);
    if (rc) return rc;
    if (halo < 1) return fail(c, SB_ERR_ARG, "a band needs ghost cells (halo >= 1)");
    if (!sigma || !theta) return fail(c, SB_ERR_ARG, "null array pointer");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (!c->aux_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_mom, hipEventDisableTiming));
    }
    if ((rc = ensure(c, c->band_mom, (size_t)5 * (c->nranks + 1) * sizeof(double)))) return rc;
    double *mine = (double *)c->band_mom.p, *gath = mine + 5;
    // (the reuse key tells single-domain scalars from a band run's: the gathered moments are in place before it is read)
    const Moments *saved_g = c->gathered;
    const int saved_n = c->ngathered;
    c->gathered = (const Moments *)gath;
    c->ngathered = c->nranks;
    // static sigma (opt-in): the scalars of the first step stand, no moments, no all-gather, no merge
    const bool reuse = reuse_stats<T>(c, sigma, nx, ny, halo);
    c->rep_launches = c->rep_rccl = c->rep_groups = c->rep_copies = 0;
    // fork: everything that talks to the other ranks goes to the second stream: the exchange of theta's ghost rows at
    // once, the all-gather of the sigma moments as soon as k_scan has published this band's (every rank issues the two
    // RCCL operations in this order), while k_scan and k_wind run on the caller's stream.
    hipError_t he = hipEventRecord(c->ev_fork, st);
    if (he == hipSuccess) he = hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0);
    if (he != hipSuccess) { c->gathered = saved_g; c->ngathered = saved_n; c->band_geo = 0; return hipfail(c, he, "band step fork"); }
    // The ghost rows of theta first: they depend on nothing this step computes.  On a strip kernel only the rows that
    // come from a NEIGHBOUR travel: the east-west ghost columns (the periodic wrap of the row itself) and the ghost rows
    // beyond a pole (the edge row again) follow from theta's interior, and the strip kernels take them from there by index
    // arithmetic (Geo::band) -- no fill kernel on the communication stream, three launches per band step (round 3: four,
    // and the fill, running behind the caller's stream's kernels rather than beside them, held the join up).  The tile
    // kernel (double precision, radii beyond 16) reads every ghost cell as filled: the whole swap_bounds for it.
    // The table contrast and the guard for band steps read the whole frame too, and their kernels see plain SB_BND_HALO
    // geometry (Geo::band == 0) -- the one fill launch is what either switch costs a strip kernel here.  One predicate,
    // beside the one that decides which switches serve the two phases below: sb_band_folds_frame, sb_diag_plan.hpp.
    const bool folds = sb_band_folds_frame(c->sw, sb_plan_contrast(plan_input<T>(c, nx, ny)), nx);
    const int band_geo = folds ? (GEO_BAND_EW | (c->rank == 0 ? GEO_BAND_SOUTH : 0) | (c->rank == c->nranks - 1 ? GEO_BAND_NORTH : 0)) : 0;
    rc = folds ? exchange_rows_dev<T>(c, theta, nx, ny, halo, (void *)c->aux_stream)
               : swap_bounds_dev<T>(c, theta, nx, ny, halo, (void *)c->aux_stream);
    c->band_geo = band_geo;
    // Phase 1 on the caller's stream: k_scan -- whose last workgroup merges this band's sigma moments and leaves them for
    // the all-gather (one rank: in the gathered set itself) -- then k_wind.  (The moments used to be formed by a kernel
    // of their own on the communication stream; with the caller's stream filling every CU that kernel ran behind
    // k_scan and k_wind, not beside them, and held the join up by 17 us: profiles/r03_band_step_cost.log.)
    c->band_moments_out = reuse ? nullptr : (Moments *)(c->nranks == 1 ? gath : mine);
    if (!rc) rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, halo, SB_BND_HALO, p, u, v, theta, mask, z, sigma, ws, wd,
                                        thc, sb_con, tun, (void *)st, 1);
    c->band_moments_out = nullptr;
    // The all-gather is enqueued in EVERY step of a multi-rank run, whether or not this rank keeps its sigma statistics
    // (sb_set_static_sigma): whether a rank keeps them is its own business -- its sigma pointer, its shape, the step in
    // which it switched the option -- and ranks that disagreed about a collective used to hang (round 3 documented that as
    // a rule for the caller; now there is nothing to agree on).  A rank that keeps its statistics contributes the moments
    // of its band it formed then (they stand: its sigma did), a rank that forms them anew receives everybody's.
    if (!rc && c->nranks > 1) {
        if (!reuse) {
            he = hipStreamWaitEvent(c->aux_stream, c->ev_mom, 0);      // (recorded behind k_scan by phase 1)
            if (he != hipSuccess) rc = hipfail(c, he, "band step moments event");
        }
        if (!rc) rc = sb_allgather_moments_dev(c, mine, gath, (void *)c->aux_stream);
    }
    // (whatever happened on the way: the second stream is joined into the caller's again)
    he = hipEventRecord(c->ev_join, c->aux_stream);
    if (he == hipSuccess) he = hipStreamWaitEvent(st, c->ev_join, 0);
    if (he != hipSuccess && !rc) rc = hipfail(c, he, "band step join");
    if (!rc) rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, halo, SB_BND_HALO, p, u, v, theta, mask, z, sigma,
                                        ws, wd, thc, sb_con, tun, (void *)st, 2);
    c->gathered = saved_g;
    c->ngathered = saved_n;
    c->band_geo = 0;
    return rc;
}

template <typename T>
int diag_dev(sb_ctx *c, int tn, const T *p, const T *z, const T *std_, const T *theta, const T *v, const T *u,
             const T *cdist, T *ws, T *wd, T *thc, T target_plev, T thresh_wind, T thresh_winddir, T thresh_windch,
             T thresh_thc, T target_time, T maxdist, T timestep, int nps, int nlons, int nlats, T *output,
             void *stream) {
    int rc = check_dims<T>(c, nlons, nlats, nps, 0, SB_BND_WRAPPER);
    if (rc) return rc;
    if (!p || !z || !std_ || !theta || !v || !u || !cdist || !ws || !wd || !thc || !output)
        return fail(c, SB_ERR_ARG, "null array pointer");
    DiagJob<T> job{};
    job.g = make_geo<T>(nlons, nlats, 0, SB_BND_WRAPPER, nlats - 1);   // ref: seabreeze_diag_python.f90:165
    job.nz = nps;
    job.flavour = SB_FLAVOUR_WRAPPER;
    job.tn = tn;
    // unit conversions in the working precision, ref :146-148
    const T dt_s = timestep * T(60.);
    const T period = target_time * (T(60.) * T(60.));
    job.target_plev = target_plev * T(100.);
    job.refresh = sb_modulo<T>((T)tn * dt_s, period) < T(0.0001) ? 1 : 0;   // ref :271
    job.thr_wind = thresh_wind; job.thr_dir = thresh_winddir; job.thr_ch = thresh_windch;
    job.thr_thc = thresh_thc; job.maxdist = maxdist;
    job.fill = T(2.0E20);                                         // ref :173
    job.p = p; job.u = u; job.v = v; job.theta = theta; job.mask = cdist; job.z = z; job.sigma = std_;
    job.mask_ld = nlons; job.mask_off = 0; job.level_rule = 0;
    job.ws = ws; job.wd = wd; job.thc = thc; job.sb_con = nullptr; job.out = output;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (job.g.rows < 1) return SB_OK;                             // nlats == 1: the reference loop is empty
    return run_diag<T>(c, job, st);
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

template <typename T>
int seabreeze_diag_host(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, int bnd, const T *p,
                        const T *u, const T *v, const T *theta, const T *mask, const T *z, const T *sigma, T *ws,
                        T *wd, T *thc, T *sb_con, const sb_tunables *tun) {
    int rc = check_dims<T>(c, nx, ny, nz, halo, bnd);
    if (rc) return rc;
    if (!p || !u || !v || !theta || !mask || !z || !sigma || !ws || !wd || !thc || !sb_con)
        return fail(c, SB_ERR_ARG, "null array pointer");
    const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, n2h = (size_t)(nx + 2 * halo) * (ny + 2 * halo);
    Stager s(c);
    T *dp = s.in(p, n3), *du = s.in(u, n3), *dv = s.in(v, n3);
    T *dth = s.in(theta, n2h), *dm = s.in(mask, n2h), *dz = s.in(z, n2h), *dsg = s.in(sigma, n2h);
    T *dws = s.in(ws, n2), *dwd = s.in(wd, n2), *dthc = s.in(thc, n2), *dsb = s.in(sb_con, n2);
    if (s.rc) return s.rc;
    rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, halo, bnd, dp, du, dv, dth, dm, dz, dsg, dws, dwd,
                               dthc, dsb, tun, nullptr);
    if (rc) return rc;
    s.back(ws, dws, n2); s.back(wd, dwd, n2); s.back(thc, dthc, n2); s.back(sb_con, dsb, n2);
    return s.finish();
}

// UM vn10.7 field layout (ref: UM/vn10.7/sea_breeze_diag.F90:55-117): p, u, v, sb_con on pdims and windspeed,
// winddir, thc on tdims (no ghost cells); theta, z, sigma on tdims_s (ghost width hs); mask on tdims_l (hl >= hs).
template <typename T>
int seabreeze_diag_um_dev(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int hs, int hl, const T *p,
                          const T *u, const T *v, T *theta, const T *z, const T *sigma, const T *mask, T *ws, T *wd,
                          T *thc, T *sb_con, int flags, int *error, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!error) return fail(c, SB_ERR_ARG, "null error pointer");
    *error = 0;
    if (ny < 1 || nz < 1 || nx < 1) { *error = 1; return SB_OK; }           // ref: UM :198-202
    if (hs < 0 || hl < hs) return fail(c, SB_ERR_ARG, "UM layout: need 0 <= halo_s <= halo_l");
    if (flags & ~(SB_UM_THETA_TO_T0 | SB_UM_LEVEL_WALK)) return fail(c, SB_ERR_ARG, "unknown UM flag");
    const int bnd = hs > 0 ? SB_BND_HALO : SB_BND_GLOBAL;
    int rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, hs, bnd, p, u, v, theta, mask, z, sigma, ws, wd, thc,
                                   sb_con, nullptr, stream, 3, hl, (flags & SB_UM_LEVEL_WALK) ? 1 : 0);
    if (rc) return rc;
    if (flags & SB_UM_THETA_TO_T0) {
        hipStream_t st = stream ? (hipStream_t)stream : c->stream;
        HIPCHK(c, sb_launch_theta_to_t0<T>(theta, z, sigma, (size_t)(nx + 2 * hs) * (ny + 2 * hs), (const T *)c->stats, st));
    }
    return SB_OK;
}

template <typename T>
int seabreeze_diag_um_host(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int hs, int hl, const T *p,
                           const T *u, const T *v, T *theta, const T *z, const T *sigma, const T *mask, T *ws, T *wd,
                           T *thc, T *sb_con, int flags, int *error) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!error) return fail(c, SB_ERR_ARG, "null error pointer");
    *error = 0;
    if (ny < 1 || nz < 1 || nx < 1) { *error = 1; return SB_OK; }
    if (hs < 0 || hl < hs) return fail(c, SB_ERR_ARG, "UM layout: need 0 <= halo_s <= halo_l");
    if (!p || !u || !v || !theta || !mask || !z || !sigma || !ws || !wd || !thc || !sb_con)
        return fail(c, SB_ERR_ARG, "null array pointer");
    const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, ns = (size_t)(nx + 2 * hs) * (ny + 2 * hs),
                 nl = (size_t)(nx + 2 * hl) * (ny + 2 * hl);
    Stager s(c);
    T *dp = s.in(p, n3), *du = s.in(u, n3), *dv = s.in(v, n3);
    T *dth = s.in(theta, ns), *dz = s.in(z, ns), *dsg = s.in(sigma, ns), *dm = s.in(mask, nl);
    T *dws = s.in(ws, n2), *dwd = s.in(wd, n2), *dthc = s.in(thc, n2), *dsb = s.in(sb_con, n2);
    if (s.rc) return s.rc;
    int rc = seabreeze_diag_um_dev<T>(c, timestep_s, tn, nx, ny, nz, hs, hl, dp, du, dv, dth, dz, dsg, dm, dws, dwd, dthc,
                                      dsb, flags, error, nullptr);
    if (rc) return rc;
    s.back(ws, dws, n2); s.back(wd, dwd, n2); s.back(thc, dthc, n2); s.back(sb_con, dsb, n2);
    if (flags & SB_UM_THETA_TO_T0) s.back(theta, dth, ns);
    return s.finish();
}

template <typename T>
int diag_host(sb_ctx *c, int tn, const T *p, const T *z, const T *std_, const T *theta, const T *v, const T *u,
              const T *cdist, T *ws, T *wd, T *thc, T target_plev, T thresh_wind, T thresh_winddir, T thresh_windch,
              T thresh_thc, T target_time, T maxdist, T timestep, int nps, int nlons, int nlats, T *output) {
    int rc = check_dims<T>(c, nlons, nlats, nps, 0, SB_BND_WRAPPER);
    if (rc) return rc;
    if (!p || !z || !std_ || !theta || !v || !u || !cdist || !ws || !wd || !thc || !output)
        return fail(c, SB_ERR_ARG, "null array pointer");
    const size_t n2 = (size_t)nlons * nlats;
    // p is one column for the whole grid (ref: seabreeze_diag_python.f90:228), so the level is known
    // before anything is uploaded: pick it here exactly as the kernel would (first minimum, working
    // precision, target converted like ref :148) and send only that u/v plane -- 2 planes instead of
    // 2*nps over PCIe, same result.
    int lev = 0;
    {
        const T tp = target_plev * T(100.);
        T best = std::fabs(p[0] - tp);
        for (int k = 1; k < nps; ++k) {
            const T a = std::fabs(p[k] - tp);
            if (a < best) { best = a; lev = k; }
        }
    }
    Stager s(c);
    T *dp = s.in(p + lev, (size_t)1), *dz = s.in(z, n2), *dsd = s.in(std_, n2), *dth = s.in(theta, n2);
    T *dv = s.in(v + (size_t)lev * n2, n2), *du = s.in(u + (size_t)lev * n2, n2), *dcd = s.in(cdist, n2);
    nps = 1;
    T *dws = s.in(ws, n2), *dwd = s.in(wd, n2), *dthc = s.in(thc, n2);
    T *dout = s.out<T>(4 * n2);              // nothing to upload: the kernels write rows 1..nlats-1 of every plane
    if (s.rc) return s.rc;
    rc = diag_dev<T>(c, tn, dp, dz, dsd, dth, dv, du, dcd, dws, dwd, dthc, target_plev, thresh_wind, thresh_winddir,
                     thresh_windch, thresh_thc, target_time, maxdist, timestep, nps, nlons, nlats, dout, nullptr);
    if (rc) return rc;
    // Only what the call changed travels back.  windspeed / winddir change on the first step and on the
    // steps the target_time branch fires (ref :268-273), thc at the band cells of every step; row nlats
    // of the output planes is never written (ref :165) and stays as the caller passed it.
    const T dt_s = timestep * T(60.), period = target_time * (T(60.) * T(60.));
    const bool refresh = sb_modulo<T>((T)tn * dt_s, period) < T(0.0001);
    if (refresh || tn < 2) { s.back(ws, dws, n2); s.back(wd, dwd, n2); }
    s.back(thc, dthc, n2);
    const size_t nwritten = (size_t)nlons * (nlats > 0 ? nlats - 1 : 0);
    for (int pl = 0; pl < 4 && nwritten > 0; ++pl) s.back(output + (size_t)pl * n2, dout + (size_t)pl * n2, nwritten);
    return s.finish();
}

// ---- streaming diag (f2py flavour): SURVEY.md 8(f) rank 1 ---------------------------------------------------
// The reference's Python driver calls diag once per timestep with the same z, std, cdist and threads windspeed,
// winddir, thc through its return values (ref: python_wrapper/seabreezediag/__init__.py:222-245).  Here those six
// planes stay on the device between sb_diag_stream_begin and sb_diag_stream_end; a step uploads theta and the one
// u, v plane its 1-D p selects through pinned, double-buffered staging (asynchronous copies), and brings back only
// the sb_con plane -- of the PREVIOUS step, so that the host copies of step i+1 overlap the device work of step i.
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void stream_release(sb_ctx *c) {
    DiagStream &d = c->ds;
    for (DevBuf *b : {&d.z, &d.sd, &d.cdist, &d.ws, &d.wd, &d.thc, &d.p1, &d.theta, &d.v, &d.u, &d.out, &d.lsm, &d.ice, &d.icebits,
                      &d.icemarks, &d.icecoast})
        if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    for (int k = 0; k < 2; ++k) {
        if (d.pin_ice[k]) (void)hipHostFree(d.pin_ice[k]);
        if (d.ev_ice[k]) (void)hipEventDestroy(d.ev_ice[k]);
        if (d.ev_ice_t[k]) (void)hipEventDestroy(d.ev_ice_t[k]);
        d.ev_ice_t[k] = nullptr;
        d.pin_ice[k] = nullptr;
        d.ev_ice[k] = nullptr;
        if (d.pin_in[k]) (void)hipHostFree(d.pin_in[k]);
        if (d.pin_out[k]) (void)hipHostFree(d.pin_out[k]);
        if (d.ev_in[k]) (void)hipEventDestroy(d.ev_in[k]);
        if (d.ev_out[k]) (void)hipEventDestroy(d.ev_out[k]);
        d.pin_in[k] = d.pin_out[k] = nullptr;
        d.ev_in[k] = d.ev_out[k] = nullptr;
    }
    d.pin_in_cap = d.pin_out_cap = d.pin_ice_cap = 0;
    d.active = false;
    d.ice_ready = false;
    delete d.pool;
    d.pool = nullptr;
}

template <typename T>
int stream_begin(sb_ctx *c, int nlons, int nlats, const T *z, const T *sd, const T *cdist, const T *ws, const T *wd,
                 const T *thc) {
    int rc = check_dims<T>(c, nlons, nlats, 1, 0, SB_BND_WRAPPER);
    if (rc) return rc;
    if (!z || !sd || !cdist || !ws || !wd || !thc) return fail(c, SB_ERR_ARG, "null array pointer");
    DiagStream &d = c->ds;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stats_valid = false;                 // a new std field arrives in the same device buffer
    const size_t n2 = (size_t)nlons * nlats, b2 = n2 * sizeof(T);
    for (DevBuf *b : {&d.z, &d.sd, &d.cdist, &d.ws, &d.wd, &d.thc, &d.theta, &d.v, &d.u})
        if ((rc = ensure(c, *b, b2))) return rc;
    if ((rc = ensure(c, d.out, 4 * b2))) return rc;
    if ((rc = ensure(c, d.p1, 16))) return rc;
    const size_t in_bytes = 3 * b2 + 16, out_bytes = b2;
    if (d.pin_in_cap < in_bytes || d.pin_out_cap < out_bytes) {
        for (int k = 0; k < 2; ++k) {
            if (d.pin_in[k]) (void)hipHostFree(d.pin_in[k]);
            if (d.pin_out[k]) (void)hipHostFree(d.pin_out[k]);
            d.pin_in[k] = d.pin_out[k] = nullptr;
            HIPCHK(c, hipHostMalloc(&d.pin_in[k], in_bytes, hipHostMallocDefault));
            HIPCHK(c, hipHostMalloc(&d.pin_out[k], out_bytes, hipHostMallocDefault));
        }
        d.pin_in_cap = in_bytes;
        d.pin_out_cap = out_bytes;
    }
    for (int k = 0; k < 2; ++k) {
        if (!d.ev_in[k]) HIPCHK(c, hipEventCreateWithFlags(&d.ev_in[k], hipEventDisableTiming));
        if (!d.ev_out[k]) HIPCHK(c, hipEventCreateWithFlags(&d.ev_out[k], hipEventDisableTiming));
    }
    const T *src[6] = {z, sd, cdist, ws, wd, thc};
    DevBuf *dst[6] = {&d.z, &d.sd, &d.cdist, &d.ws, &d.wd, &d.thc};
    for (int i = 0; i < 6; ++i) HIPCHK(c, hipMemcpyAsync(dst[i]->p, src[i], b2, hipMemcpyHostToDevice, c->stream));
    // the output planes start from zero: row nlats of every plane is never written by the kernels (ref :165)
    HIPCHK(c, hipMemsetAsync(d.out.p, 0, 4 * b2, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!d.pool) {
        unsigned hw = std::thread::hardware_concurrency();
        d.pool = new HostPool((int)std::min(7u, hw > 1 ? hw - 1 : 1u));       // + the calling thread
    }
    d.nlons = nlons; d.nlats = nlats; d.esz = (int)sizeof(T);
    d.steps = 0;
    d.host_copy_s = d.enqueue_s = d.wait_s = 0.0;
    d.active = true;
    d.ice_ready = false;                    // a moving coast is asked for per stream (sb_diag_stream_coast)
    return SB_OK;
}

// sb_con of the step in `slot` -> rows 1..nlats-1 of a caller's double plane (what the reference's driver keeps)
template <typename T>
void stream_copy_out(const DiagStream &d, int slot, double *dst) {
    const T *src = (const T *)d.pin_out[slot];
    const size_t n = (size_t)d.nlons * (d.nlats > 0 ? d.nlats - 1 : 0);
    const int parts = d.pool ? d.pool->threads() : 1;
    auto range = [&](int k) {
        const size_t a = n * (size_t)k / parts, b = n * (size_t)(k + 1) / parts;
        for (size_t i = a; i < b; ++i) dst[i] = (double)src[i];
    };
    if (d.pool && n >= (size_t)1 << 16) d.pool->run(parts, range);
    else
        for (int k = 0; k < parts; ++k) range(k);
}

template <typename T>
int stream_step(sb_ctx *c, int tn, const T *p, int nps, const T *theta, const T *v, const T *u, T target_plev,
                T thresh_wind, T thresh_winddir, T thresh_windch, T thresh_thc, T target_time, T maxdist, T timestep,
                double *sb_con_prev, int *have_prev) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    DiagStream &d = c->ds;
    if (!d.active || d.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_diag_stream_step without a matching sb_diag_stream_begin");
    if (!p || nps < 1 || !theta || !v || !u || !have_prev) return fail(c, SB_ERR_ARG, "bad stream_step arguments");
    const size_t n2 = (size_t)d.nlons * d.nlats, b2 = n2 * sizeof(T);
    int lev = 0;                                                 // as diag_host: the level is known on the host
    {
        const T tp = target_plev * T(100.);
        T best = std::fabs(p[0] - tp);
        for (int k = 1; k < nps; ++k) {
            const T a = std::fabs(p[k] - tp);
            if (a < best) { best = a; lev = k; }
        }
    }
    const int slot = (int)(d.steps & 1);
    double t0 = now_s();
    // the staging slot was last read by the upload of two steps ago
    if (d.steps >= 2) HIPCHK(c, hipEventSynchronize(d.ev_in[slot]));
    double t1 = now_s();
    d.wait_s += t1 - t0;
    char *pin = (char *)d.pin_in[slot];
    {
        // three planes cut into ranges for the pool's threads: a single memcpy stream would be the longest item of the step
        const char *src[3] = {(const char *)theta, (const char *)(v + (size_t)lev * n2), (const char *)(u + (size_t)lev * n2)};
        const int per = d.pool && b2 >= ((size_t)1 << 18) ? std::max(1, d.pool->threads() / 3 + (d.pool->threads() % 3 ? 1 : 0)) : 1;
        auto piece = [&](int k) {
            const int f = k / per, j = k % per;
            const size_t a = b2 * (size_t)j / per, b = b2 * (size_t)(j + 1) / per;
            std::memcpy(pin + (size_t)f * b2 + a, src[f] + a, b - a);
        };
        if (d.pool && per * 3 > 1) d.pool->run(3 * per, piece);
        else for (int k = 0; k < 3; ++k) piece(k);
        std::memcpy(pin + 3 * b2, p + lev, sizeof(T));
    }
    double t2 = now_s();
    d.host_copy_s += t2 - t1;
    HIPCHK(c, hipMemcpyAsync(d.theta.p, pin, b2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.v.p, pin + b2, b2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.u.p, pin + 2 * b2, b2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.p1.p, pin + 3 * b2, sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(d.ev_in[slot], c->stream));
    int rc = diag_dev<T>(c, tn, (const T *)d.p1.p, (const T *)d.z.p, (const T *)d.sd.p, (const T *)d.theta.p,
                         (const T *)d.v.p, (const T *)d.u.p, (const T *)d.cdist.p, (T *)d.ws.p, (T *)d.wd.p, (T *)d.thc.p,
                         target_plev, thresh_wind, thresh_winddir, thresh_windch, thresh_thc, target_time, maxdist,
                         timestep, 1, d.nlons, d.nlats, (T *)d.out.p, nullptr);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d.pin_out[slot], d.out.p, b2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(d.ev_out[slot], c->stream));
    double t3 = now_s();
    d.enqueue_s += t3 - t2;
    // the previous step's sb_con: its copy finished while this step's planes were being staged
    *have_prev = 0;
    if (d.steps > 0 && sb_con_prev) {
        HIPCHK(c, hipEventSynchronize(d.ev_out[1 - slot]));
        double t4 = now_s();
        d.wait_s += t4 - t3;
        stream_copy_out<T>(d, 1 - slot, sb_con_prev);
        d.host_copy_s += now_s() - t4;
        *have_prev = 1;
    }
    d.steps++;
    return SB_OK;
}

template <typename T>
int stream_end(sb_ctx *c, double *sb_con_last, T *output4, T *ws, T *wd, T *thc) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    DiagStream &d = c->ds;
    if (!d.active || d.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_diag_stream_end without a matching sb_diag_stream_begin");
    const size_t n2 = (size_t)d.nlons * d.nlats, b2 = n2 * sizeof(T);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (d.steps > 0 && sb_con_last) stream_copy_out<T>(d, (int)((d.steps - 1) & 1), sb_con_last);
    if (output4) HIPCHK(c, hipMemcpyAsync(output4, d.out.p, 4 * b2, hipMemcpyDeviceToHost, c->stream));
    if (ws) HIPCHK(c, hipMemcpyAsync(ws, d.ws.p, b2, hipMemcpyDeviceToHost, c->stream));
    if (wd) HIPCHK(c, hipMemcpyAsync(wd, d.wd.p, b2, hipMemcpyDeviceToHost, c->stream));
    if (thc) HIPCHK(c, hipMemcpyAsync(thc, d.thc.p, b2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    d.active = false;
    return SB_OK;
}

template <typename T>
int sigmoid_dev(sb_ctx *c, int nx, int ny, const T *ary, T *sm, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !ary || !sm) return fail(c, SB_ERR_ARG, "bad sigmoid arguments");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    c->stats_valid = false;                 // the shared scalars now belong to `ary`, not to a diag call's sigma
    HIPCHK(c, sb_launch_stats<T>(ary, nx, ny, nx, 0, c->partials, (T *)c->stats, nullptr, (int *)c->ticket + 1, st));
    HIPCHK(c, sb_launch_sigmoid_apply<T>(ary, sm, (size_t)nx * ny, (const T *)c->stats, st));
    return SB_OK;
}

template <typename T>
int sigmoid_host(sb_ctx *c, int nx, int ny, const T *ary, T *sm) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !ary || !sm) return fail(c, SB_ERR_ARG, "bad sigmoid arguments");
    const size_t n = (size_t)nx * ny;
    Stager s(c);
    T *da = s.in(ary, n), *ds = s.out<T>(n);
    if (s.rc) return s.rc;
    int rc = sigmoid_dev<T>(c, nx, ny, da, ds, nullptr);
    if (rc) return rc;
    s.back(sm, ds, n);
    return s.finish();
}

template <typename T>
int sigma_moments_dev(sb_ctx *c, int nx, int ny, int halo, const T *sigma, double *moments5, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || halo < 0 || !sigma || !moments5) return fail(c, SB_ERR_ARG, "bad sigma_moments arguments");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const int nxh = nx + 2 * halo;
    HIPCHK(c, sb_launch_stats<T>(sigma, nx, ny, nxh, (size_t)halo * nxh + halo, c->partials, (T *)c->stats,
                                 (Moments *)moments5, (int *)c->ticket + 1, st));
    return SB_OK;
}

template <typename T>
int get_edges_dev(sb_ctx *c, int nx, int ny, const T *lsm, const T *ci, int rule, int bnd, T *coast, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !lsm || !ci || !coast) return fail(c, SB_ERR_ARG, "bad get_edges arguments");
    if (rule < 0 || rule > 1) return fail(c, SB_ERR_ARG, "unknown mask rule");
    if (bnd != SB_BND_WRAPPER && bnd != SB_BND_GLOBAL) return fail(c, SB_ERR_ARG, "get_edges: boundary must be WRAPPER or GLOBAL");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, sb_launch_edges<T>(lsm, ci, coast, nx, ny, rule, bnd, st));
    return SB_OK;
}

template <typename T>
int get_edges_host(sb_ctx *c, int nx, int ny, const T *lsm, const T *ci, int rule, int bnd, T *coast) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !lsm || !ci || !coast) return fail(c, SB_ERR_ARG, "bad get_edges arguments");
    const size_t n = (size_t)nx * ny;
    Stager s(c);
    T *dl = s.in(lsm, n), *dc = s.in(ci, n), *dco = s.out<T>(n);
    if (s.rc) return s.rc;
    int rc = get_edges_dev<T>(c, nx, ny, dl, dc, rule, bnd, dco, nullptr);
    if (rc) return rc;
    s.back(coast, dco, n);
    return s.finish();
}

// window half-width from the grid spacing at 70 degrees, ref: sobel.f90:129-137
template <typename T>
int dist_window(int nx, int ny, const T *lon, const T *lat, T maxdist, int *k) {
    if (nx < 2 || ny < 2 || !lon || !lat || !k) return fail(nullptr, SB_ERR_ARG, "bad dist_window arguments");
    const T R = T(6370.9989), pi = T(3.1415926), d2r = pi / T(180.0);
    int tlat = 0;
    T best = std::fabs(T(70) - lat[0]);
    for (int i = 1; i < ny; ++i) {
        const T a = std::fabs(T(70) - lat[i]);
        if (a < best) { best = a; tlat = i; }
    }
    if (tlat + 1 >= ny) return fail(nullptr, SB_ERR_ARG, "latitude nearest 70 deg is the last row (the reference reads out of bounds there)");
    const T p0 = d2r * lat[tlat], p1 = d2r * lat[tlat + 1];
    const T dphi = p1 - p0, dlam = d2r * lon[1] - d2r * lon[0];
    const T sp = std::sin(dphi / T(2)), sl = std::sin(dlam / T(2));
    const T a = sp * sp + (std::cos(p1) * (std::cos(p0) * (sl * sl)));
    const T dx = (R * T(2)) * std::atan2(std::sqrt(a), std::sqrt(T(1) - a));
    *k = (int)(maxdist / dx);
    return SB_OK;
}

// The coordinate tables on the device -- phi = d2r*lat, the folded longitudes in radians (ref: sobel.f90:130,165-174),
// sin and cos of half of them (k_dist_bits, fp64) -- and what the host derives from the coordinates (may the kernel keep
// only the nearest hit per side of a row?) stand for as long as the coordinates do: they are keyed on the CONTENT of
// lon and lat (a byte comparison of two short vectors), made and uploaded when it changes, and left alone otherwise --
// a `_dev` call then enqueues two kernels and returns, without a copy and without a synchronisation (round 3
// recomputed, uploaded and waited in every call: a third of get_dist's 230 us).
// lat: the ny latitudes of the SOURCE rows -- the whole grid's, or (sb_band_get_dist_*) the entries of a band's frame rows
// that may hold a source; nothing else of the caller's vector is looked at.
template <typename T>
int dist_tables(sb_ctx *c, int nx, int ny, const T *lon, const T *lat, hipStream_t st) {
    const size_t kb = ((size_t)nx + ny) * sizeof(T);
    bool same = c->dist_key.size() == kb + 3 * sizeof(int) && c->vecs.p != nullptr;
    const int dims[3] = {nx, ny, (int)sizeof(T)};
    if (same) same = std::memcmp(c->dist_key.data(), dims, sizeof(dims)) == 0 &&
                     std::memcmp(c->dist_key.data() + sizeof(dims), lon, (size_t)nx * sizeof(T)) == 0 &&
                     std::memcmp(c->dist_key.data() + sizeof(dims) + (size_t)nx * sizeof(T), lat, (size_t)ny * sizeof(T)) == 0;
    int rc;
    if (!same) {
        // (the tables of the call before may still be on their way from the host vector that is rewritten now)
        if (!c->dist_hv.empty()) HIPCHK(c, hipDeviceSynchronize());
        c->dist_key.clear();
        const T pi = T(3.1415926), d2r = pi / T(180.0);
        c->dist_hv.resize(((size_t)3 * nx + ny) * sizeof(T));
        T *hv = (T *)c->dist_hv.data();
        for (int i = 0; i < ny; ++i) hv[i] = d2r * lat[i];
        for (int j = 0; j < nx; ++j) hv[ny + j] = (lon[j] > T(180)) ? d2r * (lon[j] - T(360.)) : d2r * lon[j];
        for (int j = 0; j < nx; ++j) { hv[ny + nx + j] = std::sin(hv[ny + j] / T(2)); hv[ny + 2 * (size_t)nx + j] = std::cos(hv[ny + j] / T(2)); }
        if ((rc = ensure(c, c->vecs, c->dist_hv.size()))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->vecs.p, hv, c->dist_hv.size(), hipMemcpyHostToDevice, st));   // (dist_hv lives on with the context)
        c->dist_upload_stream = st;
        c->dist_traits = sb_dist_traits<T>(lon, lat, nx, ny);
        c->dist_key.resize(kb + sizeof(dims));
        std::memcpy(c->dist_key.data(), dims, sizeof(dims));
        std::memcpy(c->dist_key.data() + sizeof(dims), lon, (size_t)nx * sizeof(T));
        std::memcpy(c->dist_key.data() + sizeof(dims) + (size_t)nx * sizeof(T), lat, (size_t)ny * sizeof(T));
    }
    if (same && c->dist_upload_stream && c->dist_upload_stream != st) {
        // (the tables were uploaded on another stream: once, make sure they have landed before this stream reads them)
        HIPCHK(c, hipStreamSynchronize(c->dist_upload_stream));
        c->dist_upload_stream = nullptr;
    }
    return SB_OK;
}

template <typename T>
int get_dist_dev(sb_ctx *c, int nx, int ny, const T *coast, const T *mask, const T *lon, const T *lat, T maxdist,
                 int kwin, T *cdist, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !coast || !mask || !lon || !lat || !cdist)
        return fail(c, SB_ERR_ARG, "bad get_dist arguments");
    int k = kwin;
    if (kwin < 0) {
        int rc = dist_window<T>(nx, ny, lon, lat, maxdist, &k);
        if (rc) { c->err = g_err; return rc; }
    }
    if (k > SB_DIST_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "get_dist: window half-width " + std::to_string(k) + " exceeds SB_DIST_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_MAX_WINDOW) + " cells");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    int rc;
    if ((rc = dist_tables<T>(c, nx, ny, lon, lat, st))) return rc;
    const T *dphi = (const T *)c->vecs.p, *dlam = dphi + ny;
    if ((rc = ensure(c, c->coastbits, (size_t)ny * ((nx + 63) / 64) * sizeof(uint64_t)))) return rc;
    HIPCHK(c, sb_launch_dist<T>(coast, mask, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx, cdist, nx, ny, k, maxdist,
                                (uint64_t *)c->coastbits.p, sb_dist_cuts(c->dist_traits, k), st));
    // a distance field made here bounds the search radius of the following diag calls
    c->radius_hint = k + 1;
    return SB_OK;
}

template <typename T>
int get_dist_host(sb_ctx *c, int nx, int ny, const T *coast, const T *mask, const T *lon, const T *lat, T maxdist,
                  int kwin, T *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !coast || !mask || !lon || !lat || !cdist)
        return fail(c, SB_ERR_ARG, "bad get_dist arguments");
    const size_t n = (size_t)nx * ny;
    Stager s(c);
    T *dco = s.in(coast, n), *dm = s.in(mask, n), *dcd = s.out<T>(n);
    if (s.rc) return s.rc;
    int rc = get_dist_dev<T>(c, nx, ny, dco, dm, lon, lat, maxdist, kwin, dcd, nullptr);
    if (rc) return rc;
    s.back(cdist, dcd, n);
    return s.finish();
}

// ---- a stream whose coast moves with the sea ice (sb_diag_stream_coast_*, sb_diag_stream_ice_*) ----
// The reference's driver forms get_edges(lsm, ci[ts]) and get_dist(coast, lsm, ...) at every timestep (ref:
// python_wrapper/seabreezediag/__init__.py:222-245).  Here the stream keeps lsm, the coast as a bit plane and cdist on the
// device; an ice call stages the plane through pinned memory like a step's planes and enqueues the update on the
// context's stream, in order between the steps: k_edge_bits_delta and the distance kernel over the marked tiles
// (sb_ice_plan.hpp says which path, and what a changed word reaches).  k_scan of the next step compares the band planes
// with what the step before left, so the stored plans and windows follow the rewritten cdist by themselves.
template <typename T>
int stream_coast(sb_ctx *c, const T *lsm, const T *lon, const T *lat, T maxdist, int incremental) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    DiagStream &d = c->ds;
    if (!d.active || d.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_diag_stream_coast without a matching sb_diag_stream_begin");
    if (d.steps != 0 || d.ice_ready) return fail(c, SB_ERR_ARG, "sb_diag_stream_coast: once, between sb_diag_stream_begin and the first step");
    if (!lsm || !lon || !lat) return fail(c, SB_ERR_ARG, "null array pointer");
    const int nx = d.nlons, ny = d.nlats;
    int k = 0, rc = dist_window<T>(nx, ny, lon, lat, maxdist, &k);
    if (rc) { c->err = g_err; return rc; }
    if (k > SB_DIST_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "sb_diag_stream_coast: window half-width " + std::to_string(k) + " exceeds SB_DIST_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_MAX_WINDOW) + " cells");
    const size_t b2 = (size_t)nx * ny * sizeof(T), bitbytes = (size_t)ny * ((nx + 63) / 64) * sizeof(uint64_t);
    const size_t markbytes = ((size_t)ny * sb_ice_tiles(nx) + 3) & ~(size_t)3;
    if ((rc = ensure(c, d.lsm, b2)) || (rc = ensure(c, d.ice, b2)) || (rc = ensure(c, d.icebits, bitbytes)) ||
        (rc = ensure(c, d.icemarks, markbytes + 4 * sizeof(unsigned))))
        return rc;
    if (sb_ice_path(nx, k, incremental) == SbIcePath::WHOLE && (rc = ensure(c, d.icecoast, b2))) return rc;
    if (d.pin_ice_cap < b2) {
        for (int s = 0; s < 2; ++s) {
            if (d.pin_ice[s]) (void)hipHostFree(d.pin_ice[s]);
            d.pin_ice[s] = nullptr;
            d.pin_ice_cap = 0;
            HIPCHK(c, hipHostMalloc(&d.pin_ice[s], b2, hipHostMallocDefault));
        }
        d.pin_ice_cap = b2;
    }
    for (int s = 0; s < 2; ++s) {
        if (!d.ev_ice[s]) HIPCHK(c, hipEventCreateWithFlags(&d.ev_ice[s], hipEventDisableTiming));
        if (!d.ev_ice_t[s]) HIPCHK(c, hipEventCreate(&d.ev_ice_t[s]));
    }
    if ((rc = dist_tables<T>(c, nx, ny, lon, lat, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(d.lsm.p, lsm, b2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d.icebits.p, 0, bitbytes, c->stream));           // the empty coast: the first ice call differs from it
    HIPCHK(c, hipMemsetAsync((char *)d.icemarks.p + markbytes, 0, 4 * sizeof(unsigned), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                // (lsm is the caller's pageable array)
    d.ice_lonlat.resize(((size_t)nx + ny) * sizeof(T));
    std::memcpy(d.ice_lonlat.data(), lon, (size_t)nx * sizeof(T));
    std::memcpy(d.ice_lonlat.data() + (size_t)nx * sizeof(T), lat, (size_t)ny * sizeof(T));
    d.ice_k = k; d.ice_incremental = incremental ? 1 : 0; d.ice_maxdist = (double)maxdist;
    d.ice_mark_bytes = markbytes;
    d.ice_calls = 0;
    d.ice_ready = true;
    c->radius_hint = k + 1;                 // as get_dist_dev: the distance field bounds the search radius of the steps
    return SB_OK;
}

template <typename T>
int stream_ice(sb_ctx *c, const T *ci) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    DiagStream &d = c->ds;
    if (!d.active || d.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_diag_stream_ice without a matching sb_diag_stream_begin");
    if (!d.ice_ready) return fail(c, SB_ERR_ARG, "sb_diag_stream_ice without sb_diag_stream_coast");
    if (!ci) return fail(c, SB_ERR_ARG, "null array pointer");
    const int nx = d.nlons, ny = d.nlats, k = d.ice_k;
    const size_t b2 = (size_t)nx * ny * sizeof(T);
    const int slot = (int)(d.ice_calls & 1), first = d.ice_calls == 0 ? 1 : 0;
    double t0 = now_s();
    if (d.ice_calls >= 2) HIPCHK(c, hipEventSynchronize(d.ev_ice[slot]));      // the slot's upload of two ice calls ago
    double t1 = now_s();
    d.wait_s += t1 - t0;
    {
        char *pin = (char *)d.pin_ice[slot];
        const char *src = (const char *)ci;
        const int parts = d.pool && b2 >= ((size_t)1 << 18) ? d.pool->threads() : 1;
        auto piece = [&](int j) {
            const size_t a = b2 * (size_t)j / parts, b = b2 * (size_t)(j + 1) / parts;
            std::memcpy(pin + a, src + a, b - a);
        };
        if (parts > 1) d.pool->run(parts, piece);
        else piece(0);
    }
    double t2 = now_s();
    d.host_copy_s += t2 - t1;
    hipStream_t st = c->stream;
    HIPCHK(c, hipEventRecord(d.ev_ice_t[0], st));
    HIPCHK(c, hipMemcpyAsync(d.ice.p, d.pin_ice[slot], b2, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(d.ev_ice[slot], st));
    // (the tables are keyed on the coordinates' content: another get_dist call on this context may have replaced them)
    const T *lon = (const T *)d.ice_lonlat.data(), *lat = lon + nx;
    int rc;
    if ((rc = dist_tables<T>(c, nx, ny, lon, lat, st))) return rc;
    const T *dphi = (const T *)c->vecs.p, *dlam = dphi + ny;
    const int cuts = sb_dist_cuts(c->dist_traits, k);
    const T maxdist = (T)d.ice_maxdist;
    if (sb_ice_path(nx, k, d.ice_incremental) == SbIcePath::WHOLE) {
        HIPCHK(c, sb_launch_edges<T>((const T *)d.lsm.p, (const T *)d.ice.p, (T *)d.icecoast.p, nx, ny, 0, BND_WRAPPER, st));
        HIPCHK(c, sb_launch_dist<T>((const T *)d.icecoast.p, (const T *)d.lsm.p, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx,
                                    (T *)d.cdist.p, nx, ny, k, maxdist, (uint64_t *)d.icebits.p, cuts, st));
    } else {
        unsigned char *marks = (unsigned char *)d.icemarks.p;
        unsigned *rep = (unsigned *)(marks + d.ice_mark_bytes);
        // the first call computes everything: every tile marked by the host; rep[0] cleared either way
        if (first) {
            HIPCHK(c, hipMemsetAsync(marks, 1, d.ice_mark_bytes, st));
            HIPCHK(c, hipMemsetAsync(rep, 0, sizeof(unsigned), st));
        } else
            HIPCHK(c, hipMemsetAsync(marks, 0, d.ice_mark_bytes + sizeof(unsigned), st));
        HIPCHK(c, sb_launch_edge_bits_delta<T>((const T *)d.lsm.p, (const T *)d.ice.p, (uint64_t *)d.icebits.p, marks, rep, nx, ny, k,
                                               first, st));
        HIPCHK(c, sb_launch_dist_dirty<T>((const T *)d.lsm.p, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx, (T *)d.cdist.p, nx, ny, k,
                                          maxdist, (const uint64_t *)d.icebits.p, cuts, marks, st));
    }
    HIPCHK(c, hipEventRecord(d.ev_ice_t[1], st));
    c->radius_hint = k + 1;
    d.ice_calls++;
    d.enqueue_s += now_s() - t2;
    return SB_OK;
}

template <typename T>
int stream_get_cdist(sb_ctx *c, T *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    DiagStream &d = c->ds;
    if (!d.active || d.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_diag_stream_get_cdist without a matching sb_diag_stream_begin");
    if (!cdist) return fail(c, SB_ERR_ARG, "null array pointer");
    HIPCHK(c, hipMemcpyAsync(cdist, d.cdist.p, (size_t)d.nlons * d.nlats * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SB_OK;
}

// ---- the coast setup of one latitude band (sb_band_get_edges_*, sb_band_get_dist_*) ----
// Fields in the band step's frame, (nx + 2*halo) x (ny + 2*halo) with the interior at (halo, halo); the interior comes out
// as rows of the whole-grid call's field.  What is read beyond the band's own rows: at a cut side one ghost row (edges),
// kwin ghost rows of coast (distance); at a pole side nothing -- the kernels clamp (edges) or end their source range
// (distance) there as on the globe.
template <typename T>
int check_band_edges(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *lsm, const T *ci, int rule, T *coast) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || halo < 0 || !lsm || !ci || !coast) return fail(c, SB_ERR_ARG, "bad band_get_edges arguments");
    if (rule < 0 || rule > 1) return fail(c, SB_ERR_ARG, "unknown mask rule");
    if ((!south || !north) && halo < 1)
        return fail(c, SB_ERR_ARG, "band_get_edges: a cut side needs halo >= 1 (the Sobel reads the neighbour band's edge row)");
    return SB_OK;
}

template <typename T>
int band_get_edges_dev(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *lsm, const T *ci, int rule,
                       T *coast, void *stream) {
    int rc = check_band_edges<T>(c, nx, ny, halo, south, north, lsm, ci, rule, coast);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, sb_launch_edges_band<T>(lsm, ci, coast, nx, ny, halo, south ? 1 : 0, north ? 1 : 0, rule, st));
    return SB_OK;
}

template <typename T>
int band_get_edges_host(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *lsm, const T *ci, int rule,
                        T *coast) {
    int rc = check_band_edges<T>(c, nx, ny, halo, south, north, lsm, ci, rule, coast);
    if (rc) return rc;
    const size_t n = (size_t)(nx + 2 * halo) * (ny + 2 * halo);
    Stager s(c);
    T *dl = s.in(lsm, n), *dc = s.in(ci, n), *dco = s.in((const T *)coast, n);   // (coast in as well: its ghost cells stay)
    if (s.rc) return s.rc;
    rc = band_get_edges_dev<T>(c, nx, ny, halo, south, north, dl, dc, rule, dco, nullptr);
    if (rc) return rc;
    s.back(coast, dco, n);
    return s.finish();
}

template <typename T>
int check_band_dist(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *coast, const T *mask, const T *lon,
                    const T *lat, int kwin, T *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || halo < 0 || !coast || !mask || !lon || !lat || !cdist)
        return fail(c, SB_ERR_ARG, "bad band_get_dist arguments");
    if (kwin < 0)
        return fail(c, SB_ERR_ARG, "band_get_dist: kwin must be given (the derived half-width needs the global latitudes: "
                                   "sb_dist_window_* on those)");
    if (kwin > SB_DIST_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "band_get_dist: window half-width " + std::to_string(kwin) + " exceeds SB_DIST_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_MAX_WINDOW) + " cells");
    if ((!south || !north) && kwin > halo)
        return fail(c, SB_ERR_ARG, "band_get_dist: a cut side needs kwin <= halo (the window reads kwin ghost rows of coast), got kwin = " +
                                       std::to_string(kwin) + ", halo = " + std::to_string(halo));
    const size_t n = (size_t)(nx + 2 * halo) * (ny + 2 * halo);
    const uintptr_t a = (uintptr_t)coast, b = (uintptr_t)cdist;
    if (a < b + n * sizeof(T) && b < a + n * sizeof(T))
        return fail(c, SB_ERR_ARG, "band_get_dist: coast and cdist overlap (a window reads coast's ghost rows, which are the "
                                   "neighbour band's cells)");
    return SB_OK;
}

template <typename T>
int band_get_dist_dev(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *coast, const T *mask, const T *lon,
                      const T *lat, T maxdist, int kwin, T *cdist, void *stream) {
    int rc = check_band_dist<T>(c, nx, ny, halo, south, north, coast, mask, lon, lat, kwin, cdist);
    if (rc) return rc;
    // the source rows: frame rows f0 .. f0 + nys - 1, the band's own and kwin ghost rows on each cut side; the targets are
    // source rows r0 .. r1 - 1.  The tables, their key and the traits see those rows' latitudes only.
    const int k = kwin, ld = nx + 2 * halo;
    const SbBandRows br = sb_band_rows(ny, halo, south != 0, north != 0, k);
    const int f0 = br.f0, nys = br.nys, r0 = br.r0, r1 = br.r1;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if ((rc = dist_tables<T>(c, nx, nys, lon, lat + f0, st))) return rc;
    const T *dphi = (const T *)c->vecs.p, *dlam = dphi + nys;
    if ((rc = ensure(c, c->coastbits, (size_t)nys * ((nx + 63) / 64) * sizeof(uint64_t)))) return rc;
    const size_t o = (size_t)f0 * ld + halo;
    HIPCHK(c, sb_launch_dist_band<T>(coast + o, mask + o, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx, cdist + o, nx, nys, r0, r1,
                                     ld, k, maxdist, (uint64_t *)c->coastbits.p, sb_dist_cuts(c->dist_traits, k), st));
    c->radius_hint = k + 1;
    return SB_OK;
}

template <typename T>
int band_get_dist_host(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *coast, const T *mask, const T *lon,
                       const T *lat, T maxdist, int kwin, T *cdist) {
    int rc = check_band_dist<T>(c, nx, ny, halo, south, north, coast, mask, lon, lat, kwin, cdist);
    if (rc) return rc;
    const size_t n = (size_t)(nx + 2 * halo) * (ny + 2 * halo);
    Stager s(c);
    T *dco = s.in(coast, n), *dm = s.in(mask, n), *dcd = s.in((const T *)cdist, n);   // (cdist in as well: its ghost cells stay)
    if (s.rc) return s.rc;
    rc = band_get_dist_dev<T>(c, nx, ny, halo, south, north, dco, dm, lon, lat, maxdist, kwin, dcd, nullptr);
    if (rc) return rc;
    s.back(cdist, dcd, n);
    return s.finish();
}

// ---- search_radius: every band cell's window radius from mask alone (sb_radius_kernels.hip) ----
// band < 0: the whole-grid form under rule bnd; else the band step's frame (SB_BND_HALO) with GEO_BAND_* = band.
template <typename T>
int check_search_radius(sb_ctx *c, int nx, int ny, int halo, int bnd, const T *mask, const int *radius, const long long *summary,
                        const long long *hist, int nhist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || halo < 0 || !mask) return fail(c, SB_ERR_ARG, "bad search_radius arguments");
    if (bnd != BND_WRAPPER && bnd != BND_GLOBAL && bnd != BND_HALO) return fail(c, SB_ERR_ARG, "unknown boundary rule");
    if (bnd != BND_HALO && halo != 0) return fail(c, SB_ERR_ARG, "halo must be 0 unless bnd == SB_BND_HALO");
    if (hist && nhist != 0 && nhist < 2) return fail(c, SB_ERR_ARG, "search_radius: nhist must be 0 or at least 2");
    if (nhist < 0) return fail(c, SB_ERR_ARG, "search_radius: negative nhist");
    if (!radius && !summary && !(hist && nhist)) return fail(c, SB_ERR_ARG, "search_radius: no result asked for");
    const long long nxh = (long long)nx + 2LL * halo, nyh = (long long)ny + 2LL * halo;
    if (nxh > SB_RADIUS_MAX_W)
        return fail(c, SB_ERR_ARG, "search_radius: rows wider than " + std::to_string(SB_RADIUS_MAX_W) + " cells are not served");
    // the kernels count 64-cell segments of the frame in 32 bits
    if (nyh * ((nxh + 63) / 64) > SB_RADIUS_MAX_SEGS)
        return fail(c, SB_ERR_ARG, "search_radius: a frame of more than " + std::to_string(SB_RADIUS_MAX_SEGS) +
                                       " 64-cell segments (rows x words per row) is not served");
    return SB_OK;
}

template <typename T>
int search_radius_dev(sb_ctx *c, int nx, int ny, int halo, int bnd, int band, const T *mask, T maxdist, int *radius,
                      long long *summary, long long *hist, int nhist, void *stream) {
    int rc = check_search_radius<T>(c, nx, ny, halo, bnd, mask, radius, summary, hist, nhist);
    if (rc) return rc;
    if (!hist || nhist == 0) { hist = nullptr; nhist = 0; }
    const SbRadiusGeo g = sb_radius_geo(nx, ny, halo, bnd, band);
    if ((rc = ensure(c, c->rad_ws, sb_radius_ws_bytes(g)))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, sb_launch_search_radius<T>(mask, maxdist, g, c->rad_ws.p, radius, summary, hist, nhist, st));
    return SB_OK;
}

template <typename T>
int search_radius_host(sb_ctx *c, int nx, int ny, int halo, int bnd, int band, const T *mask, T maxdist, int *radius,
                       long long *summary, long long *hist, int nhist) {
    int rc = check_search_radius<T>(c, nx, ny, halo, bnd, mask, radius, summary, hist, nhist);
    if (rc) return rc;
    if (!hist || nhist == 0) { hist = nullptr; nhist = 0; }
    // (buffers of its own, not the Stager's: a staged diag call forgets sigma's statistics, this call forgets nothing)
    const size_t nm = (size_t)(nx + 2 * halo) * (ny + 2 * halo) * sizeof(T), n2 = (size_t)nx * ny;
    const size_t o_sum = (n2 * sizeof(int) + 7) & ~(size_t)7, o_hist = o_sum + 4 * sizeof(long long);
    if ((rc = ensure(c, c->rad_mask, nm))) return rc;
    if ((rc = ensure(c, c->rad_out, o_hist + (size_t)nhist * sizeof(long long)))) return rc;
    char *out = (char *)c->rad_out.p;
    HIPCHK(c, hipMemcpyAsync(c->rad_mask.p, mask, nm, hipMemcpyHostToDevice, c->stream));
    rc = search_radius_dev<T>(c, nx, ny, halo, bnd, band, (const T *)c->rad_mask.p, maxdist, radius ? (int *)out : nullptr,
                              (long long *)(out + o_sum), hist ? (long long *)(out + o_hist) : nullptr, nhist, nullptr);
    if (rc) return rc;
    if (radius) HIPCHK(c, hipMemcpyAsync(radius, out, n2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (summary) HIPCHK(c, hipMemcpyAsync(summary, out + o_sum, 4 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (hist) HIPCHK(c, hipMemcpyAsync(hist, out + o_hist, (size_t)nhist * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SB_OK;
}

inline int band_geo_of(int south, int north) {
    return GEO_BAND_EW | (south ? GEO_BAND_SOUTH : 0) | (north ? GEO_BAND_NORTH : 0);
}

// UM vn10.7 coast setup on the tdims_l layout (ref: UM/vn10.7/sea_breeze_diag.F90:328-601): fields with ghost cells are
// (nx + 2*hi) x (ny + 2*hj); the ghost cells of the outputs are left to the caller's swap_bounds
template <typename T>
int get_edges_um_dev(sb_ctx *c, int nx, int ny, int hi, int hj, const T *lf, const T *ci, T *coast, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !lf || !ci || !coast) return fail(c, SB_ERR_ARG, "bad get_edges_um arguments");
    if (hi < 1 || hj < 1) return fail(c, SB_ERR_ARG, "get_edges_um: halo_i and halo_j must be >= 1 (the Sobel reads the ghost ring)");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, sb_launch_edges_um<T>(lf, ci, coast, nx, ny, hi, hj, st));
    return SB_OK;
}

template <typename T>
int get_edges_um_host(sb_ctx *c, int nx, int ny, int hi, int hj, const T *lf, const T *ci, T *coast) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !lf || !ci || !coast) return fail(c, SB_ERR_ARG, "bad get_edges_um arguments");
    if (hi < 1 || hj < 1) return fail(c, SB_ERR_ARG, "get_edges_um: halo_i and halo_j must be >= 1 (the Sobel reads the ghost ring)");
    const size_t n = (size_t)(nx + 2 * hi) * (ny + 2 * hj);
    Stager s(c);
    T *dl = s.in(lf, n), *dc = s.in(ci, n), *dco = s.in(coast, n);     // (coast in as well: its ghost cells stay)
    if (s.rc) return s.rc;
    int rc = get_edges_um_dev<T>(c, nx, ny, hi, hj, dl, dc, dco, nullptr);
    if (rc) return rc;
    s.back(coast, dco, n);
    return s.finish();
}

template <typename T>
int check_dist_um(sb_ctx *c, int nx, int ny, int hi, int hj, const T *coast, const T *lf, const T *tlat, const T *tlon,
                  T *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !coast || !lf || !tlat || !tlon || !cdist) return fail(c, SB_ERR_ARG, "bad get_dist_um arguments");
    if (hi < 0 || hi > 31 || hj < 0 || hj > 31)
        return fail(c, SB_ERR_ARG, "get_dist_um: the window is +-halo_i x +-halo_j with 0 <= halo_i, halo_j <= 31");
    return SB_OK;
}

// sb_get_dist_um_win_*: the window stated apart from the layout (halo_i, halo_j >= 0 say where the interior lies)
template <typename T>
int check_dist_um_win(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const T *coast, const T *lf, const T *tlat,
                      const T *tlon, T *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || hi < 0 || hj < 0 || !coast || !lf || !tlat || !tlon || !cdist)
        return fail(c, SB_ERR_ARG, "bad get_dist_um_win arguments");
    if (wi < 0 || wi > SB_DIST_UM_MAX_WINDOW || wj < 0 || wj > SB_DIST_UM_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "get_dist_um_win: the window +-" + std::to_string(wi) + " x +-" + std::to_string(wj) +
                                       " needs 0 <= win_i, win_j <= SB_DIST_UM_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_UM_MAX_WINDOW) + " cells");
    return SB_OK;
}

template <typename T>
int get_dist_um_win_dev(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const T *coast, const T *lf,
                        const T *tlat, const T *tlon, T maxdist, T *cdist, void *stream) {
    int rc = check_dist_um_win<T>(c, nx, ny, hi, hj, wi, wj, coast, lf, tlat, tlon, cdist);
    if (rc) return rc;
    // the coordinates are device fields: nothing is derived from them on the host, nothing is kept between calls
    if ((rc = ensure(c, c->umbits, (size_t)ny * ((nx + 63) / 64) * sizeof(uint64_t)))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, sb_launch_dist_um_win<T>(coast, lf, tlat, tlon, cdist, nx, ny, hi, hj, wi, wj, maxdist, (uint64_t *)c->umbits.p, st));
    return SB_OK;
}

template <typename T>
int get_dist_um_win_host(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const T *coast, const T *lf,
                         const T *tlat, const T *tlon, T maxdist, T *cdist) {
    int rc = check_dist_um_win<T>(c, nx, ny, hi, hj, wi, wj, coast, lf, tlat, tlon, cdist);
    if (rc) return rc;
    const size_t n = (size_t)nx * ny, nl = (size_t)(nx + 2 * hi) * (ny + 2 * hj);
    Stager s(c);
    // (cdist in as well: its ghost cells stay; with cdist == coast both copies hold the same field)
    T *dco = s.in(coast, nl), *dl = s.in(lf, n), *dla = s.in(tlat, n), *dlo = s.in(tlon, n), *dcd = s.in((const T *)cdist, nl);
    if (s.rc) return s.rc;
    rc = get_dist_um_win_dev<T>(c, nx, ny, hi, hj, wi, wj, dco, dl, dla, dlo, maxdist, dcd, nullptr);
    if (rc) return rc;
    s.back(cdist, dcd, nl);
    return s.finish();
}

// sb_get_dist_um_*: the window is the layout's ghost width, at most 31 cells each way
template <typename T>
int get_dist_um_dev(sb_ctx *c, int nx, int ny, int hi, int hj, const T *coast, const T *lf, const T *tlat, const T *tlon,
                    T maxdist, T *cdist, void *stream) {
    int rc = check_dist_um<T>(c, nx, ny, hi, hj, coast, lf, tlat, tlon, cdist);
    if (rc) return rc;
    return get_dist_um_win_dev<T>(c, nx, ny, hi, hj, hi, hj, coast, lf, tlat, tlon, maxdist, cdist, stream);
}

template <typename T>
int get_dist_um_host(sb_ctx *c, int nx, int ny, int hi, int hj, const T *coast, const T *lf, const T *tlat,
                     const T *tlon, T maxdist, T *cdist) {
    int rc = check_dist_um<T>(c, nx, ny, hi, hj, coast, lf, tlat, tlon, cdist);
    if (rc) return rc;
    return get_dist_um_win_host<T>(c, nx, ny, hi, hj, hi, hj, coast, lf, tlat, tlon, maxdist, cdist);
}

}  // namespace

// ======================================================================================
// extern "C"
// ======================================================================================
extern "C" {

const char *sb_version(void) { return "seabreeze_hip 0.1.0 (gfx950)"; }

const char *sb_last_error(const sb_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

void sb_default_tunables(sb_tunables *t) {
    if (!t) return;
    t->target_plev_pa = 100 * 700.;
    t->thresh_wind = 11.;
    t->thresh_winddir = 90.;
    t->thresh_windch = 5.;
    t->thresh_thc = 0.75;
    t->target_time_s = 6. * 60 * 60;
    t->maxdist_km = 180.;
}

int sb_get_threads(int *nt) {
    if (!nt) return fail(nullptr, SB_ERR_ARG, "null pointer");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *nt = n;
    return SB_OK;
}

int sb_create(sb_ctx **out, int device) {
    if (!out) return fail(nullptr, SB_ERR_ARG, "null pointer");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1)
        return fail(nullptr, SB_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= n) return fail(nullptr, SB_ERR_ARG, "device index out of range");
    if ((e = hipSetDevice(device)) != hipSuccess) return hipfail(nullptr, e, "hipSetDevice");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hipfail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, SB_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    sb_ctx *c = new sb_ctx();
    c->device = device;
    c->ncu = c->ncu_dev = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return hipfail(nullptr, e, "hipStreamCreate");
    }
    bool ok = hipMalloc((void **)&c->partials, SB_STATS_MAX_BLOCKS * sizeof(Moments)) == hipSuccess &&
              hipMalloc((void **)&c->ticket, SB_TICKET_WORDS * sizeof(unsigned int)) == hipSuccess &&   // (see SB_TICKET_*)
              hipMalloc(&c->stats, 4 * sizeof(double)) == hipSuccess &&
              hipMalloc((void **)&c->counters, 2 * sizeof(int)) == hipSuccess &&
              hipMalloc((void **)&c->seg_count, SB_SEG_PARTS * sizeof(int)) == hipSuccess &&
              hipMemset(c->seg_count, 0, SB_SEG_PARTS * sizeof(int)) == hipSuccess &&
              hipMemset(c->ticket, 0, SB_TICKET_WORDS * sizeof(unsigned int)) == hipSuccess &&
              hipMemset(c->counters, 0, 2 * sizeof(int)) == hipSuccess &&
              hipDeviceSynchronize() == hipSuccess;   // the null-stream memsets have landed before any other stream runs
    if (!ok) {
        sb_destroy(c);
        return fail(nullptr, SB_ERR_ALLOC, "context allocation failed");
    }
    *out = c;
    return SB_OK;
}

int sb_destroy(sb_ctx *c) {
    if (!c) return SB_OK;
    (void)hipSetDevice(c->device);
    if (c->comm) (void)sb_comm_finalize(c);
    stream_release(c);
    if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_mom) (void)hipEventDestroy(c->ev_mom);
    if (c->band_mom.p) (void)hipFree(c->band_mom.p);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    for (DevBuf *b : {&c->t0, &c->bandbits, &c->clsbits, &c->tiles, &c->vecs, &c->nws, &c->nwd, &c->coastbits, &c->tile_list,
                      &c->seg_list, &c->stamps, &c->jobcopy, &c->plan, &c->umbits, &c->tabA, &c->tabL, &c->tabC, &c->tabS, &c->tabW,
                      &c->tabRep, &c->rad_ws, &c->rad_mask, &c->rad_out, &c->guardA, &c->guardB, &c->guardRep, &c->guardWs, &c->guardWd})
        if (b->p) (void)hipFree(b->p);
    for (DevBuf &b : c->stage)
        if (b.p) (void)hipFree(b.p);
    if (c->partials) (void)hipFree(c->partials);
    if (c->ticket) (void)hipFree(c->ticket);
    if (c->stats) (void)hipFree(c->stats);
    if (c->counters) (void)hipFree(c->counters);
    if (c->seg_count) (void)hipFree(c->seg_count);
    delete c;
    return SB_OK;
}

int sb_synchronize(sb_ctx *c) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SB_OK;
}


int sb_sigma_moments_f64_dev(sb_ctx *c, int nx, int ny, int halo, const double *sigma, double *m5, void *stream) {
    return sigma_moments_dev<double>(c, nx, ny, halo, sigma, m5, stream);
}
int sb_sigma_moments_f32_dev(sb_ctx *c, int nx, int ny, int halo, const float *sigma, double *m5, void *stream) {
    return sigma_moments_dev<float>(c, nx, ny, halo, sigma, m5, stream);
}

int sb_use_gathered_moments(sb_ctx *c, const double *gathered, int nparts) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (gathered && nparts < 1) return fail(c, SB_ERR_ARG, "nparts must be >= 1");
    static_assert(sizeof(Moments) == 5 * sizeof(double), "Moments is 5 doubles");
    c->gathered = (const Moments *)gathered;
    c->ngathered = gathered ? nparts : 0;
    return SB_OK;
}

int sb_profile_begin(sb_ctx *c, int max_calls) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (max_calls < 1 || max_calls > 100000) return fail(c, SB_ERR_ARG, "max_calls out of range");
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    c->prof_ev.assign((size_t)SB_PROF_EVENTS * max_calls, nullptr);
    c->prof_mask.assign((size_t)max_calls, 0u);
    for (hipEvent_t &e : c->prof_ev) HIPCHK(c, hipEventCreate(&e));
    c->prof_calls = 0;
    c->prof_max = max_calls;
    return SB_OK;
}

int sb_profile_end(sb_ctx *c, double avg_ms[SB_PROF_KERNELS], int *ncalls) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!avg_ms || !ncalls) return fail(c, SB_ERR_ARG, "null pointer");
    HIPCHK(c, hipDeviceSynchronize());
    // event pair k brackets kernel k (SB_PROF_*); a kernel a call did not launch has no interval
    double sum[SB_PROF_KERNELS] = {0, 0, 0, 0, 0};
    int cnt[SB_PROF_KERNELS] = {0, 0, 0, 0, 0};
    for (int i = 0; i < c->prof_calls; ++i)
        for (int k = 0; k < SB_PROF_KERNELS; ++k) {
            if (!((c->prof_mask[(size_t)i] >> k) & 1u)) continue;
            float ms = 0.f;
            const hipEvent_t *e = &c->prof_ev[(size_t)SB_PROF_EVENTS * i];
            HIPCHK(c, hipEventElapsedTime(&ms, e[2 * k], e[2 * k + 1]));
            sum[k] += ms;
            ++cnt[k];
        }
    *ncalls = c->prof_calls;
    for (int k = 0; k < SB_PROF_KERNELS; ++k) avg_ms[k] = cnt[k] ? sum[k] / cnt[k] : 0.0;
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    c->prof_ev.clear();
    c->prof_mask.clear();
    c->prof_calls = c->prof_max = 0;
    return SB_OK;
}

int sb_diag_stream_stats(sb_ctx *c, long *steps, double seconds[3]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!steps || !seconds) return fail(c, SB_ERR_ARG, "null pointer");
    *steps = c->ds.steps;
    seconds[0] = c->ds.host_copy_s; seconds[1] = c->ds.enqueue_s; seconds[2] = c->ds.wait_s;
    return SB_OK;
}

int sb_diag_stream_ice_report(sb_ctx *c, long long rep[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rep) return fail(c, SB_ERR_ARG, "null report");
    DiagStream &d = c->ds;
    if (!d.ice_ready) return fail(c, SB_ERR_ARG, "sb_diag_stream_ice_report without sb_diag_stream_coast");
    const long long tiles = (long long)d.nlats * sb_ice_tiles(d.nlons);
    rep[0] = d.ice_calls; rep[1] = 0; rep[2] = 0; rep[3] = tiles;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sb_ice_path(d.nlons, d.ice_k, d.ice_incremental) == SbIcePath::WHOLE) {
        // every call computes every tile and compares nothing
        rep[1] = -1;
        rep[2] = d.ice_calls ? tiles : 0;
        return SB_OK;
    }
    if (d.ice_calls == 0) return SB_OK;
    std::vector<unsigned char> host(d.ice_mark_bytes + 2 * sizeof(unsigned));
    HIPCHK(c, hipMemcpy(host.data(), d.icemarks.p, host.size(), hipMemcpyDeviceToHost));
    for (long long i = 0; i < tiles; ++i) rep[2] += host[(size_t)i] ? 1 : 0;
    unsigned words[2];
    std::memcpy(words, host.data() + d.ice_mark_bytes, sizeof(words));
    rep[1] = words[1];
    return SB_OK;
}

int sb_diag_stream_ice_time(sb_ctx *c, double *ms) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    DiagStream &d = c->ds;
    if (!ms || !d.ice_ready || d.ice_calls == 0) return fail(c, SB_ERR_ARG, "sb_diag_stream_ice_time without an ice call");
    HIPCHK(c, hipEventSynchronize(d.ev_ice_t[1]));
    float t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&t, d.ev_ice_t[0], d.ev_ice_t[1]));
    *ms = (double)t;
    return SB_OK;
}

int sb_set_search_radius_hint(sb_ctx *c, int radius) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (radius < 1) return fail(c, SB_ERR_ARG, "radius must be >= 1");
    c->radius_hint = radius;
    return SB_OK;
}

#ifdef SB_STAMPS
// diagnostic build only: the per-workgroup clock sums of the last k_thc3 launch
int sb_debug_plan(sb_ctx *c, void *host, long long bytes) {      // the strip kernel's stored plan (diagnostic build)
    if (!c || !host || !c->plan.p || bytes < 0 || (size_t)bytes > c->plan.cap) return SB_ERR_ARG;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(host, c->plan.p, (size_t)bytes, hipMemcpyDeviceToHost));
    return SB_OK;
}
int sb_debug_stamps(sb_ctx *c, long long *host, int nwg) {
    if (!c || !host || !c->stamps.p) return SB_ERR_ARG;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(host, c->stamps.p, (size_t)nwg * SB_NSTAMP * sizeof(long long), hipMemcpyDeviceToHost));
    return SB_OK;
}
#endif

int sb_last_counters(sb_ctx *c, long long counters[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!counters) return fail(c, SB_ERR_ARG, "null pointer");
    if (!c->have_last) return fail(c, SB_ERR_ARG, "no diag call yet");
    HIPCHK(c, hipDeviceSynchronize());
    const Geo &g = c->last_g;
    std::vector<uint64_t> bits((size_t)g.nyh * g.nw);
    std::vector<int> tiles((size_t)c->last_tiles + 2);
    int cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpy(bits.data(), c->bandbits.p, bits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(tiles.data(), c->last_flags, tiles.size() * sizeof(int), hipMemcpyDeviceToHost));
    cnt[0] = tiles[(size_t)c->last_tiles];
    cnt[1] = tiles[(size_t)c->last_tiles + 1];
    tiles.resize((size_t)c->last_tiles);
    long long nb = 0;
    for (uint64_t w : bits) nb += __builtin_popcountll(w);
    int mx = 0;
    for (int t : tiles) mx = t > mx ? t : mx;
    counters[0] = nb; counters[1] = cnt[0]; counters[2] = cnt[1]; counters[3] = mx;
    return SB_OK;
}

#define SB_DEFINE(T, SFX)                                                                                          \
    int sb_seabreeze_diag_##SFX(sb_ctx *c, T dt, int tn, int nx, int ny, int nz, int halo, int bnd, const T *p,     \
                                const T *u, const T *v, const T *theta, const T *mask, const T *z, const T *sigma,  \
                                T *ws, T *wd, T *thc, T *sb_con, const sb_tunables *tun) {                          \
        return seabreeze_diag_host<T>(c, dt, tn, nx, ny, nz, halo, bnd, p, u, v, theta, mask, z, sigma, ws, wd,     \
                                      thc, sb_con, tun);                                                            \
    }                                                                                                              \
    int sb_seabreeze_diag_##SFX##_dev(sb_ctx *c, T dt, int tn, int nx, int ny, int nz, int halo, int bnd,           \
                                      const T *p, const T *u, const T *v, const T *theta, const T *mask,            \
                                      const T *z, const T *sigma, T *ws, T *wd, T *thc, T *sb_con,                  \
                                      const sb_tunables *tun, void *stream) {                                       \
        return seabreeze_diag_dev<T>(c, dt, tn, nx, ny, nz, halo, bnd, p, u, v, theta, mask, z, sigma, ws, wd, thc, \
                                     sb_con, tun, stream);                                                          \
    }                                                                                                              \
    int sb_diag_##SFX(sb_ctx *c, int tn, const T *p, const T *z, const T *sd, const T *theta, const T *v,           \
                      const T *u, const T *cdist, T *ws, T *wd, T *thc, T a0, T a1, T a2, T a3, T a4, T a5, T a6,   \
                      T a7, int nps, int nlons, int nlats, T *output) {                                             \
        return diag_host<T>(c, tn, p, z, sd, theta, v, u, cdist, ws, wd, thc, a0, a1, a2, a3, a4, a5, a6, a7, nps,  \
                            nlons, nlats, output);                                                                  \
    }                                                                                                              \
    int sb_diag_##SFX##_dev(sb_ctx *c, int tn, const T *p, const T *z, const T *sd, const T *theta, const T *v,     \
                            const T *u, const T *cdist, T *ws, T *wd, T *thc, T a0, T a1, T a2, T a3, T a4, T a5,   \
                            T a6, T a7, int nps, int nlons, int nlats, T *output, void *stream) {                   \
        return diag_dev<T>(c, tn, p, z, sd, theta, v, u, cdist, ws, wd, thc, a0, a1, a2, a3, a4, a5, a6, a7, nps,   \
                           nlons, nlats, output, stream);                                                           \
    }                                                                                                              \
    int sb_sigmoid_##SFX(sb_ctx *c, int nx, int ny, const T *ary, T *sm) {                                          \
        return sigmoid_host<T>(c, nx, ny, ary, sm);                                                                 \
    }                                                                                                              \
    int sb_sigmoid_##SFX##_dev(sb_ctx *c, int nx, int ny, const T *ary, T *sm, void *stream) {                      \
        return sigmoid_dev<T>(c, nx, ny, ary, sm, stream);                                                          \
    }                                                                                                              \
    int sb_get_edges_##SFX(sb_ctx *c, int nx, int ny, const T *lsm, const T *ci, int rule, int bnd, T *coast) {     \
        return get_edges_host<T>(c, nx, ny, lsm, ci, rule, bnd, coast);                                             \
    }                                                                                                              \
    int sb_get_edges_##SFX##_dev(sb_ctx *c, int nx, int ny, const T *lsm, const T *ci, int rule, int bnd,           \
                                 T *coast, void *stream) {                                                          \
        return get_edges_dev<T>(c, nx, ny, lsm, ci, rule, bnd, coast, stream);                                      \
    }                                                                                                              \
    int sb_get_dist_##SFX(sb_ctx *c, int nx, int ny, const T *coast, const T *mask, const T *lon, const T *lat,     \
                          T maxdist, int kwin, T *cdist) {                                                          \
        return get_dist_host<T>(c, nx, ny, coast, mask, lon, lat, maxdist, kwin, cdist);                            \
    }                                                                                                              \
    int sb_get_dist_##SFX##_dev(sb_ctx *c, int nx, int ny, const T *coast, const T *mask, const T *lon,             \
                                const T *lat, T maxdist, int kwin, T *cdist, void *stream) {                        \
        return get_dist_dev<T>(c, nx, ny, coast, mask, lon, lat, maxdist, kwin, cdist, stream);                     \
    }                                                                                                              \
    int sb_band_get_edges_##SFX(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *lsm,            \
                                const T *ci, int rule, T *coast) {                                                  \
        return band_get_edges_host<T>(c, nx, ny, halo, south, north, lsm, ci, rule, coast);                         \
    }                                                                                                              \
    int sb_band_get_edges_##SFX##_dev(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *lsm,      \
                                      const T *ci, int rule, T *coast, void *stream) {                              \
        return band_get_edges_dev<T>(c, nx, ny, halo, south, north, lsm, ci, rule, coast, stream);                  \
    }                                                                                                              \
    int sb_band_get_dist_##SFX(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *coast,           \
                               const T *mask, const T *lon, const T *lat, T maxdist, int kwin, T *cdist) {          \
        return band_get_dist_host<T>(c, nx, ny, halo, south, north, coast, mask, lon, lat, maxdist, kwin, cdist);   \
    }                                                                                                              \
    int sb_band_get_dist_##SFX##_dev(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *coast,     \
                                     const T *mask, const T *lon, const T *lat, T maxdist, int kwin, T *cdist,      \
                                     void *stream) {                                                                \
        return band_get_dist_dev<T>(c, nx, ny, halo, south, north, coast, mask, lon, lat, maxdist, kwin, cdist,     \
                                    stream);                                                                        \
    }                                                                                                              \
    int sb_search_radius_##SFX(sb_ctx *c, int nx, int ny, int halo, int bnd, const T *mask, T maxdist, int *radius,\
                               long long *summary, long long *hist, int nhist) {                                   \
        return search_radius_host<T>(c, nx, ny, halo, bnd, 0, mask, maxdist, radius, summary, hist, nhist);        \
    }                                                                                                              \
    int sb_search_radius_##SFX##_dev(sb_ctx *c, int nx, int ny, int halo, int bnd, const T *mask, T maxdist,       \
                                     int *radius, long long *summary, long long *hist, int nhist, void *stream) {  \
        return search_radius_dev<T>(c, nx, ny, halo, bnd, 0, mask, maxdist, radius, summary, hist, nhist, stream); \
    }                                                                                                              \
    int sb_band_search_radius_##SFX(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *mask,      \
                                    T maxdist, int *radius, long long *summary, long long *hist, int nhist) {      \
        return search_radius_host<T>(c, nx, ny, halo, BND_HALO, band_geo_of(south, north), mask, maxdist, radius,  \
                                     summary, hist, nhist);                                                        \
    }                                                                                                              \
    int sb_band_search_radius_##SFX##_dev(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *mask,\
                                          T maxdist, int *radius, long long *summary, long long *hist, int nhist,  \
                                          void *stream) {                                                          \
        return search_radius_dev<T>(c, nx, ny, halo, BND_HALO, band_geo_of(south, north), mask, maxdist, radius,   \
                                    summary, hist, nhist, stream);                                                 \
    }                                                                                                              \
    int sb_get_edges_um_##SFX(sb_ctx *c, int nx, int ny, int hi, int hj, const T *lf, const T *ci, T *coast) {       \
        return get_edges_um_host<T>(c, nx, ny, hi, hj, lf, ci, coast);                                              \
    }                                                                                                              \
    int sb_get_edges_um_##SFX##_dev(sb_ctx *c, int nx, int ny, int hi, int hj, const T *lf, const T *ci, T *coast,  \
                                    void *stream) {                                                                 \
        return get_edges_um_dev<T>(c, nx, ny, hi, hj, lf, ci, coast, stream);                                       \
    }                                                                                                              \
    int sb_get_dist_um_##SFX(sb_ctx *c, int nx, int ny, int hi, int hj, const T *coast, const T *lf,                \
                             const T *tlat, const T *tlon, T maxdist, T *cdist) {                                   \
        return get_dist_um_host<T>(c, nx, ny, hi, hj, coast, lf, tlat, tlon, maxdist, cdist);                       \
    }                                                                                                              \
    int sb_get_dist_um_##SFX##_dev(sb_ctx *c, int nx, int ny, int hi, int hj, const T *coast, const T *lf,          \
                                   const T *tlat, const T *tlon, T maxdist, T *cdist, void *stream) {               \
        return get_dist_um_dev<T>(c, nx, ny, hi, hj, coast, lf, tlat, tlon, maxdist, cdist, stream);                \
    }                                                                                                              \
    int sb_get_dist_um_win_##SFX(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const T *coast,         \
                                 const T *lf, const T *tlat, const T *tlon, T maxdist, T *cdist) {                  \
        return get_dist_um_win_host<T>(c, nx, ny, hi, hj, wi, wj, coast, lf, tlat, tlon, maxdist, cdist);           \
    }                                                                                                              \
    int sb_get_dist_um_win_##SFX##_dev(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const T *coast,   \
                                       const T *lf, const T *tlat, const T *tlon, T maxdist, T *cdist,              \
                                       void *stream) {                                                              \
        return get_dist_um_win_dev<T>(c, nx, ny, hi, hj, wi, wj, coast, lf, tlat, tlon, maxdist, cdist, stream);    \
    }                                                                                                              \
    int sb_dist_window_##SFX(int nx, int ny, const T *lon, const T *lat, T maxdist, int *k) {                       \
        return dist_window<T>(nx, ny, lon, lat, maxdist, k);                                                        \
    }                                                                                                              \
    int sb_diag_stream_begin_##SFX(sb_ctx *c, int nlons, int nlats, const T *z, const T *sd, const T *cdist,         \
                                   const T *ws, const T *wd, const T *thc) {                                        \
        return stream_begin<T>(c, nlons, nlats, z, sd, cdist, ws, wd, thc);                                         \
    }                                                                                                              \
    int sb_diag_stream_step_##SFX(sb_ctx *c, int tn, const T *p, int nps, const T *theta, const T *v, const T *u,   \
                                  T a0, T a1, T a2, T a3, T a4, T a5, T a6, T a7, double *sb_con_prev,              \
                                  int *have_prev) {                                                                 \
        return stream_step<T>(c, tn, p, nps, theta, v, u, a0, a1, a2, a3, a4, a5, a6, a7, sb_con_prev, have_prev);  \
    }                                                                                                              \
    int sb_diag_stream_end_##SFX(sb_ctx *c, double *sb_con_last, T *output4, T *ws, T *wd, T *thc) {                \
        return stream_end<T>(c, sb_con_last, output4, ws, wd, thc);                                                 \
    }                                                                                                              \
    int sb_diag_stream_coast_##SFX(sb_ctx *c, const T *lsm, const T *lon, const T *lat, T maxdist, int incremental) { \
        return stream_coast<T>(c, lsm, lon, lat, maxdist, incremental);                                             \
    }                                                                                                              \
    int sb_diag_stream_ice_##SFX(sb_ctx *c, const T *ci) { return stream_ice<T>(c, ci); }                           \
    int sb_diag_stream_get_cdist_##SFX(sb_ctx *c, T *cdist) { return stream_get_cdist<T>(c, cdist); }               \
    int sb_seabreeze_diag_um_##SFX(sb_ctx *c, T dt, int tn, int nx, int ny, int nz, int hs, int hl, const T *p,     \
                                   const T *u, const T *v, T *theta, const T *z, const T *sigma, const T *mask,     \
                                   T *ws, T *wd, T *thc, T *sb_con, int flags, int *error) {                        \
        return seabreeze_diag_um_host<T>(c, dt, tn, nx, ny, nz, hs, hl, p, u, v, theta, z, sigma, mask, ws, wd, thc, \
                                         sb_con, flags, error);                                                     \
    }                                                                                                              \
    int sb_seabreeze_diag_um_##SFX##_dev(sb_ctx *c, T dt, int tn, int nx, int ny, int nz, int hs, int hl,           \
                                         const T *p, const T *u, const T *v, T *theta, const T *z, const T *sigma,  \
                                         const T *mask, T *ws, T *wd, T *thc, T *sb_con, int flags, int *error,     \
                                         void *stream) {                                                            \
        return seabreeze_diag_um_dev<T>(c, dt, tn, nx, ny, nz, hs, hl, p, u, v, theta, z, sigma, mask, ws, wd, thc, \
                                        sb_con, flags, error, stream);                                              \
    }

SB_DEFINE(double, f64)
SB_DEFINE(float, f32)

}  // extern "C"

// --------------------------------------------------------------------------------------
// Latitude-band communication over RCCL (xGMI).  librccl.so is opened on demand, so the
// library loads and every single-GPU entry point works without it.
// --------------------------------------------------------------------------------------
namespace {
struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId *);
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*GroupStart)();
    ncclResult_t (*GroupEnd)();
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
    const char *(*GetErrorString)(ncclResult_t);
    void *lib = nullptr;
} g_rccl;

int rccl_load(sb_ctx *c) {
    if (g_rccl.lib) return SB_OK;
    void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(c, SB_ERR_COMM, std::string("cannot load librccl.so: ") + dlerror());
#define SB_RCCL_SYM(field, name)                                                        \
    *(void **)(&g_rccl.field) = dlsym(lib, name);                                       \
    if (!g_rccl.field) return fail(c, SB_ERR_COMM, std::string("librccl.so lacks ") + name);
    SB_RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
    SB_RCCL_SYM(CommInitRank, "ncclCommInitRank")
    SB_RCCL_SYM(CommDestroy, "ncclCommDestroy")
    SB_RCCL_SYM(GroupStart, "ncclGroupStart")
    SB_RCCL_SYM(GroupEnd, "ncclGroupEnd")
    SB_RCCL_SYM(Send, "ncclSend")
    SB_RCCL_SYM(Recv, "ncclRecv")
    SB_RCCL_SYM(AllGather, "ncclAllGather")
    SB_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef SB_RCCL_SYM
    g_rccl.lib = lib;
    return SB_OK;
}

#define NCCLCHK(c, call)                                                                              \
    do {                                                                                              \
        ncclResult_t r__ = (call);                                                                    \
        if (r__ != ncclSuccess) return fail((c), SB_ERR_COMM, std::string(#call) + ": " + g_rccl.GetErrorString(r__)); \
    } while (0)

// the north-south rows of swap_bounds alone: my first / last `halo` interior rows out, the neighbours' into my ghost rows
template <typename T>
int exchange_rows_dev(sb_ctx *c, T *field, int nx, int ny, int halo, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!field || nx < 1 || ny < 1 || halo < 0) return fail(c, SB_ERR_ARG, "bad swap_bounds arguments");
    if (halo == 0 || c->nranks < 2) return SB_OK;
    if (ny < halo) return fail(c, SB_ERR_ARG, "band thinner than the halo");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t rowlen = (size_t)nx + 2 * halo, slab = rowlen * halo;
    const ncclDataType_t dt = sizeof(T) == 8 ? ncclDouble : ncclFloat;
    const bool south = c->rank == 0, north = c->rank == c->nranks - 1;
    ncclComm_t comm = (ncclComm_t)c->comm;
    NCCLCHK(c, g_rccl.GroupStart());
    if (!south) {
        NCCLCHK(c, g_rccl.Send(field + slab, slab, dt, c->rank - 1, comm, st));
        NCCLCHK(c, g_rccl.Recv(field, slab, dt, c->rank - 1, comm, st));
        c->rep_rccl += 2;
    }
    if (!north) {
        NCCLCHK(c, g_rccl.Send(field + rowlen * ny, slab, dt, c->rank + 1, comm, st));
        NCCLCHK(c, g_rccl.Recv(field + rowlen * (ny + halo), slab, dt, c->rank + 1, comm, st));
        c->rep_rccl += 2;
    }
    NCCLCHK(c, g_rccl.GroupEnd());
    c->rep_groups += 1;
    return SB_OK;
}

template <typename T>
int swap_bounds_dev(sb_ctx *c, T *field, int nx, int ny, int halo, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!field || nx < 1 || ny < 1 || halo < 0) return fail(c, SB_ERR_ARG, "bad swap_bounds arguments");
    if (halo == 0) return SB_OK;
    if (c->nranks > 1 && ny < halo) return fail(c, SB_ERR_ARG, "band thinner than the halo");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t rowlen = (size_t)nx + 2 * halo, slab = rowlen * halo;
    const ncclDataType_t dt = sizeof(T) == 8 ? ncclDouble : ncclFloat;
    const bool south = c->rank == 0, north = c->rank == c->nranks - 1;
    if (c->nranks > 1) {
        // one group: my first/last `halo` interior rows out, the neighbours' into my ghost rows
        ncclComm_t comm = (ncclComm_t)c->comm;
        NCCLCHK(c, g_rccl.GroupStart());
        if (!south) {
            NCCLCHK(c, g_rccl.Send(field + slab, slab, dt, c->rank - 1, comm, st));
            NCCLCHK(c, g_rccl.Recv(field, slab, dt, c->rank - 1, comm, st));
            c->rep_rccl += 2;
        }
        if (!north) {
            NCCLCHK(c, g_rccl.Send(field + rowlen * ny, slab, dt, c->rank + 1, comm, st));
            NCCLCHK(c, g_rccl.Recv(field + rowlen * (ny + halo), slab, dt, c->rank + 1, comm, st));
            c->rep_rccl += 2;
        }
        NCCLCHK(c, g_rccl.GroupEnd());
        c->rep_groups += 1;
    }
    HIPCHK(c, sb_launch_fill_ghosts<T>(field, nx, ny, halo, south ? 1 : 0, north ? 1 : 0, st));
    c->rep_launches += 1;
    return SB_OK;
}
}  // namespace

template <typename T>
static int fill_ghosts_dev(sb_ctx *c, T *field, int nx, int ny, int halo, int south, int north, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!field || nx < 1 || ny < 1 || halo < 0) return fail(c, SB_ERR_ARG, "bad fill_ghosts arguments");
    if (halo == 0) return SB_OK;
    HIPCHK(c, sb_launch_fill_ghosts<T>(field, nx, ny, halo, south ? 1 : 0, north ? 1 : 0, stream ? (hipStream_t)stream : c->stream));
    return SB_OK;
}

extern "C" {

int sb_comm_get_unique_id(unsigned char id[128]) {
    if (!id) return fail(nullptr, SB_ERR_ARG, "null pointer");
    int rc = rccl_load(nullptr);
    if (rc) return rc;
    ncclUniqueId u;
    ncclResult_t r = g_rccl.GetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, SB_ERR_COMM, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
    static_assert(sizeof(u.internal) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(id, u.internal, 128);
    return SB_OK;
}

int sb_comm_init(sb_ctx *c, const unsigned char id[128], int rank, int nranks) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, SB_ERR_ARG, "bad communicator arguments");
    if (c->comm) return fail(c, SB_ERR_ARG, "communicator already initialised");
    int rc = rccl_load(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, 128);
    ncclComm_t comm = nullptr;
    NCCLCHK(c, g_rccl.CommInitRank(&comm, nranks, u, rank));
    c->comm = comm;
    c->rank = rank;
    c->nranks = nranks;
    return SB_OK;
}

int sb_comm_finalize(sb_ctx *c) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (c->comm) {
        // every RCCL operation of a band step is enqueued on the communication stream: nothing may be in flight
        if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
        (void)hipStreamSynchronize(c->stream);
        NCCLCHK(c, g_rccl.CommDestroy((ncclComm_t)c->comm));
    }
    c->comm = nullptr;
    c->rank = 0;
    c->nranks = 1;
    return SB_OK;
}

int sb_band_seabreeze_diag_f64_dev(sb_ctx *c, double dt, int tn, int nx, int ny, int nz, int halo, const double *p,
                                   const double *u, const double *v, double *theta, const double *mask,
                                   const double *z, const double *sigma, double *ws, double *wd, double *thc,
                                   double *sb_con, const sb_tunables *tun, void *stream) {
    return band_diag_dev<double>(c, dt, tn, nx, ny, nz, halo, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con, tun,
                                 stream);
}
int sb_band_seabreeze_diag_f32_dev(sb_ctx *c, float dt, int tn, int nx, int ny, int nz, int halo, const float *p,
                                   const float *u, const float *v, float *theta, const float *mask, const float *z,
                                   const float *sigma, float *ws, float *wd, float *thc, float *sb_con,
                                   const sb_tunables *tun, void *stream) {
    return band_diag_dev<float>(c, dt, tn, nx, ny, nz, halo, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con, tun,
                                stream);
}

int sb_swap_bounds_f64_dev(sb_ctx *c, double *field, int nx, int ny, int halo, void *stream) {
    return swap_bounds_dev<double>(c, field, nx, ny, halo, stream);
}
int sb_swap_bounds_f32_dev(sb_ctx *c, float *field, int nx, int ny, int halo, void *stream) {
    return swap_bounds_dev<float>(c, field, nx, ny, halo, stream);
}

int sb_fill_ghosts_f64_dev(sb_ctx *c, double *field, int nx, int ny, int halo, int south, int north, void *stream) {
    return fill_ghosts_dev<double>(c, field, nx, ny, halo, south, north, stream);
}
int sb_fill_ghosts_f32_dev(sb_ctx *c, float *field, int nx, int ny, int halo, int south, int north, void *stream) {
    return fill_ghosts_dev<float>(c, field, nx, ny, halo, south, north, stream);
}

}  // extern "C"

// ---- host-pointer forms for host models that keep their fields in host memory (the Fortran modules) ----
namespace {
template <typename T>
int swap_bounds_host(sb_ctx *c, T *field, int nx, int ny, int halo) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!field || nx < 1 || ny < 1 || halo < 0) return fail(c, SB_ERR_ARG, "bad swap_bounds arguments");
    if (halo == 0) return SB_OK;
    const size_t n = (size_t)(nx + 2 * halo) * (ny + 2 * halo);
    Stager s(c);
    T *d = s.in(field, n);
    if (s.rc) return s.rc;
    int rc = swap_bounds_dev<T>(c, d, nx, ny, halo, nullptr);
    if (rc) return rc;
    s.back(field, d, n);
    return s.finish();
}

template <typename T>
int band_diag_host(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, const T *p, const T *u, const T *v,
                   T *theta, const T *mask, const T *z, const T *sigma, T *ws, T *wd, T *thc, T *sb_con,
                   const sb_tunables *tun) {
    int rc = check_dims<T>(c, nx, ny, nz, halo, SB_BND_HALO);
    if (rc) return rc;
    if (!p || !u || !v || !theta || !mask || !z || !sigma || !ws || !wd || !thc || !sb_con)
        return fail(c, SB_ERR_ARG, "null array pointer");
    const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, n2h = (size_t)(nx + 2 * halo) * (ny + 2 * halo);
    Stager s(c);
    T *dp = s.in(p, n3), *du = s.in(u, n3), *dv = s.in(v, n3);
    T *dth = s.in(theta, n2h), *dm = s.in(mask, n2h), *dz = s.in(z, n2h), *dsg = s.in(sigma, n2h);
    T *dws = s.in(ws, n2), *dwd = s.in(wd, n2), *dthc = s.in(thc, n2), *dsb = s.in(sb_con, n2);
    if (s.rc) return s.rc;
    rc = band_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, halo, dp, du, dv, dth, dm, dz, dsg, dws, dwd, dthc, dsb, tun, nullptr);
    if (rc) return rc;
    s.back(theta, dth, n2h);                      // its ghost cells were filled by the exchange
    s.back(ws, dws, n2); s.back(wd, dwd, n2); s.back(thc, dthc, n2); s.back(sb_con, dsb, n2);
    return s.finish();
}
}  // namespace

extern "C" {

int sb_swap_bounds_f64(sb_ctx *c, double *field, int nx, int ny, int halo) { return swap_bounds_host<double>(c, field, nx, ny, halo); }
int sb_swap_bounds_f32(sb_ctx *c, float *field, int nx, int ny, int halo) { return swap_bounds_host<float>(c, field, nx, ny, halo); }

int sb_band_seabreeze_diag_f64(sb_ctx *c, double dt, int tn, int nx, int ny, int nz, int halo, const double *p,
                               const double *u, const double *v, double *theta, const double *mask, const double *z,
                               const double *sigma, double *ws, double *wd, double *thc, double *sb_con,
                               const sb_tunables *tun) {
    return band_diag_host<double>(c, dt, tn, nx, ny, nz, halo, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con, tun);
}
int sb_band_seabreeze_diag_f32(sb_ctx *c, float dt, int tn, int nx, int ny, int nz, int halo, const float *p,
                               const float *u, const float *v, float *theta, const float *mask, const float *z,
                               const float *sigma, float *ws, float *wd, float *thc, float *sb_con,
                               const sb_tunables *tun) {
    return band_diag_host<float>(c, dt, tn, nx, ny, nz, halo, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con, tun);
}

int sb_comm_rank(sb_ctx *c, int *rank, int *nranks) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rank || !nranks) return fail(c, SB_ERR_ARG, "null pointer");
    *rank = c->rank;
    *nranks = c->comm ? c->nranks : 0;            // 0: no communicator
    return SB_OK;
}

// device memory for host models that keep fields resident between calls (Fortran: type(c_ptr))
int sb_device_malloc(sb_ctx *c, size_t nbytes, void **dptr) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!dptr) return fail(c, SB_ERR_ARG, "null pointer");
    *dptr = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipMalloc(dptr, nbytes ? nbytes : 8);
    if (e != hipSuccess) return fail(c, SB_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    return SB_OK;
}
int sb_device_free(sb_ctx *c, void *dptr) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (dptr) HIPCHK(c, hipFree(dptr));
    return SB_OK;
}
int sb_device_upload(sb_ctx *c, void *dst_dev, const void *src_host, size_t nbytes) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!dst_dev || !src_host) return fail(c, SB_ERR_ARG, "null pointer");
    HIPCHK(c, hipMemcpyAsync(dst_dev, src_host, nbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SB_OK;
}
int sb_device_download(sb_ctx *c, void *dst_host, const void *src_dev, size_t nbytes) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!dst_host || !src_dev) return fail(c, SB_ERR_ARG, "null pointer");
    HIPCHK(c, hipMemcpyAsync(dst_host, src_dev, nbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SB_OK;
}

int sb_allgather_moments_dev(sb_ctx *c, const double *mine5, double *gathered, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!mine5 || !gathered) return fail(c, SB_ERR_ARG, "null pointer");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (c->nranks == 1) {
        HIPCHK(c, hipMemcpyAsync(gathered, mine5, 5 * sizeof(double), hipMemcpyDeviceToDevice, st));
        c->rep_copies += 1;
        return SB_OK;
    }
    NCCLCHK(c, g_rccl.AllGather(mine5, gathered, 5, ncclDouble, (ncclComm_t)c->comm, st));
    c->rep_rccl += 1;
    return SB_OK;
}

int sb_set_fold(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->no_fold = on ? 0 : 1;
    return SB_OK;
}

int sb_set_workgroups(sb_ctx *c, int n) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (n < 0 || n > c->ncu_dev) return fail(c, SB_ERR_ARG, "sb_set_workgroups: 0 (the default) or 1 .. the device's compute units");
    HIPCHK(c, hipDeviceSynchronize());
    c->ncu = n == 0 ? c->ncu_dev : n;
    c->plan_bits = nullptr;                          // (the stored plan was made for another number of workgroups)
    return SB_OK;
}

int sb_set_band_order(sb_ctx *c, int contrast_first) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->band_late_wind = contrast_first ? 1 : 0;
    return SB_OK;
}

int sb_set_wind_pairs(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->no_wind_pairs = on ? 0 : 1;
    return SB_OK;
}

int sb_last_wind_pairs(sb_ctx *c, int *ran) {
    if (!c || !ran) return fail(c, SB_ERR_ARG, "sb_last_wind_pairs: null argument");
    *ran = c->last_wind_pairs;
    return SB_OK;
}

int sb_set_plan_cache(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->no_plan_cache = on ? 0 : 1;
    return SB_OK;
}

int sb_set_wide_strip(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->no_wide_strip = on ? 0 : 1;
    c->plan_bits = nullptr;
    return SB_OK;
}

int sb_set_static_sigma(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->static_sigma = on ? 1 : 0;
    c->stats_valid = false;
    return SB_OK;
}

int sb_set_table_contrast(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->sw.table = on != 0;
    return SB_OK;
}

int sb_set_table_contrast_bands(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->sw.table_bands = on != 0;
    return SB_OK;
}

int sb_set_table_contrast_f2py(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->sw.table_f2py = on != 0;
    return SB_OK;
}

int sb_set_table_window_cache(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->sw.table_cache = on != 0;
    sb_tab_cache_toggled(c->tabc);                   // (whatever W holds, the next call that uses it fills it)
    if (on) { c->tab_rep_reset = true; c->tab_calls = 0; }
    return SB_OK;
}

int sb_table_cache_report(sb_ctx *c, long long rep[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rep) return fail(c, SB_ERR_ARG, "null pointer");
    rep[0] = rep[1] = rep[2] = rep[3] = 0;
    if (c->tab_rep_reset || !c->tabRep.p) return SB_OK;      // (no call with the cache in effect since the switch was turned on)
    HIPCHK(c, hipDeviceSynchronize());
    std::vector<unsigned> d(SB_TAB_REP_HDR + (size_t)2 * c->tab_waves);
    HIPCHK(c, hipMemcpy(d.data(), c->tabRep.p, d.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (c->tab_last)
        for (int w = 0; w < c->tab_waves; ++w) { rep[0] += d[SB_TAB_REP_HDR + 2 * w]; rep[1] += d[SB_TAB_REP_HDR + 2 * w + 1]; }
    rep[2] = d[0]; rep[3] = c->tab_calls;
    return SB_OK;
}

int sb_set_nonfinite_guard(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->sw.guard = on != 0;
    c->guard_rep_reset = true; c->guard_calls = 0; c->guard_last = false;
    return SB_OK;
}

int sb_set_nonfinite_guard_bands(sb_ctx *c, int on) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    c->sw.guard_bands = on != 0;
    c->guard_rep_reset = true; c->guard_calls = 0; c->guard_last = false;
    // later band steps on the same planes get another Geo::band (the whole swap_bounds against neighbour rows only), which
    // the key of the strip kernel's stored plan does not hold: the next call plans afresh
    c->plan_bits = nullptr;
    return SB_OK;
}

int sb_guard_report(sb_ctx *c, long long rep[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rep) return fail(c, SB_ERR_ARG, "null pointer");
    rep[0] = rep[1] = rep[2] = rep[3] = 0;
    if (!c->guard_last || !c->guardRep.p) return SB_OK;      // (the last diag call was not one the guard served)
    HIPCHK(c, hipDeviceSynchronize());
    unsigned d[3];
    HIPCHK(c, hipMemcpy(d, c->guardRep.p, sizeof(d), hipMemcpyDeviceToHost));
    rep[0] = d[0]; rep[1] = d[1]; rep[2] = d[2]; rep[3] = c->guard_calls;
    return SB_OK;
}

int sb_last_step_report(sb_ctx *c, int report[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!report) return fail(c, SB_ERR_ARG, "null pointer");
    report[0] = c->rep_launches; report[1] = c->rep_rccl; report[2] = c->rep_groups; report[3] = c->rep_copies;
    return SB_OK;
}

}  // extern "C"

