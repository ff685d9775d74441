// sb_capi_stream.hip -- the streaming form of the f2py-flavour diag (sb_diag_stream_*): its host thread pool, the steps,
// and the coast that moves with the sea ice.
#include "sb_ctx.hpp"
#include "sb_ice_plan.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

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

// ---- streaming diag (f2py flavour): SURVEY.md 8(f) rank 1 ---------------------------------------------------
// The reference's Python driver calls diag once per timestep with the same z, std, cdist and threads windspeed,
// winddir, thc through its return values (ref: python_wrapper/seabreezediag/__init__.py:222-245).  Here those six
// planes stay on the device between sb_diag_stream_begin and sb_diag_stream_end; a step uploads theta and the one
// u, v plane its 1-D p selects through pinned, double-buffered staging (asynchronous copies), and brings back only
// the sb_con plane -- of the PREVIOUS step, so that the host copies of step i+1 overlap the device work of step i.
void stream_release(sb_ctx *c) {
    DiagStream &d = c->ds;
    for (DevBuf *b : {&d.z, &d.sd, &d.cdist, &d.ws, &d.wd, &d.thc, &d.p1, &d.theta, &d.v, &d.u, &d.out, &d.lsm, &d.ice})
        if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    ice_free(d.it);
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

namespace {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <typename T>
int stream_begin(sb_ctx *c, int nlons, int nlats, const T *z, const T *sd, const T *cdist, const T *ws, const T *wd,
                 const T *thc) {
    int rc = check_dims(c, nlons, nlats, 1, 0, SB_BND_WRAPPER);
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
    const int lev = pick_level<T>(p, nps, target_plev);          // as diag_host: the level is known on the host
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
    if ((rc = ensure(c, d.lsm, b2)) || (rc = ensure(c, d.ice, b2)) ||
        (rc = ice_open(c, d.it, bitbytes, sb_ice_marks(nx, ny), sb_ice_path(nx, k, incremental) == SbIcePath::WHOLE ? b2 : 0,
                       incremental, c->stream)))
        return rc;
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
    HIPCHK(c, hipStreamSynchronize(c->stream));                                // (lsm is the caller's pageable array)
    d.ice_lonlat.resize(((size_t)nx + ny) * sizeof(T));
    std::memcpy(d.ice_lonlat.data(), lon, (size_t)nx * sizeof(T));
    std::memcpy(d.ice_lonlat.data() + (size_t)nx * sizeof(T), lat, (size_t)ny * sizeof(T));
    d.ice_k = k; d.ice_maxdist = (double)maxdist;
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
    const int slot = (int)(d.it.calls & 1);
    double t0 = now_s();
    if (d.it.calls >= 2) HIPCHK(c, hipEventSynchronize(d.ev_ice[slot]));      // the slot's upload of two ice calls ago
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
    if (sb_ice_path(nx, k, d.it.incremental) == SbIcePath::WHOLE) {
        HIPCHK(c, sb_launch_edges<T>((const T *)d.lsm.p, (const T *)d.ice.p, (T *)d.it.coast.p, nx, ny, 0, BND_WRAPPER, st));
        HIPCHK(c, sb_launch_dist<T>((const T *)d.it.coast.p, (const T *)d.lsm.p, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx,
                                    (T *)d.cdist.p, nx, ny, k, maxdist, (uint64_t *)d.it.bits.p, cuts, st));
    } else {
        IceCall ic;
        if ((rc = ice_begin(c, d.it, st, ic))) return rc;
        HIPCHK(c, sb_launch_edge_bits_delta<T>((const T *)d.lsm.p, (const T *)d.ice.p, (uint64_t *)d.it.bits.p, ic.marks, ic.rep, nx,
                                               ny, k, ic.first, st));
        HIPCHK(c, sb_launch_dist_dirty<T>((const T *)d.lsm.p, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx, (T *)d.cdist.p, nx, ny, k,
                                          maxdist, (const uint64_t *)d.it.bits.p, cuts, ic.marks, st));
    }
    HIPCHK(c, hipEventRecord(d.ev_ice_t[1], st));
    c->radius_hint = k + 1;
    d.it.calls++;
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

}  // namespace

extern "C" {

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
    return ice_report(c, d.it, sb_ice_marks(d.nlons, d.nlats), sb_ice_path(d.nlons, d.ice_k, d.it.incremental) == SbIcePath::WHOLE,
                      false, rep);
}

int sb_diag_stream_ice_time(sb_ctx *c, double *ms) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    DiagStream &d = c->ds;
    if (!ms || !d.ice_ready || d.it.calls == 0) return fail(c, SB_ERR_ARG, "sb_diag_stream_ice_time without an ice call");
    HIPCHK(c, hipEventSynchronize(d.ev_ice_t[1]));
    float t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&t, d.ev_ice_t[0], d.ev_ice_t[1]));
    *ms = (double)t;
    return SB_OK;
}

#define SB_DEFINE(T, SFX)                                                                                          \
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
    int sb_diag_stream_get_cdist_##SFX(sb_ctx *c, T *cdist) { return stream_get_cdist<T>(c, cdist); }

SB_DEFINE(double, f64)
SB_DEFINE(float, f32)
#undef SB_DEFINE

}  // extern "C"
