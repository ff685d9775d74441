// sb_capi.hip -- the C ABI of libseabreeze_hip.so (see include/seabreeze_hip.h).
//
// Host-pointer entry points stage through device buffers owned by the context and
// synchronise before returning; `_dev` entry points only enqueue.  There is no CPU
// fallback anywhere in this file: no device => SB_ERR_NO_DEVICE.
#include "sb_ctx.hpp"

#include <cstring>

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
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->partials) (void)hipFree(c->partials);
    if (c->ticket) (void)hipFree(c->ticket);
    if (c->stats) (void)hipFree(c->stats);
    if (c->counters) (void)hipFree(c->counters);
    if (c->seg_count) (void)hipFree(c->seg_count);
    delete c;                               // (every DevBuf of the context frees itself here, behind the streams)
    return SB_OK;
}

int sb_synchronize(sb_ctx *c) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    HIPCHK(c, hipStreamSynchronize(c->stream));
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
