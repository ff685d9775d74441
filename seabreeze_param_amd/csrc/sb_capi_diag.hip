// sb_capi_diag.hip -- the diag calls of the C ABI: the workspace planner of one call (run_diag), the generic, UM and
// f2py flavours in their `_dev` and host-pointer forms, sigmoid and the sigma moments.
#include "sb_ctx.hpp"

#include <cstring>

// the launch plan's input (sb_diag_plan.hpp) as far as the context and the domain give it: all the contrast kernel's choice needs
template <typename T>
SbPlanIn plan_input(const sb_ctx *c, const SbBandCall &call, int nx, int rows) {
    SbPlanIn in{};
    in.esize = (int)sizeof(T); in.nx = nx; in.rows = rows; in.halo = sb_pick_halo(c->radius_hint);
    in.no_wide_strip = c->no_wide_strip != 0; in.no_fold = c->no_fold != 0; in.no_plan_cache = c->no_plan_cache != 0;
    in.band_late_wind = c->band_late_wind != 0; in.gathered = call.gathered != nullptr;
    in.shapes = sb_contrast_shapes(nx, rows);
    return in;
}

// sigma's statistics of an earlier complete call still stand (opt-in, same array, same shape)
template <typename T>
bool reuse_stats(const sb_ctx *c, const SbBandCall &call, const T *sigma, int nx, int ny, int halo) {
    return c->static_sigma && c->host_depth == 0 && c->stats_valid && c->stats_sigma == (const void *)sigma && c->stats_dims[0] == nx &&
           c->stats_dims[1] == ny && c->stats_dims[2] == halo && c->stats_dims[3] == (int)sizeof(T) &&
           c->stats_ngathered == (call.gathered ? call.ngathered : 0);   // single-domain scalars are not a band run's
}

namespace {

// Prepare workspace + job; enqueue the kernels of one diag call, or of one phase of a band step (call.phases).
template <typename T>
int run_diag(sb_ctx *c, DiagJob<T> &job, hipStream_t st, const SbBandCall &call) {
    const Geo &g = job.g;
    const int phases = call.phases;
    const size_t ncell = (size_t)g.nxh * g.nyh;
    const size_t nbits = (size_t)g.nyh * g.nw * sizeof(uint64_t);
    int rc;
    c->tab_last = false;                // (sb_table_cache_report: until this call has been enqueued with the cache in effect)
    c->guard_last = false;              // (sb_guard_report likewise)
    if ((rc = ensure(c, c->bandbits, nbits))) return rc;
    if ((rc = ensure(c, c->clsbits, nbits))) return rc;
    SbPlanIn in = plan_input<T>(c, call, g.nx, g.rows);
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
    lc.gathered = call.gathered; lc.ngathered = call.ngathered; lc.ncu = c->ncu;
    lc.wind_pairs = c->no_wind_pairs ? 0 : 1; lc.wind_pairs_ran = &c->last_wind_pairs;
    lc.moments_out = (phases == 1) ? call.moments_out : nullptr;   // (a band step: k_scan publishes this band's moments)
    lc.moments_event = (phases == 1 && c->nranks > 1) ? c->ev_mom : nullptr;   // (one rank: nobody waits for them)
    lc.stats_ticket = (int *)c->ticket + 1;
    // every decision about the kernels of this call: the plan's (the job's mode fields are the executor's to set)
    in.t0_fly = job.t0_fly != 0; in.moments_out = lc.moments_out != nullptr;
    in.reuse_stats = reuse_stats<T>(c, call, job.sigma, g.nx, g.ny, g.h);
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
        c->stats_ngathered = call.gathered ? call.ngathered : 0;
    }
    c->last_flags = flags_now;
    c->flag_parity = 1 - c->flag_parity;
    c->last_g = g;
    c->last_tiles = ntile;
    c->have_last = true;
    return SB_OK;
}

}  // namespace

template <typename T>
int seabreeze_diag_dev(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, int bnd, const T *p,
                       const T *u, const T *v, const T *theta, const T *mask, const T *z, const T *sigma, T *ws,
                       T *wd, T *thc, T *sb_con, const sb_tunables *tun, void *stream, const SbBandCall &call,
                       int mask_halo, int level_rule) {
    int rc = check_diag(c, nx, ny, nz, halo, bnd, {p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con});
    if (rc) return rc;
    sb_tunables d;
    sb_default_tunables(&d);
    if (tun) d = *tun;
    DiagJob<T> job{};
    job.g = make_geo<T>(nx, ny, halo, bnd, ny);
    if (bnd == SB_BND_HALO) job.g.band = call.geo;    // (a band step whose strip kernel reads no east-west / polar ghost cells of theta)
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
    hipStream_t st = stream_of(c, stream);
    return run_diag<T>(c, job, st, call);
}

template <typename T>
int diag_dev(sb_ctx *c, int tn, const T *p, const T *z, const T *std_, const T *theta, const T *v, const T *u,
             const T *cdist, T *ws, T *wd, T *thc, T target_plev, T thresh_wind, T thresh_winddir, T thresh_windch,
             T thresh_thc, T target_time, T maxdist, T timestep, int nps, int nlons, int nlats, T *output,
             void *stream) {
    int rc = check_diag(c, nlons, nlats, nps, 0, SB_BND_WRAPPER, {p, z, std_, theta, v, u, cdist, ws, wd, thc, output});
    if (rc) return rc;
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
    hipStream_t st = stream_of(c, stream);
    if (job.g.rows < 1) return SB_OK;                             // nlats == 1: the reference loop is empty
    return run_diag<T>(c, job, st, plain_call(c));
}

namespace {

template <typename T>
int seabreeze_diag_host(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, int bnd, const T *p,
                        const T *u, const T *v, const T *theta, const T *mask, const T *z, const T *sigma, T *ws,
                        T *wd, T *thc, T *sb_con, const sb_tunables *tun) {
    int rc = check_diag(c, nx, ny, nz, halo, bnd, {p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con});
    if (rc) return rc;
    const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, n2h = (size_t)(nx + 2 * halo) * (ny + 2 * halo);
    Stager s(c);
    T *dp = s.in(p, n3), *du = s.in(u, n3), *dv = s.in(v, n3);
    T *dth = s.in(theta, n2h), *dm = s.in(mask, n2h), *dz = s.in(z, n2h), *dsg = s.in(sigma, n2h);
    T *dws = s.in(ws, n2), *dwd = s.in(wd, n2), *dthc = s.in(thc, n2), *dsb = s.in(sb_con, n2);
    if (s.rc) return s.rc;
    rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, halo, bnd, dp, du, dv, dth, dm, dz, dsg, dws, dwd,
                               dthc, dsb, tun, nullptr, plain_call(c));
    if (rc) return rc;
    s.back(ws, dws, n2); s.back(wd, dwd, n2); s.back(thc, dthc, n2); s.back(sb_con, dsb, n2);
    return s.finish();
}

// the UM forms' own checks; *error = 1 (and SB_OK): the reference's error return, nothing to compute (ref: UM :198-202)
int check_diag_um(sb_ctx *c, int nx, int ny, int nz, int hs, int hl, int flags, int *error,
                  std::initializer_list<const void *> arrays) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!error) return fail(c, SB_ERR_ARG, "null error pointer");
    *error = 0;
    if (ny < 1 || nz < 1 || nx < 1) { *error = 1; return SB_OK; }
    if (hs < 0 || hl < hs) return fail(c, SB_ERR_ARG, "UM layout: need 0 <= halo_s <= halo_l");
    if (flags & ~(SB_UM_THETA_TO_T0 | SB_UM_LEVEL_WALK)) return fail(c, SB_ERR_ARG, "unknown UM flag");
    return check_diag(c, nx, ny, nz, hs, hs > 0 ? SB_BND_HALO : SB_BND_GLOBAL, arrays);
}

// UM vn10.7 field layout (ref: UM/vn10.7/sea_breeze_diag.F90:55-117): p, u, v, sb_con on pdims and windspeed,
// winddir, thc on tdims (no ghost cells); theta, z, sigma on tdims_s (ghost width hs); mask on tdims_l (hl >= hs).
template <typename T>
int seabreeze_diag_um_dev(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int hs, int hl, const T *p,
                          const T *u, const T *v, T *theta, const T *z, const T *sigma, const T *mask, T *ws, T *wd,
                          T *thc, T *sb_con, int flags, int *error, void *stream) {
    int rc = check_diag_um(c, nx, ny, nz, hs, hl, flags, error, {p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con});
    if (rc || *error) return rc;
    const int bnd = hs > 0 ? SB_BND_HALO : SB_BND_GLOBAL;
    rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, hs, bnd, p, u, v, theta, mask, z, sigma, ws, wd, thc,
                                   sb_con, nullptr, stream, plain_call(c), hl, (flags & SB_UM_LEVEL_WALK) ? 1 : 0);
    if (rc) return rc;
    if (flags & SB_UM_THETA_TO_T0) {
        hipStream_t st = stream_of(c, stream);
        HIPCHK(c, sb_launch_theta_to_t0<T>(theta, z, sigma, (size_t)(nx + 2 * hs) * (ny + 2 * hs), (const T *)c->stats, st));
    }
    return SB_OK;
}

template <typename T>
int seabreeze_diag_um_host(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int hs, int hl, const T *p,
                           const T *u, const T *v, T *theta, const T *z, const T *sigma, const T *mask, T *ws, T *wd,
                           T *thc, T *sb_con, int flags, int *error) {
    int rc = check_diag_um(c, nx, ny, nz, hs, hl, flags, error, {p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con});
    if (rc || *error) return rc;
    const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, ns = (size_t)(nx + 2 * hs) * (ny + 2 * hs),
                 nl = (size_t)(nx + 2 * hl) * (ny + 2 * hl);
    Stager s(c);
    T *dp = s.in(p, n3), *du = s.in(u, n3), *dv = s.in(v, n3);
    T *dth = s.in(theta, ns), *dz = s.in(z, ns), *dsg = s.in(sigma, ns), *dm = s.in(mask, nl);
    T *dws = s.in(ws, n2), *dwd = s.in(wd, n2), *dthc = s.in(thc, n2), *dsb = s.in(sb_con, n2);
    if (s.rc) return s.rc;
    rc = seabreeze_diag_um_dev<T>(c, timestep_s, tn, nx, ny, nz, hs, hl, dp, du, dv, dth, dz, dsg, dm, dws, dwd, dthc,
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
    int rc = check_diag(c, nlons, nlats, nps, 0, SB_BND_WRAPPER, {p, z, std_, theta, v, u, cdist, ws, wd, thc, output});
    if (rc) return rc;
    const size_t n2 = (size_t)nlons * nlats;
    // p is one column for the whole grid (ref: seabreeze_diag_python.f90:228), so the level is known
    // before anything is uploaded: pick it here exactly as the kernel would (pick_level) and send only that
    // u/v plane -- 2 planes instead of 2*nps over PCIe, same result.
    const int lev = pick_level<T>(p, nps, target_plev);
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

int check_sigmoid(sb_ctx *c, int nx, int ny, const void *ary, const void *sm) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !ary || !sm) return fail(c, SB_ERR_ARG, "bad sigmoid arguments");
    return SB_OK;
}

template <typename T>
int sigmoid_dev(sb_ctx *c, int nx, int ny, const T *ary, T *sm, void *stream) {
    int rc = check_sigmoid(c, nx, ny, ary, sm);
    if (rc) return rc;
    hipStream_t st = stream_of(c, stream);
    c->stats_valid = false;                 // the shared scalars now belong to `ary`, not to a diag call's sigma
    HIPCHK(c, sb_launch_stats<T>(ary, nx, ny, nx, 0, c->partials, (T *)c->stats, nullptr, (int *)c->ticket + 1, st));
    HIPCHK(c, sb_launch_sigmoid_apply<T>(ary, sm, (size_t)nx * ny, (const T *)c->stats, st));
    return SB_OK;
}

template <typename T>
int sigmoid_host(sb_ctx *c, int nx, int ny, const T *ary, T *sm) {
    int rc = check_sigmoid(c, nx, ny, ary, sm);
    if (rc) return rc;
    const size_t n = (size_t)nx * ny;
    Stager s(c);
    T *da = s.in(ary, n), *ds = s.out<T>(n);
    if (s.rc) return s.rc;
    rc = sigmoid_dev<T>(c, nx, ny, da, ds, nullptr);
    if (rc) return rc;
    s.back(sm, ds, n);
    return s.finish();
}

template <typename T>
int sigma_moments_dev(sb_ctx *c, int nx, int ny, int halo, const T *sigma, double *moments5, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || halo < 0 || !sigma || !moments5) return fail(c, SB_ERR_ARG, "bad sigma_moments arguments");
    hipStream_t st = stream_of(c, stream);
    const int nxh = nx + 2 * halo;
    HIPCHK(c, sb_launch_stats<T>(sigma, nx, ny, nxh, (size_t)halo * nxh + halo, c->partials, (T *)c->stats,
                                 (Moments *)moments5, (int *)c->ticket + 1, st));
    return SB_OK;
}

}  // namespace

// what the other units call (sb_ctx.hpp): emitted here for both precisions
#define SB_INST(T)                                                                                                      \
    template int seabreeze_diag_dev<T>(sb_ctx *, T, int, int, int, int, int, int, const T *, const T *, const T *,      \
                                       const T *, const T *, const T *, const T *, T *, T *, T *, T *,                  \
                                       const sb_tunables *, void *, const SbBandCall &, int, int);                      \
    template int diag_dev<T>(sb_ctx *, int, const T *, const T *, const T *, const T *, const T *, const T *,           \
                             const T *, T *, T *, T *, T, T, T, T, T, T, T, T, int, int, int, T *, void *);             \
    template SbPlanIn plan_input<T>(const sb_ctx *, const SbBandCall &, int, int);                                      \
    template bool reuse_stats<T>(const sb_ctx *, const SbBandCall &, const T *, int, int, int);
SB_INST(double)
SB_INST(float)
#undef SB_INST

extern "C" {

int sb_use_gathered_moments(sb_ctx *c, const double *gathered, int nparts) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (gathered && nparts < 1) return fail(c, SB_ERR_ARG, "nparts must be >= 1");
    static_assert(sizeof(Moments) == 5 * sizeof(double), "Moments is 5 doubles");
    c->gathered = (const Moments *)gathered;
    c->ngathered = gathered ? nparts : 0;
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
                                     sb_con, tun, stream, plain_call(c));                                          \
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
    int sb_sigma_moments_##SFX##_dev(sb_ctx *c, int nx, int ny, int halo, const T *sigma, double *m5, void *stream) { \
        return sigma_moments_dev<T>(c, nx, ny, halo, sigma, m5, stream);                                            \
    }                                                                                                              \
    int sb_sigmoid_##SFX(sb_ctx *c, int nx, int ny, const T *ary, T *sm) {                                          \
        return sigmoid_host<T>(c, nx, ny, ary, sm);                                                                 \
    }                                                                                                              \
    int sb_sigmoid_##SFX##_dev(sb_ctx *c, int nx, int ny, const T *ary, T *sm, void *stream) {                      \
        return sigmoid_dev<T>(c, nx, ny, ary, sm, stream);                                                          \
    }                                                                                                              \
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
#undef SB_DEFINE

}  // extern "C"
