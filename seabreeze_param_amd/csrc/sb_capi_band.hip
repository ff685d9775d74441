// sb_capi_band.hip -- latitude bands of a multi-GPU run: the RCCL loader and communicator, the exchange of ghost rows and
// the band step.
// Latitude-band communication over RCCL (xGMI).  librccl.so is opened on demand, so the
// library loads and every single-GPU entry point works without it.
#include "sb_ctx.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cstring>

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
    hipStream_t st = stream_of(c, stream);
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
    // the neighbours' rows (one rank: none; a band thinner than the halo is the exchange's to refuse), then the local part
    const int rc = c->nranks > 1 ? exchange_rows_dev<T>(c, field, nx, ny, halo, stream) : SB_OK;
    if (rc) return rc;
    const bool south = c->rank == 0, north = c->rank == c->nranks - 1;
    HIPCHK(c, sb_launch_fill_ghosts<T>(field, nx, ny, halo, south ? 1 : 0, north ? 1 : 0, stream_of(c, stream)));
    c->rep_launches += 1;
    return SB_OK;
}

// One model step of a latitude band: the communication (this band's sigma moments and their all-gather, theta's
// ghost rows) runs on the context's second stream while k_scan, k_prep and k_wind, which need neither, run
// on the caller's stream; the two join before k_thc3, which merges the gathered moments in its prologue.
// What the two diag calls underneath must know of the step -- the phase, the gathered set, Geo::band, where k_scan leaves
// the band's moments -- travels in their SbBandCall argument: nothing is parked on the context, nothing to put back.
template <typename T>
int band_diag_dev(sb_ctx *c, T timestep_s, int tn, int nx, int ny, int nz, int halo, const T *p, const T *u,
                  const T *v, T *theta, const T *mask, const T *z, const T *sigma, T *ws, T *wd, T *thc, T *sb_con,
                  const sb_tunables *tun, void *stream) {
    int rc = check_dims(c, nx, ny, nz, halo, SB_BND_HALO);
    if (rc) return rc;
    if (halo < 1) return fail(c, SB_ERR_ARG, "a band needs ghost cells (halo >= 1)");
    if (!sigma || !theta) return fail(c, SB_ERR_ARG, "null array pointer");
    hipStream_t st = stream_of(c, stream);
    if (!c->aux_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_mom, hipEventDisableTiming));
    }
    if ((rc = ensure(c, c->band_mom, (size_t)5 * (c->nranks + 1) * sizeof(double)))) return rc;
    double *mine = (double *)c->band_mom.p, *gath = mine + 5;
    // what the two phases below hand down instead of a plain call's values: the gathered set is this step's own (the reuse
    // key tells single-domain scalars from a band run's by it)
    SbBandCall ph1;
    ph1.phases = 1; ph1.gathered = (const Moments *)gath; ph1.ngathered = c->nranks;
    // static sigma (opt-in): the scalars of the first step stand, no moments, no all-gather, no merge
    const bool reuse = reuse_stats<T>(c, ph1, sigma, nx, ny, halo);
    c->rep_launches = c->rep_rccl = c->rep_groups = c->rep_copies = 0;
    // fork: everything that talks to the other ranks goes to the second stream: the exchange of theta's ghost rows at
    // once, the all-gather of the sigma moments as soon as k_scan has published this band's (every rank issues the two
    // RCCL operations in this order), while k_scan and k_wind run on the caller's stream.
    hipError_t he = hipEventRecord(c->ev_fork, st);
    if (he == hipSuccess) he = hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0);
    if (he != hipSuccess) return hipfail(c, he, "band step fork");
    // The ghost rows of theta first: they depend on nothing this step computes.  On a strip kernel only the rows that
    // come from a NEIGHBOUR travel: the east-west ghost columns (the periodic wrap of the row itself) and the ghost rows
    // beyond a pole (the edge row again) follow from theta's interior, and the strip kernels take them from there by index
    // arithmetic (Geo::band) -- no fill kernel on the communication stream, three launches per band step (round 3: four,
    // and the fill, running behind the caller's stream's kernels rather than beside them, held the join up).  The tile
    // kernel (double precision, radii beyond 16) reads every ghost cell as filled: the whole swap_bounds for it.
    // The table contrast and the guard for band steps read the whole frame too, and their kernels see plain SB_BND_HALO
    // geometry (Geo::band == 0) -- the one fill launch is what either switch costs a strip kernel here.  One predicate,
    // beside the one that decides which switches serve the two phases below: sb_band_folds_frame, sb_diag_plan.hpp.
    const bool folds = sb_band_folds_frame(c->sw, sb_plan_contrast(plan_input<T>(c, ph1, nx, ny)), nx);
    ph1.geo = folds ? (GEO_BAND_EW | (c->rank == 0 ? GEO_BAND_SOUTH : 0) | (c->rank == c->nranks - 1 ? GEO_BAND_NORTH : 0)) : 0;
    rc = folds ? exchange_rows_dev<T>(c, theta, nx, ny, halo, (void *)c->aux_stream)
               : swap_bounds_dev<T>(c, theta, nx, ny, halo, (void *)c->aux_stream);
    // Phase 1 on the caller's stream: k_scan -- whose last workgroup merges this band's sigma moments and leaves them for
    // the all-gather (one rank: in the gathered set itself) -- then k_wind.  (The moments used to be formed by a kernel
    // of their own on the communication stream; with the caller's stream filling every CU that kernel ran behind
    // k_scan and k_wind, not beside them, and held the join up by 17 us: profiles/r03_band_step_cost.log.)
    ph1.moments_out = reuse ? nullptr : (Moments *)(c->nranks == 1 ? gath : mine);
    if (!rc) rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, halo, SB_BND_HALO, p, u, v, theta, mask, z, sigma, ws, wd,
                                        thc, sb_con, tun, (void *)st, ph1);
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
    SbBandCall ph2 = ph1;
    ph2.phases = 2; ph2.moments_out = nullptr;
    if (!rc) rc = seabreeze_diag_dev<T>(c, timestep_s, tn, nx, ny, nz, halo, SB_BND_HALO, p, u, v, theta, mask, z, sigma,
                                        ws, wd, thc, sb_con, tun, (void *)st, ph2);
    return rc;
}

template <typename T>
int fill_ghosts_dev(sb_ctx *c, T *field, int nx, int ny, int halo, int south, int north, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!field || nx < 1 || ny < 1 || halo < 0) return fail(c, SB_ERR_ARG, "bad fill_ghosts arguments");
    if (halo == 0) return SB_OK;
    HIPCHK(c, sb_launch_fill_ghosts<T>(field, nx, ny, halo, south ? 1 : 0, north ? 1 : 0, stream_of(c, stream)));
    return SB_OK;
}

// ---- host-pointer forms for host models that keep their fields in host memory (the Fortran modules) ----
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
    int rc = check_diag(c, nx, ny, nz, halo, SB_BND_HALO, {p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con});
    if (rc) return rc;
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

int sb_comm_rank(sb_ctx *c, int *rank, int *nranks) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rank || !nranks) return fail(c, SB_ERR_ARG, "null pointer");
    *rank = c->rank;
    *nranks = c->comm ? c->nranks : 0;            // 0: no communicator
    return SB_OK;
}

int sb_allgather_moments_dev(sb_ctx *c, const double *mine5, double *gathered, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!mine5 || !gathered) return fail(c, SB_ERR_ARG, "null pointer");
    hipStream_t st = stream_of(c, stream);
    if (c->nranks == 1) {
        HIPCHK(c, hipMemcpyAsync(gathered, mine5, 5 * sizeof(double), hipMemcpyDeviceToDevice, st));
        c->rep_copies += 1;
        return SB_OK;
    }
    NCCLCHK(c, g_rccl.AllGather(mine5, gathered, 5, ncclDouble, (ncclComm_t)c->comm, st));
    c->rep_rccl += 1;
    return SB_OK;
}

#define SB_DEFINE(T, SFX)                                                                                          \
    int sb_band_seabreeze_diag_##SFX(sb_ctx *c, T dt, int tn, int nx, int ny, int nz, int halo, const T *p,        \
                                     const T *u, const T *v, T *theta, const T *mask, const T *z, const T *sigma,  \
                                     T *ws, T *wd, T *thc, T *sb_con, const sb_tunables *tun) {                    \
        return band_diag_host<T>(c, dt, tn, nx, ny, nz, halo, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con, \
                                 tun);                                                                             \
    }                                                                                                              \
    int sb_band_seabreeze_diag_##SFX##_dev(sb_ctx *c, T dt, int tn, int nx, int ny, int nz, int halo, const T *p,  \
                                           const T *u, const T *v, T *theta, const T *mask, const T *z,            \
                                           const T *sigma, T *ws, T *wd, T *thc, T *sb_con,                        \
                                           const sb_tunables *tun, void *stream) {                                 \
        return band_diag_dev<T>(c, dt, tn, nx, ny, nz, halo, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con,  \
                                tun, stream);                                                                      \
    }                                                                                                              \
    int sb_swap_bounds_##SFX(sb_ctx *c, T *field, int nx, int ny, int halo) {                                      \
        return swap_bounds_host<T>(c, field, nx, ny, halo);                                                        \
    }                                                                                                              \
    int sb_swap_bounds_##SFX##_dev(sb_ctx *c, T *field, int nx, int ny, int halo, void *stream) {                  \
        return swap_bounds_dev<T>(c, field, nx, ny, halo, stream);                                                 \
    }                                                                                                              \
    int sb_fill_ghosts_##SFX##_dev(sb_ctx *c, T *field, int nx, int ny, int halo, int south, int north,            \
                                   void *stream) {                                                                 \
        return fill_ghosts_dev<T>(c, field, nx, ny, halo, south, north, stream);                                   \
    }

SB_DEFINE(double, f64)
SB_DEFINE(float, f32)
#undef SB_DEFINE

}  // extern "C"
