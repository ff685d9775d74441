// sb_capi_coast.hip -- the coast setup of the C ABI: get_edges and get_dist on the whole grid, on one latitude band and in
// the UM layout and on one tile of its 2-D decomposition, a band's, a UM-layout and a UM tile's coast that move with the sea
// ice, and search_radius.
#include "sb_ctx.hpp"
#include "sb_ice_plan.hpp"

#include <cmath>
#include <cstring>

namespace {

int check_edges(sb_ctx *c, int nx, int ny, const void *lsm, const void *ci, int rule, int bnd, const void *coast) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !lsm || !ci || !coast) return fail(c, SB_ERR_ARG, "bad get_edges arguments");
    if (rule < 0 || rule > 1) return fail(c, SB_ERR_ARG, "unknown mask rule");
    if (bnd != SB_BND_WRAPPER && bnd != SB_BND_GLOBAL) return fail(c, SB_ERR_ARG, "get_edges: boundary must be WRAPPER or GLOBAL");
    return SB_OK;
}

template <typename T>
int get_edges_dev(sb_ctx *c, int nx, int ny, const T *lsm, const T *ci, int rule, int bnd, T *coast, void *stream) {
    int rc = check_edges(c, nx, ny, lsm, ci, rule, bnd, coast);
    if (rc) return rc;
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, sb_launch_edges<T>(lsm, ci, coast, nx, ny, rule, bnd, st));
    return SB_OK;
}

template <typename T>
int get_edges_host(sb_ctx *c, int nx, int ny, const T *lsm, const T *ci, int rule, int bnd, T *coast) {
    int rc = check_edges(c, nx, ny, lsm, ci, rule, bnd, coast);
    if (rc) return rc;
    const size_t n = (size_t)nx * ny;
    Stager s(c);
    T *dl = s.in(lsm, n), *dc = s.in(ci, n), *dco = s.out<T>(n);
    if (s.rc) return s.rc;
    rc = get_edges_dev<T>(c, nx, ny, dl, dc, rule, bnd, dco, nullptr);
    if (rc) return rc;
    s.back(coast, dco, n);
    return s.finish();
}

}  // namespace

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

template int dist_window<double>(int, int, const double *, const double *, double, int *);
template int dist_window<float>(int, int, const float *, const float *, float, int *);
template int dist_tables<double>(sb_ctx *, int, int, const double *, const double *, hipStream_t);
template int dist_tables<float>(sb_ctx *, int, int, const float *, const float *, hipStream_t);

namespace {

int check_dist(sb_ctx *c, int nx, int ny, const void *coast, const void *mask, const void *lon, const void *lat, const void *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !coast || !mask || !lon || !lat || !cdist)
        return fail(c, SB_ERR_ARG, "bad get_dist arguments");
    return SB_OK;
}

template <typename T>
int get_dist_dev(sb_ctx *c, int nx, int ny, const T *coast, const T *mask, const T *lon, const T *lat, T maxdist,
                 int kwin, T *cdist, void *stream) {
    int rc = check_dist(c, nx, ny, coast, mask, lon, lat, cdist);
    if (rc) return rc;
    int k = kwin;
    if (kwin < 0 && (rc = dist_window<T>(nx, ny, lon, lat, maxdist, &k))) { c->err = g_err; return rc; }
    if (k > SB_DIST_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "get_dist: window half-width " + std::to_string(k) + " exceeds SB_DIST_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_MAX_WINDOW) + " cells");
    hipStream_t st = stream_of(c, stream);
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
    int rc = check_dist(c, nx, ny, coast, mask, lon, lat, cdist);
    if (rc) return rc;
    const size_t n = (size_t)nx * ny;
    Stager s(c);
    T *dco = s.in(coast, n), *dm = s.in(mask, n), *dcd = s.out<T>(n);
    if (s.rc) return s.rc;
    rc = get_dist_dev<T>(c, nx, ny, dco, dm, lon, lat, maxdist, kwin, dcd, nullptr);
    if (rc) return rc;
    s.back(cdist, dcd, n);
    return s.finish();
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
    hipStream_t st = stream_of(c, stream);
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
    hipStream_t st = stream_of(c, stream);
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

// ---- a band whose coast moves with the sea ice (sb_band_coast_open_*, sb_band_ice_*_dev) ----
// setup_mask's chain -- ghost rows of lsm and ci, band edges, ghost rows of coast, band distance -- per timestep costs four
// exchanges and the whole band again.  Here the band keeps its coast as a bit plane over its SOURCE rows and forms the
// bits of the ghost source rows itself from k+1 ghost rows of lsm and ci (integer logic on land flags: exactly what the
// neighbour would have sent), so an ice call is a clear of the marks, k_edge_bits_delta and the band's distance
// kernel over the marked tiles (sb_ice_plan.hpp says which path, and what a changed word reaches); nothing is exchanged
// here, nothing waits.  k_scan of the next band step compares the band planes with what the step before left, so the
// stored plans and windows follow the rewritten cdist by themselves.
template <typename T>
int band_coast_open(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *lon, const T *lat, T maxdist, int kwin,
                    int rule, int incremental) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (c->bc.open) return fail(c, SB_ERR_ARG, "sb_band_coast_open: already open (sb_band_coast_close first)");
    if (nx < 1 || ny < 1 || halo < 0 || !lon || !lat) return fail(c, SB_ERR_ARG, "bad band_coast_open arguments");
    if (rule < 0 || rule > 1) return fail(c, SB_ERR_ARG, "unknown mask rule");
    if (kwin < 0)
        return fail(c, SB_ERR_ARG, "band_coast_open: kwin must be given (the derived half-width needs the global latitudes: "
                                   "sb_dist_window_* on those)");
    if (kwin > SB_DIST_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "band_coast_open: window half-width " + std::to_string(kwin) + " exceeds SB_DIST_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_MAX_WINDOW) + " cells");
    const SbBandIcePlan pl = sb_band_ice_plan(nx, ny, halo, south != 0, north != 0, kwin, incremental);
    if (!pl.ok)
        return fail(c, SB_ERR_ARG, "band_coast_open: a cut side needs kwin + 1 <= halo (the Sobel of the kwin-th ghost row reads "
                                   "the next one), got kwin = " + std::to_string(kwin) + ", halo = " + std::to_string(halo));
    BandCoast &b = c->bc;
    const int nys = pl.rows.nys, ld = nx + 2 * halo;
    int rc;
    if ((rc = ice_open(c, b.it, (size_t)nys * pl.nw * sizeof(uint64_t), pl.marks,
                       pl.path == SbIcePath::WHOLE ? (size_t)nys * ld * sizeof(T) : 0, incremental, c->stream)))
        return rc;
    b.lonlat.resize(((size_t)nx + nys) * sizeof(T));
    std::memcpy(b.lonlat.data(), lon, (size_t)nx * sizeof(T));
    std::memcpy(b.lonlat.data() + (size_t)nx * sizeof(T), lat + pl.rows.f0, (size_t)nys * sizeof(T));   // (nothing beyond a pole)
    // the tables of these coordinates now, so that the first ice call finds them and only enqueues
    if ((rc = dist_tables<T>(c, nx, nys, (const T *)b.lonlat.data(), (const T *)b.lonlat.data() + nx, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->dist_upload_stream == c->stream) c->dist_upload_stream = nullptr;   // (they have landed)
    b.esz = (int)sizeof(T);
    b.nx = nx; b.ny = ny; b.halo = halo; b.south = south ? 1 : 0; b.north = north ? 1 : 0;
    b.k = kwin; b.rule = rule; b.maxdist = (double)maxdist;
    b.open = true;
    return SB_OK;
}

template <typename T>
int band_ice_dev(sb_ctx *c, const T *lsm, const T *ci, T *cdist, void *stream) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    BandCoast &b = c->bc;
    if (!b.open) return fail(c, SB_ERR_ARG, "sb_band_ice without sb_band_coast_open");
    if (b.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_band_ice: the band coast was opened in the other precision");
    if (!lsm || !ci || !cdist) return fail(c, SB_ERR_ARG, "null array pointer");
    const int nx = b.nx, k = b.k, ld = nx + 2 * b.halo;
    const SbBandIcePlan pl = sb_band_ice_plan(nx, b.ny, b.halo, b.south != 0, b.north != 0, k, b.it.incremental);
    const SbBandRows br = pl.rows;
    hipStream_t st = stream_of(c, stream);
    // (the tables are keyed on the coordinates' content: another get_dist call on this context may have replaced them)
    const T *lon = (const T *)b.lonlat.data(), *lat = lon + nx;
    int rc;
    if ((rc = dist_tables<T>(c, nx, br.nys, lon, lat, st))) return rc;
    const T *dphi = (const T *)c->vecs.p, *dlam = dphi + br.nys;
    const int cuts = sb_dist_cuts(c->dist_traits, k);
    const T maxdist = (T)b.maxdist;
    const size_t o = (size_t)br.f0 * ld + b.halo;                // (column 0, source row 0) of a frame
    if (pl.path == SbIcePath::WHOLE) {
        HIPCHK(c, sb_launch_edges_band_src<T>(lsm, ci, (T *)b.it.coast.p, nx, b.halo, br, b.south, b.north, b.rule, k, st));
        HIPCHK(c, sb_launch_dist_band<T>((const T *)b.it.coast.p, lsm + o, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx, cdist + o, nx,
                                         br.nys, br.r0, br.r1, ld, k, maxdist, (uint64_t *)b.it.bits.p, cuts, st));
    } else {
        IceCall ic;
        if ((rc = ice_begin(c, b.it, st, ic))) return rc;
        HIPCHK(c, sb_launch_edge_bits_delta_band<T>(lsm, ci, (uint64_t *)b.it.bits.p, ic.marks, ic.rep, nx, b.halo, br, b.south,
                                                    b.north, b.rule, k, ic.first, st));
        HIPCHK(c, sb_launch_dist_band_dirty<T>(lsm + o, dphi, dlam, dlam + nx, dlam + 2 * (size_t)nx, cdist + o, nx, br.nys, br.r0,
                                               br.r1, ld, k, maxdist, (const uint64_t *)b.it.bits.p, cuts, ic.marks, st));
    }
    c->radius_hint = k + 1;
    b.it.calls++;
    return SB_OK;
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
    hipStream_t st = stream_of(c, stream);
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
int check_edges_um(sb_ctx *c, int nx, int ny, int hi, int hj, const void *lf, const void *ci, const void *coast) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (nx < 1 || ny < 1 || !lf || !ci || !coast) return fail(c, SB_ERR_ARG, "bad get_edges_um arguments");
    if (hi < 1 || hj < 1) return fail(c, SB_ERR_ARG, "get_edges_um: halo_i and halo_j must be >= 1 (the Sobel reads the ghost ring)");
    return SB_OK;
}

template <typename T>
int get_edges_um_dev(sb_ctx *c, int nx, int ny, int hi, int hj, const T *lf, const T *ci, T *coast, void *stream) {
    int rc = check_edges_um(c, nx, ny, hi, hj, lf, ci, coast);
    if (rc) return rc;
    hipStream_t st = stream_of(c, stream);
    HIPCHK(c, sb_launch_edges_um<T>(lf, ci, coast, nx, ny, hi, hj, st));
    return SB_OK;
}

template <typename T>
int get_edges_um_host(sb_ctx *c, int nx, int ny, int hi, int hj, const T *lf, const T *ci, T *coast) {
    int rc = check_edges_um(c, nx, ny, hi, hj, lf, ci, coast);
    if (rc) return rc;
    const size_t n = (size_t)(nx + 2 * hi) * (ny + 2 * hj);
    Stager s(c);
    T *dl = s.in(lf, n), *dc = s.in(ci, n), *dco = s.in(coast, n);     // (coast in as well: its ghost cells stay)
    if (s.rc) return s.rc;
    rc = get_edges_um_dev<T>(c, nx, ny, hi, hj, dl, dc, dco, nullptr);
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
    hipStream_t st = stream_of(c, stream);
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

// ---- one tile of a 2-D domain decomposition (sb_tile_get_edges_um_*, sb_tile_get_dist_um_*) ----
// Every field is the rank's frame, (nx + 2hi) x (ny + 2hj) with the interior at (hi, hj), ghost cells filled by the caller's
// swap_bounds; a set bit of `sides` says that side is the domain's edge.  `reach` is ext (edges: what is written beyond the
// interior on a cut side; the Sobel reads one cell more) or the window (distance: what is read), `ring` that one cell more.
int check_tile_um(sb_ctx *c, const char *what, int nx, int ny, int hi, int hj, int ri, int rj, int sides, int ring) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    const std::string w(what);
    if (nx < 1 || ny < 1 || hi < 0 || hj < 0) return fail(c, SB_ERR_ARG, "bad " + w + " arguments");
    if (sides < 0 || sides > 15) return fail(c, SB_ERR_ARG, w + ": sides must be a sum of SB_TILE_* bits, 0 .. 15");
    if (ri < 0 || rj < 0 || ri > SB_DIST_UM_MAX_WINDOW || rj > SB_DIST_UM_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, w + ": ext / win must be 0 .. SB_DIST_UM_MAX_WINDOW = " + std::to_string(SB_DIST_UM_MAX_WINDOW));
    if ((double)(nx + 2.0 * hi) * (double)(ny + 2.0 * hj) > 2.0e9) return fail(c, SB_ERR_ARG, "grid too large");
    const bool cut_i = !(sides & SB_TILE_WEST) || !(sides & SB_TILE_EAST), cut_j = !(sides & SB_TILE_SOUTH) || !(sides & SB_TILE_NORTH);
    const int need_i = cut_i ? ri + ring : ring, need_j = cut_j ? rj + ring : ring;
    if (hi < need_i || hj < need_j)
        return fail(c, SB_ERR_ARG, w + ": the halo " + std::to_string(hi) + " x " + std::to_string(hj) + " is smaller than " +
                                       std::to_string(need_i) + " x " + std::to_string(need_j) +
                                       (ring ? " (ext + 1 on a cut side, 1 on an edge side: the Sobel reads the ring beyond what it writes)"
                                             : " (the window on a cut side: its ghost cells are sources)"));
    return SB_OK;
}

inline bool overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

template <typename T>
int check_tile_edges_um(sb_ctx *c, int nx, int ny, int hi, int hj, int ei, int ej, int sides, const T *lf, const T *ci, const T *coast) {
    int rc = check_tile_um(c, "tile_get_edges_um", nx, ny, hi, hj, ei, ej, sides, 1);
    if (rc) return rc;
    if (!lf || !ci || !coast) return fail(c, SB_ERR_ARG, "tile_get_edges_um: null array pointer");
    const size_t nb = (size_t)(nx + 2 * hi) * (ny + 2 * hj) * sizeof(T);
    if (overlap(coast, lf, nb) || overlap(coast, ci, nb))
        return fail(c, SB_ERR_ARG, "tile_get_edges_um: coast_l overlaps an input (the Sobel of a cell reads its neighbours' flags)");
    return SB_OK;
}

template <typename T>
int tile_get_edges_um_dev(sb_ctx *c, int nx, int ny, int hi, int hj, int ei, int ej, int sides, const T *lf, const T *ci, T *coast,
                          void *stream) {
    int rc = check_tile_edges_um<T>(c, nx, ny, hi, hj, ei, ej, sides, lf, ci, coast);
    if (rc) return rc;
    HIPCHK(c, sb_launch_edges_um_tile<T>(lf, ci, coast, nx, ny, hi, hj, ei, ej, sides, stream_of(c, stream)));
    return SB_OK;
}

template <typename T>
int tile_get_edges_um_host(sb_ctx *c, int nx, int ny, int hi, int hj, int ei, int ej, int sides, const T *lf, const T *ci, T *coast) {
    int rc = check_tile_edges_um<T>(c, nx, ny, hi, hj, ei, ej, sides, lf, ci, coast);
    if (rc) return rc;
    const size_t n = (size_t)(nx + 2 * hi) * (ny + 2 * hj);
    Stager s(c);
    T *dl = s.in(lf, n), *dc = s.in(ci, n), *dco = s.in((const T *)coast, n);   // (coast in as well: the cells not written stay)
    if (s.rc) return s.rc;
    rc = tile_get_edges_um_dev<T>(c, nx, ny, hi, hj, ei, ej, sides, dl, dc, dco, nullptr);
    if (rc) return rc;
    s.back(coast, dco, n);
    return s.finish();
}

template <typename T>
int check_tile_dist_um(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, int sides, const T *coast, const T *lf,
                       const T *tlat, const T *tlon, const T *cdist) {
    int rc = check_tile_um(c, "tile_get_dist_um", nx, ny, hi, hj, wi, wj, sides, 0);
    if (rc) return rc;
    if (!coast || !lf || !tlat || !tlon || !cdist) return fail(c, SB_ERR_ARG, "tile_get_dist_um: null array pointer");
    return SB_OK;
}

template <typename T>
int tile_get_dist_um_dev(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, int sides, const T *coast, const T *lf,
                         const T *tlat, const T *tlon, T maxdist, T *cdist, void *stream) {
    int rc = check_tile_dist_um<T>(c, nx, ny, hi, hj, wi, wj, sides, coast, lf, tlat, tlon, cdist);
    if (rc) return rc;
    // the coordinates are device frames: nothing is derived from them on the host, nothing is kept between calls
    if ((rc = ensure(c, c->umbits, sb_dist_um_tile_bits_bytes(nx, ny, wi, wj, sides)))) return rc;
    HIPCHK(c, sb_launch_dist_um_tile<T>(coast, lf, tlat, tlon, cdist, nx, ny, hi, hj, wi, wj, sides, maxdist, (uint64_t *)c->umbits.p,
                                        stream_of(c, stream)));
    return SB_OK;
}

template <typename T>
int tile_get_dist_um_host(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, int sides, const T *coast, const T *lf,
                          const T *tlat, const T *tlon, T maxdist, T *cdist) {
    int rc = check_tile_dist_um<T>(c, nx, ny, hi, hj, wi, wj, sides, coast, lf, tlat, tlon, cdist);
    if (rc) return rc;
    const size_t n = (size_t)(nx + 2 * hi) * (ny + 2 * hj);
    Stager s(c);
    // (cdist in as well: its ghost cells stay; with cdist == coast both copies hold the same field)
    T *dco = s.in(coast, n), *dl = s.in(lf, n), *dla = s.in(tlat, n), *dlo = s.in(tlon, n), *dcd = s.in((const T *)cdist, n);
    if (s.rc) return s.rc;
    rc = tile_get_dist_um_dev<T>(c, nx, ny, hi, hj, wi, wj, sides, dco, dl, dla, dlo, maxdist, dcd, nullptr);
    if (rc) return rc;
    s.back(cdist, dcd, n);
    return s.finish();
}

// ---- a UM-layout coast that moves with the sea ice (sb_um_coast_open_*, sb_um_ice_*) ----
// The UM rebuilds its mask from icefrac inside the timestep routine (ref: UM/vn10.7/sea_breeze_diag.F90:384-445), so
// get_edges_um + get_dist_um_win per timestep cost the whole interior again.  Here the context keeps the interior's coast
// as a bit plane of its own and the coordinates on the device; an ice call is one clear of [marks | changed-word counter],
// k_edge_bits_delta and the UM distance kernel over the marked workgroups (sb_ice_plan.hpp says which path, and what a
// changed word reaches).  Nothing waits.  k_scan of the next sb_seabreeze_diag_um_* call finds the changed band planes by
// content.
template <typename T>
int um_coast_open(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const T *tlat, const T *tlon, T maxdist,
                  int incremental) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    UmCoast &u = c->um;
    if (u.open) return fail(c, SB_ERR_ARG, "sb_um_coast_open: already open (sb_um_coast_close first)");
    if (nx < 1 || ny < 1 || !tlat || !tlon) return fail(c, SB_ERR_ARG, "bad um_coast_open arguments");
    if (hi < 1 || hj < 1) return fail(c, SB_ERR_ARG, "um_coast_open: halo_i and halo_j must be >= 1 (the Sobel reads the ghost ring)");
    if (wi < 0 || wi > SB_DIST_UM_MAX_WINDOW || wj < 0 || wj > SB_DIST_UM_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "um_coast_open: the window +-" + std::to_string(wi) + " x +-" + std::to_string(wj) +
                                       " needs 0 <= win_i, win_j <= SB_DIST_UM_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_UM_MAX_WINDOW) + " cells");
    if ((double)(nx + 2.0 * hi) * (double)(ny + 2.0 * hj) > 2.0e9) return fail(c, SB_ERR_ARG, "grid too large");
    const SbUmIcePlan pl = sb_um_ice_plan(nx, ny, hi, hj, wi, wj, incremental);
    if (!pl.ok) return fail(c, SB_ERR_ARG, "bad um_coast_open arguments");
    const size_t n = (size_t)nx * ny;
    const bool whole = pl.path == SbIcePath::WHOLE;
    int rc;
    if ((rc = ensure(c, u.coords, 2 * n * sizeof(T))) || (whole && (rc = ensure(c, u.lf, n * sizeof(T)))) ||
        (rc = ice_open(c, u.it, (size_t)ny * pl.nw * sizeof(uint64_t), pl.marks,
                       whole ? (size_t)(nx + 2 * hi) * (ny + 2 * hj) * sizeof(T) : 0, incremental, c->stream)))
        return rc;
    HIPCHK(c, hipMemcpyAsync(u.coords.p, tlat, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((T *)u.coords.p + n, tlon, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                // (the caller's coordinates may go now)
    u.esz = (int)sizeof(T);
    u.nx = nx; u.ny = ny; u.hi = hi; u.hj = hj; u.wi = wi; u.wj = wj;
    u.maxdist = (double)maxdist;
    u.open = true;
    return SB_OK;
}

template <typename T>
int check_um_ice(sb_ctx *c, const T *lf, const T *ci, const T *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    const UmCoast &u = c->um;
    if (!u.open) return fail(c, SB_ERR_ARG, "sb_um_ice without sb_um_coast_open");
    if (u.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_um_ice: the UM coast was opened in the other precision");
    if (!lf || !ci || !cdist) return fail(c, SB_ERR_ARG, "null array pointer");
    return SB_OK;
}

template <typename T>
int um_ice_dev(sb_ctx *c, const T *lf, const T *ci, T *cdist, void *stream) {
    int rc = check_um_ice<T>(c, lf, ci, cdist);
    if (rc) return rc;
    UmCoast &u = c->um;
    const int nx = u.nx, ny = u.ny, hi = u.hi, hj = u.hj, NX = nx + 2 * hi;
    const T *tlat = (const T *)u.coords.p, *tlon = tlat + (size_t)nx * ny;
    const T maxdist = (T)u.maxdist;
    hipStream_t st = stream_of(c, stream);
    if (sb_um_ice_path(u.it.incremental) == SbIcePath::WHOLE) {
        // today's chain on the context's own planes; sb_launch_dist_um_win reads an interior landfrac: a copy of the frame's
        HIPCHK(c, hipMemcpy2DAsync(u.lf.p, (size_t)nx * sizeof(T), lf + (size_t)hj * NX + hi, (size_t)NX * sizeof(T),
                                   (size_t)nx * sizeof(T), (size_t)ny, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, sb_launch_edges_um<T>(lf, ci, (T *)u.it.coast.p, nx, ny, hi, hj, st));
        HIPCHK(c, sb_launch_dist_um_win<T>((const T *)u.it.coast.p, (const T *)u.lf.p, tlat, tlon, cdist, nx, ny, hi, hj, u.wi, u.wj,
                                           maxdist, (uint64_t *)u.it.bits.p, st));
    } else {
        IceCall ic;
        if ((rc = ice_begin(c, u.it, st, ic))) return rc;
        HIPCHK(c, sb_launch_edge_bits_delta_um<T>(lf, ci, (uint64_t *)u.it.bits.p, ic.marks, ic.rep, nx, ny, hi, hj, u.wi, u.wj,
                                                  ic.first, st));
        HIPCHK(c, sb_launch_dist_um_dirty<T>(lf, tlat, tlon, cdist, nx, ny, hi, hj, u.wi, u.wj, maxdist,
                                             (const uint64_t *)u.it.bits.p, ic.marks, st));
    }
    u.it.calls++;
    return SB_OK;
}

template <typename T>
int um_ice_host(sb_ctx *c, const T *lf, const T *ci, T *cdist) {
    int rc = check_um_ice<T>(c, lf, ci, cdist);
    if (rc) return rc;
    const UmCoast &u = c->um;
    const int NX = u.nx + 2 * u.hi;
    const size_t nl = (size_t)NX * (u.ny + 2 * u.hj);
    Stager s(c);
    // (cdist in as well: later calls write the marked workgroups only, the rest of the interior is the caller's from the call before)
    T *dl = s.in(lf, nl), *dc = s.in(ci, nl), *dcd = s.in((const T *)cdist, nl);
    if (s.rc) return s.rc;
    rc = um_ice_dev<T>(c, dl, dc, dcd, nullptr);
    if (rc) return rc;
    // the interior only: the caller's ghost cells are untouched
    hipError_t e = hipMemcpy2DAsync(cdist + (size_t)u.hj * NX + u.hi, (size_t)NX * sizeof(T), dcd + (size_t)u.hj * NX + u.hi,
                                    (size_t)NX * sizeof(T), (size_t)u.nx * sizeof(T), (size_t)u.ny, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return hipfail(c, e, "hipMemcpy2DAsync D2H");
    return s.finish();
}

// ---- one tile of the UM's 2-D decomposition whose coast moves with the sea ice (sb_um_tile_coast_open_*, sb_um_tile_ice_*) ----
// sb_um_ice_* keeps the UM's interior-only rule, so on a decomposed run its field depends on the cut; the tile setup calls
// give the whole-domain field but cost the whole tile per call.  Here the context keeps the coast of the tile's SOURCE
// rectangle (the interior and e* = min(window, beyond*) ghost columns / rows on each side: sb_ice_plan.hpp) as a bit plane
// of its own and the coordinate frames on the device; an ice call is one clear of [marks | changed-word counter],
// k_edge_bits_delta's tile instance and k_dist_um_tile over the marked workgroups.  Nothing waits, nothing is exchanged.
template <typename T>
int um_tile_coast_open(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const int *beyond, const T *tlat_l,
                       const T *tlon_l, T maxdist, int incremental) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    UmTileCoast &u = c->umt;
    if (u.open) return fail(c, SB_ERR_ARG, "sb_um_tile_coast_open: already open (sb_um_tile_coast_close first)");
    if (nx < 1 || ny < 1 || hi < 0 || hj < 0 || !beyond || !tlat_l || !tlon_l) return fail(c, SB_ERR_ARG, "bad um_tile_coast_open arguments");
    if (wi < 0 || wi > SB_DIST_UM_MAX_WINDOW || wj < 0 || wj > SB_DIST_UM_MAX_WINDOW)
        return fail(c, SB_ERR_ARG, "um_tile_coast_open: the window +-" + std::to_string(wi) + " x +-" + std::to_string(wj) +
                                       " needs 0 <= win_i, win_j <= SB_DIST_UM_MAX_WINDOW = " +
                                       std::to_string(SB_DIST_UM_MAX_WINDOW) + " cells");
    if (beyond[0] < 0 || beyond[1] < 0 || beyond[2] < 0 || beyond[3] < 0)
        return fail(c, SB_ERR_ARG, "um_tile_coast_open: beyond[] counts the domain's cells beyond a side: 0 (the domain's edge) or more");
    if ((double)(nx + 2.0 * hi) * (double)(ny + 2.0 * hj) > 2.0e9) return fail(c, SB_ERR_ARG, "grid too large");
    const SbUmTileIcePlan pl = sb_um_tile_ice_plan(nx, ny, hi, hj, wi, wj, beyond, incremental);
    if (!pl.ok) {
        const SbTileReach r = sb_um_tile_ice_sources(wi, wj, beyond);
        return fail(c, SB_ERR_ARG, "um_tile_coast_open: the halo " + std::to_string(hi) + " x " + std::to_string(hj) +
                                       " is smaller than " + std::to_string((r.eW > r.eE ? r.eW : r.eE) + 1) + " x " +
                                       std::to_string((r.eS > r.eN ? r.eS : r.eN) + 1) +
                                       " (min(window, beyond) + 1 on every side: the Sobel reads the ring beyond the last source cell)");
    }
    const SbTileReach r = pl.reach;
    const size_t nl = (size_t)(nx + 2 * hi) * (ny + 2 * hj);
    int rc;
    if ((rc = ensure(c, u.coords, 2 * nl * sizeof(T))) ||
        (rc = ice_open(c, u.it, (size_t)(ny + r.eS + r.eN) * pl.nw * sizeof(uint64_t), pl.marks,
                       pl.path == SbIcePath::WHOLE ? nl * sizeof(T) : 0, incremental, c->stream)))
        return rc;
    HIPCHK(c, hipMemcpyAsync(u.coords.p, tlat_l, nl * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((T *)u.coords.p + nl, tlon_l, nl * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                // (the caller's coordinates may go now)
    u.esz = (int)sizeof(T);
    u.nx = nx; u.ny = ny; u.hi = hi; u.hj = hj; u.wi = wi; u.wj = wj;
    for (int i = 0; i < 4; ++i) u.beyond[i] = beyond[i];
    u.maxdist = (double)maxdist;
    u.open = true;
    return SB_OK;
}

template <typename T>
int check_um_tile_ice(sb_ctx *c, const T *lf, const T *ci, const T *cdist) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    const UmTileCoast &u = c->umt;
    if (!u.open) return fail(c, SB_ERR_ARG, "sb_um_tile_ice without sb_um_tile_coast_open");
    if (u.esz != (int)sizeof(T)) return fail(c, SB_ERR_ARG, "sb_um_tile_ice: the UM tile coast was opened in the other precision");
    if (!lf || !ci || !cdist) return fail(c, SB_ERR_ARG, "null array pointer");
    return SB_OK;
}

template <typename T>
int um_tile_ice_dev(sb_ctx *c, const T *lf, const T *ci, T *cdist, void *stream) {
    int rc = check_um_tile_ice<T>(c, lf, ci, cdist);
    if (rc) return rc;
    UmTileCoast &u = c->umt;
    const int nx = u.nx, ny = u.ny, hi = u.hi, hj = u.hj;
    const SbUmTileIcePlan pl = sb_um_tile_ice_plan(nx, ny, hi, hj, u.wi, u.wj, u.beyond, u.it.incremental);
    const T *tlat = (const T *)u.coords.p, *tlon = tlat + (size_t)(nx + 2 * hi) * (ny + 2 * hj);
    const T maxdist = (T)u.maxdist;
    hipStream_t st = stream_of(c, stream);
    if (pl.path == SbIcePath::WHOLE) {
        // the tile setup calls' chain on the context's own planes, with the reach from `beyond`
        HIPCHK(c, sb_launch_edges_um_tile_reach<T>(lf, ci, (T *)u.it.coast.p, nx, ny, hi, hj, pl.reach, st));
        HIPCHK(c, sb_launch_dist_um_tile_reach<T>((const T *)u.it.coast.p, lf, tlat, tlon, cdist, nx, ny, hi, hj, u.wi, u.wj, pl.reach,
                                                  maxdist, (uint64_t *)u.it.bits.p, st));
    } else {
        IceCall ic;
        if ((rc = ice_begin(c, u.it, st, ic))) return rc;
        HIPCHK(c, sb_launch_edge_bits_delta_um_tile<T>(lf, ci, (uint64_t *)u.it.bits.p, ic.marks, ic.rep, nx, ny, hi, hj, u.wi, u.wj,
                                                       pl.reach, ic.first, st));
        HIPCHK(c, sb_launch_dist_um_tile_dirty<T>(lf, tlat, tlon, cdist, nx, ny, hi, hj, u.wi, u.wj, pl.reach, maxdist,
                                                  (const uint64_t *)u.it.bits.p, ic.marks, st));
    }
    u.it.calls++;
    return SB_OK;
}

template <typename T>
int um_tile_ice_host(sb_ctx *c, const T *lf, const T *ci, T *cdist) {
    int rc = check_um_tile_ice<T>(c, lf, ci, cdist);
    if (rc) return rc;
    const UmTileCoast &u = c->umt;
    const int NX = u.nx + 2 * u.hi;
    const size_t nl = (size_t)NX * (u.ny + 2 * u.hj);
    Stager s(c);
    // (cdist in as well: later calls write the marked workgroups only, the rest of the interior is the caller's from the call before)
    T *dl = s.in(lf, nl), *dc = s.in(ci, nl), *dcd = s.in((const T *)cdist, nl);
    if (s.rc) return s.rc;
    rc = um_tile_ice_dev<T>(c, dl, dc, dcd, nullptr);
    if (rc) return rc;
    // the interior only: the caller's ghost cells are untouched
    hipError_t e = hipMemcpy2DAsync(cdist + (size_t)u.hj * NX + u.hi, (size_t)NX * sizeof(T), dcd + (size_t)u.hj * NX + u.hi,
                                    (size_t)NX * sizeof(T), (size_t)u.nx * sizeof(T), (size_t)u.ny, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return hipfail(c, e, "hipMemcpy2DAsync D2H");
    return s.finish();
}

}  // namespace

extern "C" {

int sb_set_search_radius_hint(sb_ctx *c, int radius) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (radius < 1) return fail(c, SB_ERR_ARG, "radius must be >= 1");
    c->radius_hint = radius;
    return SB_OK;
}

int sb_band_ice_report(sb_ctx *c, long long rep[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rep) return fail(c, SB_ERR_ARG, "null report");
    BandCoast &b = c->bc;
    if (!b.open) return fail(c, SB_ERR_ARG, "sb_band_ice_report without sb_band_coast_open");
    return ice_report(c, b.it, sb_ice_marks(b.nx, b.ny), sb_ice_path(b.nx, b.k, b.it.incremental) == SbIcePath::WHOLE, true, rep);
}

int sb_band_coast_close(sb_ctx *c) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    BandCoast &b = c->bc;
    if (!b.open) return fail(c, SB_ERR_ARG, "sb_band_coast_close without sb_band_coast_open");
    HIPCHK(c, hipDeviceSynchronize());                           // (an ice call may still be reading the planes)
    ice_free(b.it);
    b.lonlat.clear();
    b.open = false;
    return SB_OK;
}

int sb_um_ice_report(sb_ctx *c, long long rep[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rep) return fail(c, SB_ERR_ARG, "null report");
    UmCoast &u = c->um;
    if (!u.open) return fail(c, SB_ERR_ARG, "sb_um_ice_report without sb_um_coast_open");
    return ice_report(c, u.it, sb_um_ice_marks(u.nx, u.ny), sb_um_ice_path(u.it.incremental) == SbIcePath::WHOLE, true, rep);
}

int sb_um_coast_close(sb_ctx *c) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    UmCoast &u = c->um;
    if (!u.open) return fail(c, SB_ERR_ARG, "sb_um_coast_close without sb_um_coast_open");
    HIPCHK(c, hipDeviceSynchronize());                           // (an ice call may still be reading the planes)
    for (DevBuf *d : {&u.coords, &u.lf})
        if (d->p) { (void)hipFree(d->p); d->p = nullptr; d->cap = 0; }
    ice_free(u.it);
    u.open = false;
    return SB_OK;
}

int sb_um_tile_ice_report(sb_ctx *c, long long rep[4]) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    if (!rep) return fail(c, SB_ERR_ARG, "null report");
    UmTileCoast &u = c->umt;
    if (!u.open) return fail(c, SB_ERR_ARG, "sb_um_tile_ice_report without sb_um_tile_coast_open");
    return ice_report(c, u.it, sb_um_ice_marks(u.nx, u.ny), sb_um_ice_path(u.it.incremental) == SbIcePath::WHOLE, true, rep);
}

int sb_um_tile_coast_close(sb_ctx *c) {
    if (!c) return fail(nullptr, SB_ERR_ARG, "null context");
    UmTileCoast &u = c->umt;
    if (!u.open) return fail(c, SB_ERR_ARG, "sb_um_tile_coast_close without sb_um_tile_coast_open");
    HIPCHK(c, hipDeviceSynchronize());                           // (an ice call may still be reading the planes)
    if (u.coords.p) { (void)hipFree(u.coords.p); u.coords.p = nullptr; u.coords.cap = 0; }
    ice_free(u.it);
    u.open = false;
    return SB_OK;
}

#define SB_DEFINE(T, SFX)                                                                                          \
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
    int sb_band_coast_open_##SFX(sb_ctx *c, int nx, int ny, int halo, int south, int north, const T *lon,           \
                                 const T *lat, T maxdist, int kwin, int rule, int incremental) {                    \
        return band_coast_open<T>(c, nx, ny, halo, south, north, lon, lat, maxdist, kwin, rule, incremental);       \
    }                                                                                                              \
    int sb_band_ice_##SFX##_dev(sb_ctx *c, const T *lsm, const T *ci, T *cdist, void *stream) {                     \
        return band_ice_dev<T>(c, lsm, ci, cdist, stream);                                                          \
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
    int sb_tile_get_edges_um_##SFX(sb_ctx *c, int nx, int ny, int hi, int hj, int ei, int ej, int sides, const T *lf, \
                                   const T *ci, T *coast) {                                                        \
        return tile_get_edges_um_host<T>(c, nx, ny, hi, hj, ei, ej, sides, lf, ci, coast);                         \
    }                                                                                                              \
    int sb_tile_get_edges_um_##SFX##_dev(sb_ctx *c, int nx, int ny, int hi, int hj, int ei, int ej, int sides,      \
                                         const T *lf, const T *ci, T *coast, void *stream) {                       \
        return tile_get_edges_um_dev<T>(c, nx, ny, hi, hj, ei, ej, sides, lf, ci, coast, stream);                  \
    }                                                                                                              \
    int sb_tile_get_dist_um_##SFX(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, int sides,            \
                                  const T *coast, const T *lf, const T *tlat, const T *tlon, T maxdist, T *cdist) { \
        return tile_get_dist_um_host<T>(c, nx, ny, hi, hj, wi, wj, sides, coast, lf, tlat, tlon, maxdist, cdist);  \
    }                                                                                                              \
    int sb_tile_get_dist_um_##SFX##_dev(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, int sides,      \
                                        const T *coast, const T *lf, const T *tlat, const T *tlon, T maxdist,      \
                                        T *cdist, void *stream) {                                                  \
        return tile_get_dist_um_dev<T>(c, nx, ny, hi, hj, wi, wj, sides, coast, lf, tlat, tlon, maxdist, cdist,    \
                                       stream);                                                                    \
    }                                                                                                              \
    int sb_um_coast_open_##SFX(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const T *tlat,            \
                               const T *tlon, T maxdist, int incremental) {                                         \
        return um_coast_open<T>(c, nx, ny, hi, hj, wi, wj, tlat, tlon, maxdist, incremental);                       \
    }                                                                                                              \
    int sb_um_ice_##SFX##_dev(sb_ctx *c, const T *lf, const T *ci, T *cdist, void *stream) {                        \
        return um_ice_dev<T>(c, lf, ci, cdist, stream);                                                             \
    }                                                                                                              \
    int sb_um_ice_##SFX(sb_ctx *c, const T *lf, const T *ci, T *cdist) { return um_ice_host<T>(c, lf, ci, cdist); } \
    int sb_um_tile_coast_open_##SFX(sb_ctx *c, int nx, int ny, int hi, int hj, int wi, int wj, const int *beyond,  \
                                    const T *tlat_l, const T *tlon_l, T maxdist, int incremental) {                \
        return um_tile_coast_open<T>(c, nx, ny, hi, hj, wi, wj, beyond, tlat_l, tlon_l, maxdist, incremental);     \
    }                                                                                                              \
    int sb_um_tile_ice_##SFX##_dev(sb_ctx *c, const T *lf, const T *ci, T *cdist, void *stream) {                  \
        return um_tile_ice_dev<T>(c, lf, ci, cdist, stream);                                                       \
    }                                                                                                              \
    int sb_um_tile_ice_##SFX(sb_ctx *c, const T *lf, const T *ci, T *cdist) {                                      \
        return um_tile_ice_host<T>(c, lf, ci, cdist);                                                              \
    }                                                                                                              \
    int sb_dist_window_##SFX(int nx, int ny, const T *lon, const T *lat, T maxdist, int *k) {                       \
        return dist_window<T>(nx, ny, lon, lat, maxdist, k);                                                        \
    }

SB_DEFINE(double, f64)
SB_DEFINE(float, f32)
#undef SB_DEFINE

}  // extern "C"
