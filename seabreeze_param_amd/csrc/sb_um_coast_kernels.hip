// sb_um_coast_kernels.hip -- the UM vn10.7 copy's coast setup on curvilinear (rotated-pole) grids, gfx950.
//
//   k_edges_um     binary 3x3 Sobel of the ice-aware land mask on the tdims_l layout: the rule is applied to the
//                  interior and the one-cell ring of ghost cells round it (what swap_bounds filled), 0/1 goes into the
//                  interior only                          ref: UM/vn10.7/sea_breeze_diag.F90:386-440 (get_edges)
//   k_coastbits    (sb_coast_common.hpp) coast > 0 of the interior, one 64-bit word per 64 columns (a wave ballot)
//   k_dist_um      signed haversine distance to the nearest interior coast cell within +-halo_i columns x +-halo_j
//                  rows, from per-cell coordinates     ref: UM/vn10.7/sea_breeze_diag.F90:448-601 (get_dist)
//   k_dist_um_wide the same rule for a window of up to +-255 cells stated apart from the ghost width (sb_get_dist_um_win_*)
//   k_dist_um_dirty, k_dist_um_wide_dirty  the two under DistUmDirty: only the workgroups an ice call marked (sb_um_ice_*)
//   k_edges_um_tile, k_dist_um_tile  one tile of a 2-D decomposition: ghost cells in reach are sources (sb_tile_get_*_um_*)
//   k_dist_um_tile_dirty  k_dist_um_tile under DistUmTileDirty: only the workgroups an ice call marked (sb_um_tile_ice_*)
//
// The UM's get_dist is a scatter from interior coast cells into a window that reaches into the halo; swap_bounds then
// throws the halo writes away (:584-598).  So sources and targets are interior cells only -- no wrap, no clamp -- and
// the gather below keeps the scatter's result, the sweep-order reset |cdist| > 2*maxdist -> 12000 (:578) included, by
// keeping the minimum over sources swept at or before the target (rows outer, columns inner) apart from the minimum
// over sources swept after it, as k_dist does (sb_coast_kernels.hip).
#include "../../include/seabreeze_hip.h"
#include "sb_launch.hpp"
#include "sb_coast_common.hpp"
#include "sb_ice_plan.hpp"

// (EdgesUm, k_edges_um's layout and land rule: sb_coast_common.hpp -- k_edge_bits_delta's UM instance shares it)
template <typename T>
__global__ __launch_bounds__(256) void k_edges_um(const T *__restrict__ lf, const T *__restrict__ ci, T *__restrict__ coast,
                                                  int nx, int ny, int hi, int hj) {
    __shared__ unsigned char s_land[EDGE_LDS];
    sb_edges_block(lf, ci, coast, s_land, nx, ny, EdgesUm<T>{nx + 2 * hi, ny + 2 * hj, hi, hj});   // ref: UM :420-435
}

// ---- which workgroups a UM distance launch computes, and where landfrac lies ----
// A policy G, the body's last argument (the kernels are thin __global__ wrappers round um_dist_body / um_dist_wide_body, so
// the whole-interior instances keep their names and are the kernels they were before the policy came):
//   (src_row, src_rows, bit_col, co: the row of the coast bit plane a source row is and how many it has, the plane's column of
//   a column, where a cell's coordinates lie -- the interior and nothing else under the first two policies, the expressions
//   the body held before DistUmTile came)
//   DistUmWhole  every workgroup computes; landfrac is an interior (nx, ny) field.  An empty type.
//   DistUmDirty  the coast moves with the sea ice (sb_um_ice_*): a workgroup whose byte of the mark plane (one per
//                SB_UM_ICE_ROWS-row group x 64-column tile, sb_ice_plan.hpp) is clear returns before any bit word, barrier or
//                coordinate, and the stored cdist of its cells stands.  The exit is workgroup-uniform (one byte, read by every
//                thread), so no barrier is left half-entered.  landfrac is read in the interior of its ghost-celled frame:
//                pitch ld, interior at off.
struct DistUmWhole {
    __device__ __forceinline__ bool skip(int, int) const { return false; }
    __device__ __forceinline__ size_t lf(int x, int y, int nx) const { return (size_t)y * nx + x; }
    __device__ __forceinline__ int src_row(int ys) const { return ys; }
    __device__ __forceinline__ int src_rows(int ny) const { return ny; }
    __device__ __forceinline__ int bit_col(int p) const { return p; }
    __device__ __forceinline__ size_t co(int x, int y, int nx) const { return (size_t)y * nx + x; }
};
struct DistUmDirty {
    const unsigned char *mark;
    int ntiles, ld;
    size_t off;
    __device__ __forceinline__ bool skip(int group, int tile) const { return mark[(size_t)group * ntiles + tile] == 0; }
    __device__ __forceinline__ size_t lf(int x, int y, int) const { return off + (size_t)y * ld + x; }
    __device__ __forceinline__ int src_row(int ys) const { return ys; }
    __device__ __forceinline__ int src_rows(int ny) const { return ny; }
    __device__ __forceinline__ int bit_col(int p) const { return p; }
    __device__ __forceinline__ size_t co(int x, int y, int nx) const { return (size_t)y * nx + x; }
};
// DistUmTile (k_dist_um_wide's body only): see k_dist_um_tile below.  landfrac and the coordinates are handed over at the
// interior's first cell, so a cell is y * ld + x; the reach west, south and north (each <= SB_DIST_UM_MAX_WINDOW = 255; east:
// the width of the bit plane says it) travels in one word, so two scalars are all the policy carries -- with them apart the
// fp64 instance went beyond its scalar registers' spill lanes and took a private segment (20 bytes, never addressed).
struct DistUmTile {
    int e, ld;                                                   // e = eW | eS << 8 | eN << 16
    __device__ __forceinline__ int eW() const { return e & 255; }
    __device__ __forceinline__ int eS() const { return (e >> 8) & 255; }
    __device__ __forceinline__ int eN() const { return e >> 16; }
    __device__ __forceinline__ bool skip(int, int) const { return false; }
    __device__ __forceinline__ size_t lf(int x, int y, int) const { return (size_t)y * ld + x; }
    __device__ __forceinline__ int src_row(int ys) const { return ys + eS(); }
    __device__ __forceinline__ int src_rows(int ny) const { return ny + eS() + eN(); }
    __device__ __forceinline__ int bit_col(int p) const { return p + eW(); }
    // (x, y may be negative: a ghost cell west or south of the interior; the offset is taken modulo 2^64 and the cell lies
    // inside the frame)
    __device__ __forceinline__ size_t co(int x, int y, int) const { return (size_t)y * ld + x; }
};
// DistUmTileDirty (sb_um_tile_ice_*): DistUmTile's rows, columns and offsets with DistUmDirty's exit on the mark byte --
// workgroup-uniform and ahead of every barrier, as there.  The launch is one workgroup per byte of the mark plane, so the
// plane's pitch is the grid's width and the policy carries the pointer beside DistUmTile's two scalars and nothing else.
struct DistUmTileDirty : DistUmTile {
    const unsigned char *mark;
    __device__ __forceinline__ bool skip(int group, int tile) const { return mark[(size_t)group * gridDim.x + tile] == 0; }
};

// The gather.  A workgroup holds UM_DIST_TY target rows of 64 columns (one wave per row).  Its reach is the
// (64 + 2hi) x (UM_DIST_TY + 2hj) cells round them; every reach row is one 128-bit string of coast bits in LDS, starting at
// column x0 - hi.  There is no separability on a curvilinear grid -- no per-row cos(phi), no per-column half-angle
// table -- so the per-cell terms of a SOURCE (sin and cos of half its latitude, cos of its latitude, its longitude l1)
// are formed in LDS once per staged coast cell (cells without a coast bit read no coordinates), UM_DIST_CH reach rows at a
// time; a target forms its own (cos(phi), half angles, l2) in registers.
//
// Cuts that hold without separability:
//   * c = 2R atan2(sqrt(a), sqrt(1-a)) + 0.5 grows with a: min(a) per class (before / after the target in the sweep), one
//     atan2 per class per target;
//   * a workgroup with no coast bit in its reach writes 12000 and leaves before it reads any coordinate (four
//     workgroups in five on the BASELINE masks); reach rows and staging chunks without a coast bit are skipped.
// The haversine term is not monotone along a row of a curvilinear grid, so every hit in the window is visited (no
// nearest-hit cut).
//
// fp64: sin((phi_s - phi_t)/2) = sin(phi_s/2) cos(phi_t/2) - cos(phi_s/2) sin(phi_t/2) from the staged half angles (two
// rounded products, no fma: for the same latitude the difference is exactly zero); absolute error ~2e-16, i.e. ~1e-13
// relative in a distance of one 0.1-degree cell.  The longitude difference l1 - l2 takes the sine as written: l1 and l2
// are formed differently (UM :552-563), so a cell's own l1 - l2 need not vanish, and the half-angle identity would not
// reproduce the few-ulp differences that decide distances near a cell.  fp32 takes both sines as written.
#define UM_DIST_TY 4
#define UM_DIST_CH 8
#define UM_DIST_W (64 + 2 * 31)
static_assert(UM_DIST_TY == SB_UM_ICE_ROWS, "a byte of the mark plane is one workgroup of k_dist_um");
template <typename T, typename G>
__device__ __forceinline__ void um_dist_body(const uint64_t *__restrict__ bits, const T *__restrict__ landfrac,
                                             const T *__restrict__ tlat, const T *__restrict__ tlon, T *__restrict__ cdist,
                                             int nx, int ny, int hi, int hj, int nw, T maxdist, const G g) {
    if (g.skip(blockIdx.y, blockIdx.x)) return;                    // workgroup-uniform, ahead of every barrier
    __shared__ uint64_t s_bw[UM_DIST_TY + 62][2];
    __shared__ T s_sh[UM_DIST_CH][UM_DIST_W], s_ch[UM_DIST_CH][UM_DIST_W], s_cp[UM_DIST_CH][UM_DIST_W], s_l1[UM_DIST_CH][UM_DIST_W];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, tid = threadIdx.x;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * UM_DIST_TY;
    const int xx = x0 + tx, yy = y0 + ty;
    const bool valid = xx < nx && yy < ny;
    const int NX = nx + 2 * hi;
    const int RR = UM_DIST_TY + 2 * hj, W = 64 + 2 * hi, L = 2 * hi + 1;
    const T big = SbDist<T>::big;
    // ---- the coast bits of the reach, and which reach rows hold any ----
    bool any = false;
    for (int i = tid; i < 2 * RR; i += 64 * UM_DIST_TY) {
        const int r = i >> 1, j = i & 1, ys = y0 - hj + r;
        uint64_t v = 0;
        if (ys >= 0 && ys < ny) {
            v = um_row_bits64(bits + (size_t)ys * nw, x0 - hi + 64 * j, nw);
            if (j) v &= hi ? (1ull << (2 * hi)) - 1ull : 0ull;      // (reach: W = 64 + 2hi columns)
        }
        s_bw[r][j] = v;
        any |= v != 0;
    }
    if (!__syncthreads_or(any ? 1 : 0)) {                          // no coast cell in reach: no coordinates, no trigonometry
        if (valid) cdist[(size_t)(yy + hj) * NX + xx + hi] = big;
        return;
    }
    // ---- this target's own terms ----
    const T pi = T(3.1415926), r2d = T(180.0) / pi, d2r = pi / T(180.0);      // ref: UM :509-512
    T phit = T(0), cost = T(0), sht = T(0), cht = T(0), l2 = T(0), lf = T(0);
    if (valid) {
        const size_t o = (size_t)yy * nx + xx;
        phit = tlat[o] * d2r;                                      // phi1 (ref: UM :524)
        const T lam1 = tlon[o] * d2r;                              // lam1 (:523)
        l2 = ((r2d * lam1) > T(180.)) ? d2r * ((r2d * lam1) - T(360.)) : lam1;   // ref: UM :560-564
        cost = cos(phit);
        if constexpr (sizeof(T) == 8) { sht = sin(phit / T(2)); cht = cos(phit / T(2)); }
        lf = landfrac[g.lf(xx, yy, nx)];
    }
    T a_early = SbDist<T>::none, a_late = SbDist<T>::none;
    const uint64_t lmask = (1ull << L) - 1ull;                     // (L <= 63)
    // ---- UM_DIST_CH reach rows at a time: stage the coast cells' terms, then every wave walks the rows of its window ----
    for (int r0 = 0; r0 < RR; r0 += UM_DIST_CH) {
        const int nr = RR - r0 < UM_DIST_CH ? RR - r0 : UM_DIST_CH;
        bool chunk = false;                                        // workgroup-uniform: the bits are in LDS
        for (int r = 0; r < nr; ++r) chunk |= (s_bw[r0 + r][0] | s_bw[r0 + r][1]) != 0;
        if (!chunk) continue;
        __syncthreads();                                           // (the chunk before is read by every wave)
        for (int i = tid; i < nr * W; i += 64 * UM_DIST_TY) {
            const int r = i / W, cc = i - r * W;
            if (!((s_bw[r0 + r][cc >> 6] >> (cc & 63)) & 1ull)) continue;
            const size_t o = (size_t)(y0 - hj + r0 + r) * nx + (x0 - hi + cc);   // (a set bit is an interior cell)
            const T lat = tlat[o], lon = tlon[o];
            const T phis = lat * d2r;
            s_l1[r][cc] = (lon > T(180)) ? d2r * (lon - T(360.)) : d2r * lon;     // ref: UM :552-556
            s_cp[r][cc] = cos(phis);
            if constexpr (sizeof(T) == 8) { s_sh[r][cc] = sin(phis / T(2)); s_ch[r][cc] = cos(phis / T(2)); }
            else s_sh[r][cc] = phis;
        }
        __syncthreads();
        if (!valid) continue;
        // reach rows ty .. ty + 2hj are this wave's window (source row ys = yy + ii, ii = r - ty - hj)
        const int lo = ty > r0 ? ty : r0, hiw = (ty + 2 * hj < r0 + nr - 1) ? ty + 2 * hj : r0 + nr - 1;
        for (int r = lo; r <= hiw; ++r) {
            const uint64_t s0 = s_bw[r][0], s1 = s_bw[r][1];
            if ((s0 | s1) == 0) continue;                          // workgroup-uniform
            uint64_t wb = (s0 >> tx) | (tx ? s1 << (64 - tx) : 0ull);
            wb &= lmask;
            const int rc = r - r0, ii = r - ty - hj;
            while (wb) {
                const int b = __builtin_ctzll(wb);
                wb &= wb - 1ull;
                const int cc = tx + b;                             // reach column of source column xx - hi + b
                T sp;
                if constexpr (sizeof(T) == 8) sp = s_sh[rc][cc] * cht - s_ch[rc][cc] * sht;
                else sp = sin((s_sh[rc][cc] - phit) / T(2));
                const T dlam = s_l1[rc][cc] - l2;                  // l1 - l2 (ref: UM :565)
                const T sl = sin(dlam / T(2));
                const T a = sb_hav(sp * sp, s_cp[rc][cc], cost, sl);
                const bool early = ii < 0 || (ii == 0 && b <= hi);
                if (early) a_early = a < a_early ? a : a_early;
                else a_late = a < a_late ? a : a_late;
            }
        }
    }
    if (!valid) return;
    sb_dist_write(cdist + (size_t)(yy + hj) * NX + xx + hi, sb_dist_finish_both(a_early, a_late, maxdist), &lf);
}
template <typename T>
__global__ __launch_bounds__(64 * UM_DIST_TY) void k_dist_um(const uint64_t *__restrict__ bits, const T *__restrict__ landfrac,
                                                           const T *__restrict__ tlat, const T *__restrict__ tlon,
                                                           T *__restrict__ cdist, int nx, int ny, int hi, int hj, int nw,
                                                           T maxdist) {
    um_dist_body<T>(bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, nw, maxdist, DistUmWhole{});
}
// landfrac: the first cell of the ghost-celled frame (g says where its interior lies)
template <typename T>
__global__ __launch_bounds__(64 * UM_DIST_TY) void k_dist_um_dirty(const uint64_t *__restrict__ bits,
                                                                 const T *__restrict__ landfrac, const T *__restrict__ tlat,
                                                                 const T *__restrict__ tlon, T *__restrict__ cdist, int nx,
                                                                 int ny, int hi, int hj, int nw, T maxdist, DistUmDirty g) {
    um_dist_body<T>(bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, nw, maxdist, g);
}

// ------------------------------------------------------------------------------------
// k_dist_um_wide: the gather for a window of +-wi columns x +-wj rows stated apart from the layout's ghost width
// (hi, hj), 0 <= wi, wj <= SB_DIST_UM_MAX_WINDOW (113 cells at 0.0135 degrees and 180 km).  Rule and classes are
// k_dist_um's; what changes is what is resident.  A workgroup is UMW_TY target rows of 64 columns (a wave per row); its
// reach is up to 64 + 2*255 = 574 columns and UMW_TY + 2*255 rows, so
//   * a reach row is a bit string of UMW_WORDS words from column x0 - wi on; the source rows are staged in passes that go
//     outwards from the target rows (pass 0: the target rows and UMW_A rows either side, nearest first and sides
//     alternating; pass j: the next UMW_A either side), so each sweep class meets its rows nearest first;
//   * the per-source terms (phi, cos(phi), l1) are staged for coast cells only, in a compact list of UMW_CAP entries:
//     the rows of a pass are taken in chunks of as many consecutive slots as the list holds (a row has at most
//     574 <= UMW_CAP coast cells), s_off[slot][word] is the list index of the word's first coast cell, and a target
//     finds the entry of bit b as s_off + popcount(bits below b).  LDS does not grow with the window;
//   * a workgroup with no coast bit in its reach reads bit words only, writes 12000 and leaves; a pass without a bit
//     costs its bit words, a row without one nothing more.
// fp64 takes both sines on the difference as written, sin((phi_s - phi_t)/2) and sin((l1 - l2)/2): the half-angle
// identity of k_dist_um carries an absolute error of ~2e-16 that a half-difference of 1e-4 rad (km-scale spacing) no
// longer hides (up to 1.07e-12 relative, measured).  An argument of magnitude <= UMW_SIN_POLY_MAX = 0.5 rad goes
// through the odd Taylor polynomial up to x^15 (truncation x^16/17! <= 4.3e-20 relative there); anything larger (the
// longitude term of pairs either side of 180 degrees, or near a pole) through the library sine.  fp32 takes both
// library sines as written, as k_dist_um does.
// The per-pair cut: a = sp^2 + cos(phi_s) (cos(phi_t) sl^2) >= sp^2 when both cosines are >= 0 (every product of
// non-negative terms is >= 0, and adding a non-negative term never rounds below sp^2), so a hit with sp^2 >= its
// class's minimum cannot lower it and skips the longitude sine.  Both cosines are checked per pair.
// -DSB_UM_WIN_NO_LAT_CUT builds the kernel without the cut (A/B: the field is the same to the last bit).
// ------------------------------------------------------------------------------------
#define UMW_TY 4                                                 // target rows per workgroup
#define UMW_A 30                                                 // source rows above, and below, per pass
#define UMW_SLOTS (2 * UMW_A + UMW_TY)                           // rows of bit strings resident in LDS
#define UMW_SPAN (64 + 2 * SB_DIST_UM_MAX_WINDOW)                // columns a workgroup's 64 targets can reach
#define UMW_WORDS ((UMW_SPAN + 63) / 64)
#define UMW_CAP 1024                                             // entries of the compact source list
#define UMW_SIN_POLY_MAX 0.5
static_assert(SB_DIST_UM_MAX_WINDOW <= 255, "DistUmTile packs a reach into eight bits");
static_assert(UMW_CAP >= UMW_SPAN, "k_dist_um_wide: a chunk holds at least one row");
static_assert(UMW_CAP <= 65535 && UMW_SLOTS <= 64 * UMW_TY, "k_dist_um_wide: 16-bit list offsets, a thread per slot");

// sin(x) for |x| <= UMW_SIN_POLY_MAX: x + x^3 P(x^2), the Taylor terms up to x^15
__device__ __forceinline__ double um_sin_poly(double x) {
    const double z = x * x;
    double p = -1.0 / 1307674368000.0;
    p = __builtin_fma(p, z, 1.0 / 6227020800.0);
    p = __builtin_fma(p, z, -1.0 / 39916800.0);
    p = __builtin_fma(p, z, 1.0 / 362880.0);
    p = __builtin_fma(p, z, -1.0 / 5040.0);
    p = __builtin_fma(p, z, 1.0 / 120.0);
    p = __builtin_fma(p, z, -1.0 / 6.0);
    return __builtin_fma(x * z, p, x);
}
template <typename T>
__device__ __forceinline__ T um_sin_as_written(T x) {
    if constexpr (sizeof(T) == 8) return fabs(x) <= UMW_SIN_POLY_MAX ? um_sin_poly(x) : sin(x);
    else return sin(x);
}

static_assert(UMW_TY == SB_UM_ICE_ROWS, "a byte of the mark plane is one workgroup of k_dist_um_wide");
template <typename T, typename G>
__device__ __forceinline__ void um_dist_wide_body(const uint64_t *__restrict__ bits, const T *__restrict__ landfrac,
                                                  const T *__restrict__ tlat, const T *__restrict__ tlon,
                                                  T *__restrict__ cdist, int nx, int ny, int hi, int hj, int wi, int wj,
                                                  int nw, T maxdist, const G g) {
    if (g.skip(blockIdx.y, blockIdx.x)) return;                  // workgroup-uniform, ahead of every barrier
    __shared__ uint64_t s_bw[UMW_SLOTS][UMW_WORDS];
    __shared__ unsigned short s_off[UMW_SLOTS][UMW_WORDS], s_cnt[UMW_SLOTS];
    __shared__ T s_phi[UMW_CAP], s_cp[UMW_CAP], s_l1[UMW_CAP];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, tid = threadIdx.x;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * UMW_TY;
    const int xx = x0 + tx, yy = y0 + ty;
    const bool valid = xx < nx && yy < ny;                       // (every thread stays for the barriers)
    const int NX = nx + 2 * hi;
    const int W = 64 + 2 * wi, nws = (W + 63) >> 6;              // the reach: W columns from x0 - wi on, nws <= UMW_WORDS words
    const uint64_t lastmask = (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull;
    const int qlo = tx, qhi = tx + 2 * wi, qown = tx + wi;       // this target's window in the strings, its own column
    const T pi = T(3.1415926), r2d = T(180.0) / pi, d2r = pi / T(180.0);      // ref: UM :509-512
    // slot s of pass j: the distance of its row from the block of target rows (0: a target row) and the row itself
    // (which may lie outside 0 .. ny-1)
    auto slot_k = [&](int s, int j) { return j == 0 ? (s < UMW_TY ? 0 : 1 + ((s - UMW_TY) >> 1)) : 1 + UMW_A * j + (s >> 1); };
    auto slot_row = [&](int s, int j) {
        if (j == 0 && s < UMW_TY) return y0 + s;
        const int k = slot_k(s, j), below = (j == 0 ? s - UMW_TY : s) & 1;
        return below ? y0 + UMW_TY - 1 + k : y0 - k;
    };
    T a_early = SbDist<T>::none, a_late = SbDist<T>::none;
    T phit = T(0), cost = T(0), l2 = T(0);
    bool have = false;                                           // this target's own terms are loaded (workgroup-uniform)
    const int npass = wj == 0 ? 1 : (wj + UMW_A - 1) / UMW_A;
    for (int j = 0; j < npass; ++j) {
        __syncthreads();                                         // (the pass before is read by every wave)
        const int ns = j == 0 ? UMW_SLOTS : 2 * UMW_A;
        int anyv = 0;
        for (int i = tid; i < ns * UMW_WORDS; i += 64 * UMW_TY) {
            const int s = i / UMW_WORDS, w = i - s * UMW_WORDS, ys = g.src_row(slot_row(s, j));   // (row of the bit plane)
            uint64_t v = 0;
            if (w < nws && slot_k(s, j) <= wj && ys >= 0 && ys < g.src_rows(ny)) {
                v = um_row_bits64(bits + (size_t)ys * nw, g.bit_col(x0 - wi + 64 * w), nw);
                if (w == nws - 1) v &= lastmask;
            }
            s_bw[s][w] = v;
            anyv |= v != 0 ? 1 : 0;
        }
        if (!__syncthreads_or(anyv)) continue;                   // no coast cell in this pass's rows within reach
        if (tid < ns) {
            int c = 0;
            for (int w = 0; w < nws; ++w) c += __builtin_popcountll(s_bw[tid][w]);
            s_cnt[tid] = (unsigned short)c;
        }
        if (!have) {                                             // the first coordinates this workgroup reads
            have = true;
            if (valid) {
                const size_t o = g.co(xx, yy, nx);
                phit = tlat[o] * d2r;                            // phi1 (ref: UM :524)
                const T lam1 = tlon[o] * d2r;                    // lam1 (:523)
                l2 = ((r2d * lam1) > T(180.)) ? d2r * ((r2d * lam1) - T(360.)) : lam1;   // ref: UM :560-564
                cost = cos(phit);
            }
        }
        __syncthreads();
        for (int cs = 0; cs < ns;) {
            // the chunk: slots cs .. ce-1, as many as the list holds (workgroup-uniform: the counts are in LDS)
            int ce = cs, tot = 0;
            while (ce < ns && tot + s_cnt[ce] <= UMW_CAP) tot += s_cnt[ce++];
            if (tot == 0) { cs = ce; continue; }
            __syncthreads();                                     // (the chunk before is read by every wave)
            if (tid >= cs && tid < ce) {
                int e = 0;
                for (int s = cs; s < tid; ++s) e += s_cnt[s];
                for (int w = 0; w < nws; ++w) {
                    s_off[tid][w] = (unsigned short)e;
                    e += __builtin_popcountll(s_bw[tid][w]);
                }
            }
            __syncthreads();
            // the coast cells' terms, a thread per (slot, word): cells without a coast bit read no coordinates
            for (int i = tid; i < (ce - cs) * nws; i += 64 * UMW_TY) {
                const int s = cs + i / nws, w = i - (s - cs) * nws;
                uint64_t v = s_bw[s][w];
                if (!v) continue;
                int e = s_off[s][w];
                const size_t orow = g.co(0, slot_row(s, j), nx);
                while (v) {
                    const int b = __builtin_ctzll(v);
                    v &= v - 1ull;
                    const size_t o = orow + (x0 - wi + 64 * w + b);      // (a set bit is a source cell: interior, or under DistUmTile a ghost cell in reach)
                    const T lat = tlat[o], lon = tlon[o];
                    const T phis = lat * d2r;
                    s_phi[e] = phis;
                    s_cp[e] = cos(phis);
                    s_l1[e] = (lon > T(180)) ? d2r * (lon - T(360.)) : d2r * lon;     // ref: UM :552-556
                    ++e;
                }
            }
            __syncthreads();
            if (valid)
                for (int s = cs; s < ce; ++s) {
                    if (!s_cnt[s]) continue;                     // workgroup-uniform
                    const int ii = slot_row(s, j) - yy;          // source row yy + ii
                    if (ii < -wj || ii > wj) continue;           // wave-uniform
                    for (int wd = qlo >> 6; wd <= qhi >> 6; ++wd) {
                        const uint64_t full = s_bw[s][wd];
                        uint64_t v = full;
                        if (wd == qlo >> 6) v &= ~0ull << (qlo & 63);
                        if (wd == qhi >> 6) v &= ~0ull >> (63 - (qhi & 63));
                        if (!v) continue;
                        const int base = s_off[s][wd];
                        while (v) {
                            const int b = __builtin_ctzll(v);
                            v &= v - 1ull;
                            const int e = base + __builtin_popcountll(full & ((1ull << b) - 1ull));
                            const bool early = ii < 0 || (ii == 0 && 64 * wd + b <= qown);
                            const T sp = um_sin_as_written<T>((s_phi[e] - phit) / T(2));      // dphi (ref: UM :565)
                            const T sp2 = sp * sp, cps = s_cp[e];
#ifndef SB_UM_WIN_NO_LAT_CUT
                            if (cost >= T(0) && cps >= T(0) && sp2 >= (early ? a_early : a_late)) continue;
#endif
                            const T dlam = s_l1[e] - l2;         // l1 - l2 (ref: UM :565)
                            const T sl = um_sin_as_written<T>(dlam / T(2));
                            const T a = sb_hav(sp2, cps, cost, sl);
                            if (early) a_early = a < a_early ? a : a_early;
                            else a_late = a < a_late ? a : a_late;
                        }
                    }
                }
            cs = ce;
        }
    }
    if (!valid) return;
    sb_dist_write(cdist + (size_t)(yy + hj) * NX + xx + hi, sb_dist_finish_both(a_early, a_late, maxdist),
                  landfrac + g.lf(xx, yy, nx));
}
template <typename T>
__global__ __launch_bounds__(64 * UMW_TY) void k_dist_um_wide(const uint64_t *__restrict__ bits, const T *__restrict__ landfrac,
                                                              const T *__restrict__ tlat, const T *__restrict__ tlon,
                                                              T *__restrict__ cdist, int nx, int ny, int hi, int hj, int wi,
                                                              int wj, int nw, T maxdist) {
    um_dist_wide_body<T>(bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, wi, wj, nw, maxdist, DistUmWhole{});
}
template <typename T>
__global__ __launch_bounds__(64 * UMW_TY) void k_dist_um_wide_dirty(const uint64_t *__restrict__ bits,
                                                                    const T *__restrict__ landfrac, const T *__restrict__ tlat,
                                                                    const T *__restrict__ tlon, T *__restrict__ cdist, int nx,
                                                                    int ny, int hi, int hj, int wi, int wj, int nw, T maxdist,
                                                                    DistUmDirty g) {
    um_dist_wide_body<T>(bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, wi, wj, nw, maxdist, g);
}

// ------------------------------------------------------------------------------------
// One tile of a 2-D domain decomposition (sb_tile_get_edges_um_*, sb_tile_get_dist_um_*): every field is the rank's frame
// of (nx + 2hi) x (ny + 2hj) cells with the interior at (hi, hj), ghost cells filled by the caller's swap_bounds.  A side
// is a CUT (a neighbour's cells lie beyond it) or an EDGE of the domain (nothing beyond it is a source or is written).
//   k_edges_um_tile  sb_edges_block under EdgesUmTile (sb_coast_common.hpp): the written rectangle is the interior and
//                    `ext` ghost columns / rows on every cut side, so a rank forms the coast of its ghost cells itself;
//   k_dist_um_tile   um_dist_wide_body under DistUmTile.  Sources are the coast cells of [-eW, nx+eE) x [-eS, ny+eN) in
//                    interior coordinates, e* = the window on a cut side and 0 on an edge side: the plane's rows are the source rows
//                    (src_row, src_rows: the test 0 <= ys < ny is taken on those), and the coast bit plane spans exactly that
//                    rectangle (pitch nw words, origin (-eW, -eS): bit_col), so um_row_bits64's zeros beyond the plane are the column clip.  Targets are the
//                    interior; coordinates and landfrac are read through the frame's pitch and offset (co, lf).  Whether a
//                    source is swept at or before a target is decided on row and column DIFFERENCES (ii, 64 wd + b <=
//                    qown), which a translation of the origin leaves alone: the sweep-order reset survives the cut.  No exit
//                    is added (skip is false), LDS is the body's.
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_edges_um_tile(const T *__restrict__ lf, const T *__restrict__ ci, T *__restrict__ coast,
                                                       int wx, int wy, EdgesUmTile<T> p) {
    __shared__ unsigned char s_land[EDGE_LDS];
    sb_edges_block(lf, ci, coast, s_land, wx, wy, p);
}
template <typename T>
__global__ __launch_bounds__(64 * UMW_TY) void k_dist_um_tile(const uint64_t *__restrict__ bits, const T *__restrict__ landfrac,
                                                              const T *__restrict__ tlat, const T *__restrict__ tlon,
                                                              T *__restrict__ cdist, int nx, int ny, int hi, int hj, int wi,
                                                              int wj, int nw, T maxdist, DistUmTile g) {
    // (landfrac, tlat, tlon: the interior's first cell of their frames; cdist: the frame's first cell, as in k_dist_um_wide)
    um_dist_wide_body<T>(bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, wi, wj, nw, maxdist, g);
}

template <typename T>
__global__ __launch_bounds__(64 * UMW_TY) void k_dist_um_tile_dirty(const uint64_t *__restrict__ bits,
                                                                    const T *__restrict__ landfrac, const T *__restrict__ tlat,
                                                                    const T *__restrict__ tlon, T *__restrict__ cdist, int nx,
                                                                    int ny, int hi, int hj, int wi, int wj, int nw, T maxdist,
                                                                    DistUmTileDirty g) {
    // (the pointers as in k_dist_um_tile; the bit plane is complete: k_edge_bits_delta's tile instance wrote it)
    um_dist_wide_body<T>(bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, wi, wj, nw, maxdist, g);
}

// what a tile call reaches beyond its interior on each side (SbTileReach: sb_ice_plan.hpp): `e` cells on a cut side, none
// on an edge side
static inline SbTileReach sb_tile_reach(int sides, int ei, int ej) {
    return SbTileReach{(sides & SB_TILE_WEST) ? 0 : ei, (sides & SB_TILE_EAST) ? 0 : ei, (sides & SB_TILE_SOUTH) ? 0 : ej,
                       (sides & SB_TILE_NORTH) ? 0 : ej};
}

template <typename T>
hipError_t sb_launch_edges_um_tile_reach(const T *lf, const T *ci, T *coast, int nx, int ny, int hi, int hj, SbTileReach r,
                                         hipStream_t st) {
    // the ring the Sobel reads lies inside the frame: one cell beyond the written rectangle on every side
    if (r.eW < 0 || r.eE < 0 || r.eS < 0 || r.eN < 0 || hi < r.eW + 1 || hi < r.eE + 1 || hj < r.eS + 1 || hj < r.eN + 1)
        return hipErrorInvalidValue;
    const int wx = nx + r.eW + r.eE, wy = ny + r.eS + r.eN;
    const EdgesUmTile<T> p{nx + 2 * hi, ny + 2 * hj, hi - r.eW, hj - r.eS};
    hipLaunchKernelGGL(k_edges_um_tile<T>, dim3((wx + 255) / 256, (wy + EDGE_ROWS - 1) / EDGE_ROWS), dim3(256), 0, st, lf, ci, coast,
                       wx, wy, p);
    return hipGetLastError();
}
template <typename T>
hipError_t sb_launch_edges_um_tile(const T *lf, const T *ci, T *coast, int nx, int ny, int hi, int hj, int ei, int ej, int sides,
                                   hipStream_t st) {
    if (ei < 0 || ej < 0) return hipErrorInvalidValue;
    return sb_launch_edges_um_tile_reach<T>(lf, ci, coast, nx, ny, hi, hj, sb_tile_reach(sides, ei, ej), st);
}

size_t sb_dist_um_tile_bits_bytes(int nx, int ny, int wi, int wj, int sides) {
    const SbTileReach r = sb_tile_reach(sides, wi, wj);
    return (size_t)(ny + r.eS + r.eN) * ((nx + r.eW + r.eE + 63) / 64) * sizeof(uint64_t);
}

static bool um_tile_reach_ok(int hi, int hj, int wi, int wj, const SbTileReach &r) {
    if (wi < 0 || wi > SB_DIST_UM_MAX_WINDOW || wj < 0 || wj > SB_DIST_UM_MAX_WINDOW) return false;
    // DistUmTile packs a reach into eight bits; a reach beyond the window holds no source
    if (r.eW < 0 || r.eE < 0 || r.eS < 0 || r.eN < 0 || r.eW > wi || r.eE > wi || r.eS > wj || r.eN > wj) return false;
    // every source cell lies inside the frame
    return hi >= r.eW && hi >= r.eE && hj >= r.eS && hj >= r.eN;
}

template <typename T>
hipError_t sb_launch_dist_um_tile_reach(const T *coast_l, const T *landfrac_l, const T *tlat_l, const T *tlon_l, T *cdist_l, int nx,
                                        int ny, int hi, int hj, int wi, int wj, SbTileReach r, T maxdist, uint64_t *bits,
                                        hipStream_t st) {
    if (!um_tile_reach_ok(hi, hj, wi, wj, r)) return hipErrorInvalidValue;
    const int wx = nx + r.eW + r.eE, wy = ny + r.eS + r.eN, nw = (wx + 63) / 64, NX = nx + 2 * hi;
    // (two launches: the bit plane is complete before any cdist cell is written, so cdist_l may be coast_l)
    sb_launch_coastbits<T>(coast_l, bits, wx, wy, nw, NX, (size_t)(hj - r.eS) * NX + (hi - r.eW), st);
    const DistUmTile g{r.eW | (r.eS << 8) | (r.eN << 16), NX};
    const size_t o = (size_t)hj * NX + hi;                       // the interior's first cell (cdist_l: the body adds it itself)
    hipLaunchKernelGGL(k_dist_um_tile<T>, dim3((nx + 63) / 64, (ny + UMW_TY - 1) / UMW_TY), dim3(64 * UMW_TY), 0, st, bits,
                       landfrac_l + o, tlat_l + o, tlon_l + o, cdist_l, nx, ny, hi, hj, wi, wj, nw, maxdist, g);
    return hipGetLastError();
}
template <typename T>
hipError_t sb_launch_dist_um_tile(const T *coast_l, const T *landfrac_l, const T *tlat_l, const T *tlon_l, T *cdist_l, int nx,
                                  int ny, int hi, int hj, int wi, int wj, int sides, T maxdist, uint64_t *bits, hipStream_t st) {
    if (wi < 0 || wj < 0) return hipErrorInvalidValue;
    return sb_launch_dist_um_tile_reach<T>(coast_l, landfrac_l, tlat_l, tlon_l, cdist_l, nx, ny, hi, hj, wi, wj,
                                           sb_tile_reach(sides, wi, wj), maxdist, bits, st);
}

// k_dist_um_tile over a bit plane that is already complete (k_edge_bits_delta's tile instance wrote it: the source
// rectangle r, pitch ceil((nx+eW+eE)/64) words), computing the marked workgroups of the interior alone.  Every pointer is
// the frame's first cell; marks: one byte per workgroup, ceil(ny/4) x ceil(nx/64) -- the grid, which is the plane's pitch
// DistUmTileDirty reads.
template <typename T>
hipError_t sb_launch_dist_um_tile_dirty(const T *landfrac_l, const T *tlat_l, const T *tlon_l, T *cdist_l, int nx, int ny, int hi,
                                        int hj, int wi, int wj, SbTileReach r, T maxdist, const uint64_t *bits,
                                        const unsigned char *marks, hipStream_t st) {
    if (!um_tile_reach_ok(hi, hj, wi, wj, r)) return hipErrorInvalidValue;
    const int nw = (nx + r.eW + r.eE + 63) / 64, NX = nx + 2 * hi;
    const SbIceMarks m = sb_um_ice_marks(nx, ny);
    const DistUmTileDirty g{{r.eW | (r.eS << 8) | (r.eN << 16), NX}, marks};
    const size_t o = (size_t)hj * NX + hi;
    hipLaunchKernelGGL(k_dist_um_tile_dirty<T>, dim3(m.tiles, m.rows), dim3(64 * UMW_TY), 0, st, bits, landfrac_l + o, tlat_l + o,
                       tlon_l + o, cdist_l, nx, ny, hi, hj, wi, wj, nw, maxdist, g);
    return hipGetLastError();
}

template <typename T>
hipError_t sb_launch_edges_um(const T *lf, const T *ci, T *coast, int nx, int ny, int hi, int hj, hipStream_t st) {
    hipLaunchKernelGGL(k_edges_um<T>, dim3((nx + 255) / 256, (ny + EDGE_ROWS - 1) / EDGE_ROWS), dim3(256), 0, st,
                       lf, ci, coast, nx, ny, hi, hj);
    return hipGetLastError();
}

template <typename T>
hipError_t sb_launch_dist_um_win(const T *coast, const T *landfrac, const T *tlat, const T *tlon, T *cdist, int nx, int ny,
                                 int hi, int hj, int wi, int wj, T maxdist, uint64_t *bits, hipStream_t st) {
    if (hi < 0 || hj < 0 || wi < 0 || wi > SB_DIST_UM_MAX_WINDOW || wj < 0 || wj > SB_DIST_UM_MAX_WINDOW) return hipErrorInvalidValue;
    const int nw = (nx + 63) / 64, NX = nx + 2 * hi;
    // (two launches: the bit plane is complete before any cdist cell is written, so cdist may be coast)
    sb_launch_coastbits<T>(coast, bits, nx, ny, nw, NX, (size_t)hj * NX + hi, st);
    // window = ghost width <= 31: sb_get_dist_um_*'s call, its kernel and its field, bit for bit
    if (wi == hi && wj == hj && wi <= 31 && wj <= 31)
        hipLaunchKernelGGL(k_dist_um<T>, dim3((nx + 63) / 64, (ny + UM_DIST_TY - 1) / UM_DIST_TY), dim3(64 * UM_DIST_TY), 0, st,
                           bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, nw, maxdist);
    else
        hipLaunchKernelGGL(k_dist_um_wide<T>, dim3((nx + 63) / 64, (ny + UMW_TY - 1) / UMW_TY), dim3(64 * UMW_TY), 0, st,
                           bits, landfrac, tlat, tlon, cdist, nx, ny, hi, hj, wi, wj, nw, maxdist);
    return hipGetLastError();
}

// sb_launch_dist_um_win's choice of kernel over a bit plane that is already complete (k_edge_bits_delta wrote it),
// computing the marked workgroups alone.  landfrac_l: the ghost-celled frame, read in its interior; marks: one byte per
// workgroup, ceil(ny/4) x ceil(nx/64).  One workgroup per tile as ever: an unmarked one leaves at once.
template <typename T>
hipError_t sb_launch_dist_um_dirty(const T *landfrac_l, const T *tlat, const T *tlon, T *cdist, int nx, int ny, int hi, int hj,
                                   int wi, int wj, T maxdist, const uint64_t *bits, const unsigned char *marks, hipStream_t st) {
    if (hi < 0 || hj < 0 || wi < 0 || wi > SB_DIST_UM_MAX_WINDOW || wj < 0 || wj > SB_DIST_UM_MAX_WINDOW) return hipErrorInvalidValue;
    const int nw = (nx + 63) / 64, NX = nx + 2 * hi;
    const SbIceMarks m = sb_um_ice_marks(nx, ny);
    const DistUmDirty g{marks, m.tiles, NX, (size_t)hj * NX + hi};
    const dim3 grid(m.tiles, m.rows);
    if (wi == hi && wj == hj && wi <= 31 && wj <= 31)
        hipLaunchKernelGGL(k_dist_um_dirty<T>, grid, dim3(64 * UM_DIST_TY), 0, st, bits, landfrac_l, tlat, tlon, cdist, nx, ny, hi,
                           hj, nw, maxdist, g);
    else
        hipLaunchKernelGGL(k_dist_um_wide_dirty<T>, grid, dim3(64 * UMW_TY), 0, st, bits, landfrac_l, tlat, tlon, cdist, nx, ny, hi,
                           hj, wi, wj, nw, maxdist, g);
    return hipGetLastError();
}

template hipError_t sb_launch_dist_um_dirty<float>(const float *, const float *, const float *, float *, int, int, int, int, int,
                                                   int, float, const uint64_t *, const unsigned char *, hipStream_t);
template hipError_t sb_launch_dist_um_dirty<double>(const double *, const double *, const double *, double *, int, int, int, int,
                                                    int, int, double, const uint64_t *, const unsigned char *, hipStream_t);
template hipError_t sb_launch_edges_um<float>(const float *, const float *, float *, int, int, int, int, hipStream_t);
template hipError_t sb_launch_edges_um<double>(const double *, const double *, double *, int, int, int, int, hipStream_t);

template hipError_t sb_launch_dist_um_win<float>(const float *, const float *, const float *, const float *, float *, int,
                                                 int, int, int, int, int, float, uint64_t *, hipStream_t);
template hipError_t sb_launch_dist_um_win<double>(const double *, const double *, const double *, const double *, double *,
                                                  int, int, int, int, int, int, double, uint64_t *, hipStream_t);

template hipError_t sb_launch_edges_um_tile<float>(const float *, const float *, float *, int, int, int, int, int, int, int,
                                                   hipStream_t);
template hipError_t sb_launch_edges_um_tile<double>(const double *, const double *, double *, int, int, int, int, int, int, int,
                                                    hipStream_t);
template hipError_t sb_launch_dist_um_tile<float>(const float *, const float *, const float *, const float *, float *, int, int,
                                                  int, int, int, int, int, float, uint64_t *, hipStream_t);
template hipError_t sb_launch_dist_um_tile<double>(const double *, const double *, const double *, const double *, double *, int,
                                                   int, int, int, int, int, int, double, uint64_t *, hipStream_t);
template hipError_t sb_launch_edges_um_tile_reach<float>(const float *, const float *, float *, int, int, int, int, SbTileReach,
                                                         hipStream_t);
template hipError_t sb_launch_edges_um_tile_reach<double>(const double *, const double *, double *, int, int, int, int, SbTileReach,
                                                          hipStream_t);
template hipError_t sb_launch_dist_um_tile_reach<float>(const float *, const float *, const float *, const float *, float *, int,
                                                        int, int, int, int, int, SbTileReach, float, uint64_t *, hipStream_t);
template hipError_t sb_launch_dist_um_tile_reach<double>(const double *, const double *, const double *, const double *, double *,
                                                         int, int, int, int, int, int, SbTileReach, double, uint64_t *, hipStream_t);
template hipError_t sb_launch_dist_um_tile_dirty<float>(const float *, const float *, const float *, float *, int, int, int, int,
                                                        int, int, SbTileReach, float, const uint64_t *, const unsigned char *,
                                                        hipStream_t);
template hipError_t sb_launch_dist_um_tile_dirty<double>(const double *, const double *, const double *, double *, int, int, int,
                                                         int, int, int, SbTileReach, double, const uint64_t *,
                                                         const unsigned char *, hipStream_t);
