// sb_coast_common.hpp -- what the coast setup's kernels share: sb_coast_kernels.hip (regular grids: k_edges, k_dist,
// k_dist_bits_small, k_dist_bits, k_dist_wide) and sb_um_coast_kernels.hip (the UM layout on curvilinear grids:
// k_edges_um, k_dist_um, k_dist_um_wide, k_edges_um_tile, k_dist_um_tile) and sb_ice_kernels.hip (a moving coast: k_edge_bits_delta[_band|_um|_um_tile]).
// ref: sobel.f90:19-193, UM/vn10.7/sea_breeze_diag.F90:386-601
// The Sobel block, the coast bit plane and its bit strings, the haversine term, the two forms of the epilogue (minimum a
// per sweep class -> distance -> sweep-time reset -> sign) and the per-target walk of a window that fits one word.
// Every piece is stated once; the kernels keep their staging, which is what differs between them.
#pragma once
#include <stdint.h>
#include "sb_device.hpp"
#include "sb_dist_plan.hpp"

// ---- the Sobel of a 256-column x EDGE_ROWS-row block ----
// A workgroup classifies the cells of the block and of the ring round it once (18 rows read for 16 written: 1.125 x the
// compulsory reads; with 8-row blocks the PMC passes showed 1.47 x) (two loads per cell instead of eighteen), keeps the
// land flags in LDS and takes the nine-point sums from there.  A policy P says what differs between the layouts:
//   size_t P::src(int x, int y)   field offset of the cell staged for (x, y), which may lie outside the grid: the boundary
//                                 mapping is applied to the staged cell, so a flag means exactly what the reference's
//                                 inner loop would have read at that offset
//   size_t P::dst(int x, int y)   field offset of the written cell (x, y)
//   int    P::land(T l, T c)      the land flag
//   bool   P::tail_by_index       which of two ways of writing "lanes past the ring stage row 0" the staging takes: the
//                                 same cells either way, but each layout keeps the form it was written with -- the other
//                                 one moves its kernel across an occupancy step (k_edges_um<double> 64 -> 67 VGPRs,
//                                 8 -> 7 waves per SIMD; k_edges<float> 79 -> 62, 6 -> 8)
#define EDGE_ROWS 16
#define EDGE_PITCH 264
#define EDGE_LDS ((EDGE_ROWS + 2) * EDGE_PITCH)

// sb_edges_each is the block without its store: emit(x, y, is_coast) is called for every cell of the block's rows inside
// the grid, by the threads whose column is (k_edge_bits_delta ballots the flags instead of writing a plane).
template <typename T, typename P, typename E>
__device__ __forceinline__ void sb_edges_each(const T *__restrict__ lsm, const T *__restrict__ ci, unsigned char *s_land,
                                              int nx, int ny, const P p, E emit) {
    const int x0 = blockIdx.x * 256, y0 = blockIdx.y * EDGE_ROWS;
    constexpr int NCELL = (EDGE_ROWS + 2) * 258, NIT = (NCELL + 255) / 256;
    T l[NIT], c[NIT];
#pragma unroll
    for (int j = 0; j < NIT; ++j) {                      // every load issued before the first is used
        const int i = threadIdx.x + 256 * j;
        int r, cc;                                       // (lanes past the ring: row 0)
        if constexpr (P::tail_by_index) { r = i < NCELL ? i / 258 : 0; cc = i - (i / 258) * 258; }
        else { r = i / 258; cc = i - r * 258; r = r < EDGE_ROWS + 2 ? r : 0; }
        const size_t o = p.src(x0 - 1 + cc, y0 - 1 + r);
        l[j] = lsm[o];
        c[j] = ci[o];
    }
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
        const int i = threadIdx.x + 256 * j, r = i / 258, cc = i - r * 258;
        const int land = p.land(l[j], c[j]);
        if (i < NCELL) s_land[r * EDGE_PITCH + cc] = (unsigned char)land;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= nx) return;
    // weight = reshape((/-1,-2,-1, 0,0,0, 1,2,1/),(3,3)) column-major: w(r,c) = (1,2,1)(r) * (-1,0,1)(c)
    // px += w(a+2, b+2)*m, py += w(b+2, a+2)*m     ref: sobel.f90:74-75, UM :420-427
    // -> px = sum_a (1,2,1)(a) * (m[a][2] - m[a][0]),  py = sum_b (1,2,1)(b) * (m[2][b] - m[0][b])
    int m[3][3];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) m[a + 1][b] = s_land[a * EDGE_PITCH + threadIdx.x + b];
#pragma unroll
    for (int r = 0; r < EDGE_ROWS; ++r) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            m[0][b] = m[1][b];
            m[1][b] = m[2][b];
            m[2][b] = s_land[(r + 2) * EDGE_PITCH + threadIdx.x + b];
        }
        const int px = (m[0][2] - m[0][0]) + 2 * (m[1][2] - m[1][0]) + (m[2][2] - m[2][0]);
        const int py = (m[2][0] - m[0][0]) + 2 * (m[2][1] - m[0][1]) + (m[2][2] - m[0][2]);
        const int y = y0 + r;
        if (y < ny) emit(x, y, !(px == 0 && py == 0));           // sqrt(px^2+py^2) == 0
    }
}

template <typename T, typename P>
__device__ __forceinline__ void sb_edges_block(const T *__restrict__ lsm, const T *__restrict__ ci, T *__restrict__ coast,
                                               unsigned char *s_land, int nx, int ny, const P p) {
    sb_edges_each(lsm, ci, s_land, nx, ny, p, [&](int x, int y, bool c) { coast[p.dst(x, y)] = c ? T(1) : T(0); });
}

// k_edges' layout: the boundary mapping of sb_map_cell (cyclic longitudes with the f2py flavour's column quirk, clamped
// latitudes; ref: sobel.f90:60-66, generic :340-352) and either flavour's land rule
template <typename T>
struct EdgesGrid {
    static constexpr bool tail_by_index = false;
    Geo g;
    int rule;
    __device__ __forceinline__ size_t src(int x, int y) const {
        int X, Y;
        sb_map_cell(g, x, y, X, Y);
        return (size_t)Y * g.nx + X;
    }
    __device__ __forceinline__ size_t dst(int x, int y) const { return (size_t)y * g.nx + x; }
    __device__ __forceinline__ int land(T l, T c) const {
        if (rule == 0) return (l + c > T(0.4)) ? 1 : 0;            // ref: sobel.f90:51,69
        if (c <= T(0.2)) return (l >= T(0.5)) ? 1 : 0;             // ref: generic :325-330
        return (l + c >= T(0.5)) ? 1 : 0;                          // ref: generic :332-336
    }
};

// The SOURCE rows of one latitude band in its ghost-celled frame (sb_band_ice_*: pitch ld = nx + 2h, interior at (h, h);
// source row y is frame row f0 + y, sb_band_rows): EdgesBand's rule -- SB_BND_GLOBAL seen from a band -- for the rows a
// distance window may find a coast cell in, the band's own and the k ghost rows on each cut side, so that a rank forms
// the coast bits of its ghost source rows itself instead of receiving them.  Longitude is cyclic by index arithmetic (the
// east-west ghost columns are never read); at a pole side (lo = 0 / hi = nys-1) the row clamps to the band's edge row and
// no ghost row is read; at a cut side (lo = -1 / hi = nys) the one frame row beyond the source rows is read, the (k+1)-th
// ghost row: the host holds k + 1 <= h there, so it lies inside the frame.  Rows further out are staged only for the
// unwritten rows of a ragged block and are held at that row.  dst: the whole path's scratch coast, which starts at
// (column 0, source row 0) with the frame's pitch (what sb_launch_dist_band is handed).
template <typename T>
struct EdgesBandSrc {
    static constexpr bool tail_by_index = false;
    int nx, nys, h, ld, f0, lo, hi, rule;
    __device__ __forceinline__ int cols() const { return nx; }           // the cells it forms edges of (k_edge_bits_delta)
    __device__ __forceinline__ int rows() const { return nys; }
    __device__ __forceinline__ size_t src(int x, int y) const {
        int X = x % nx;
        X = X < 0 ? X + nx : X;
        const int Y = y < lo ? lo : (y > hi ? hi : y);
        return (size_t)(f0 + Y) * ld + h + X;                    // (f0 + lo >= 0: f0 >= 1 wherever lo == -1)
    }
    __device__ __forceinline__ size_t dst(int x, int y) const { return (size_t)y * ld + x; }
    __device__ __forceinline__ int land(T l, T c) const { return EdgesGrid<T>{Geo{}, rule}.land(l, c); }
};

// k_edges_um's layout: the interior offset by (hi, hj) inside the ghost-celled field of NX x NY cells.  The ring cells are
// ghost cells of the caller; cells past the ring are clamped into the field (their flags are never read for a written
// cell).
template <typename T>
struct EdgesUm {
    static constexpr bool tail_by_index = true;
    int NX, NY, hi, hj;
    __device__ __forceinline__ int cols() const { return NX - 2 * hi; }  // the interior (k_edge_bits_delta)
    __device__ __forceinline__ int rows() const { return NY - 2 * hj; }
    __device__ __forceinline__ size_t src(int x, int y) const {
        int X = x + hi, Y = y + hj;
        X = X < NX ? X : NX - 1;
        Y = Y < NY ? Y : NY - 1;
        return (size_t)Y * NX + X;
    }
    __device__ __forceinline__ size_t dst(int x, int y) const { return (size_t)(y + hj) * NX + x + hi; }
    __device__ __forceinline__ int land(T l, T c) const {
        if (c <= T(0.2)) return (l >= T(0.5)) ? 1 : 0;            // ref: UM :390-396
        return (l + c >= T(0.5)) ? 1 : 0;                          // ref: UM :397-403
    }
};

// k_edges_um_tile's layout (one tile of a 2-D decomposition, sb_tile_get_edges_um_*): EdgesUm's rule on a written rectangle
// that is not the interior -- it takes in `ext` ghost columns / rows on every cut side -- so the pitch ld and the rows NY of
// the frame are stated apart from the rectangle's size (the kernel's nx, ny), and (ox, oy) is the frame cell of written cell
// (0, 0).  The host holds ox, oy >= 1: the ring cell (-1, -1) lies inside the frame; cells past the ring are clamped into it
// as EdgesUm clamps them.
template <typename T>
struct EdgesUmTile {
    static constexpr bool tail_by_index = true;
    int ld, NY, ox, oy;
    __device__ __forceinline__ size_t src(int x, int y) const {
        int X = x + ox, Y = y + oy;
        X = X < ld ? X : ld - 1;
        Y = Y < NY ? Y : NY - 1;
        return (size_t)Y * ld + X;
    }
    __device__ __forceinline__ size_t dst(int x, int y) const { return (size_t)(y + oy) * ld + x + ox; }
    __device__ __forceinline__ int land(T l, T c) const { return EdgesUm<T>{}.land(l, c); }
};
// ... and the same rule for k_edge_bits_delta's tile instance (sb_um_tile_ice_*), which asks its policy for the cells it
// forms edges of: the source rectangle of wx x wy cells, whose first cell is frame cell (ox, oy).  A type of its own, so
// that k_edges_um_tile's instance carries what it carried.
template <typename T>
struct EdgesUmTileSrc : EdgesUmTile<T> {
    int wx, wy;
    __device__ __forceinline__ int cols() const { return wx; }
    __device__ __forceinline__ int rows() const { return wy; }
};

// ---- the coast bit plane ----
// coast > 0 of an nx x ny field with row pitch ld whose first cell is at off0 (a regular grid: nx, 0; the interior of a
// ghost-celled UM field: nx + 2hi, hj (nx + 2hi) + hi), one 64-bit word per 64-cell segment of a row (a wave ballot;
// bits past nx are zero).  A launch of its own: the plane is complete before any distance is written.
#define COASTBITS_ROWS 8              // rows per workgroup of k_coastbits: eight loads in flight per thread
template <typename T>
__global__ __launch_bounds__(256) void k_coastbits(const T *__restrict__ coast, uint64_t *__restrict__ bits,
                                                   int nx, int ny, int nw, int ld, size_t off0) {
    const int x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * COASTBITS_ROWS;
    T v[COASTBITS_ROWS];
#pragma unroll
    for (int r = 0; r < COASTBITS_ROWS; ++r) {
        const int y = y0 + r < ny ? y0 + r : ny - 1;                 // (clamped: every load unconditional)
        v[r] = coast[off0 + (size_t)y * ld + (x < nx ? x : nx - 1)];
    }
#pragma unroll
    for (int r = 0; r < COASTBITS_ROWS; ++r) {
        const uint64_t w = __ballot(x < nx && v[r] > T(0));          // ref: sobel.f90:157, UM :551
        if ((threadIdx.x & 63) == 0 && (x >> 6) < nw && y0 + r < ny) bits[(size_t)(y0 + r) * nw + (x >> 6)] = w;
    }
}
template <typename T>
inline void sb_launch_coastbits(const T *coast, uint64_t *bits, int nx, int ny, int nw, int ld, size_t off0, hipStream_t st) {
    hipLaunchKernelGGL(k_coastbits<T>, dim3((nx + 255) / 256, (ny + COASTBITS_ROWS - 1) / COASTBITS_ROWS), dim3(256), 0, st,
                       coast, bits, nx, ny, nw, ld, off0);
}

// bits p .. p+l-1 (l <= 63, p+l <= nx) of a row of the plane
__device__ __forceinline__ uint64_t row_bits(const uint64_t *__restrict__ rw, int p, int l) {
    const int w = p >> 6, o = p & 63;
    uint64_t v = rw[w] >> o;
    if (o + l > 64) v |= rw[w + 1] << (64 - o);
    return v & ((1ull << l) - 1ull);
}
// 64 bits of a row from column p on, all of them inside the row (p >= 0, p + 64 <= nx)
__device__ __forceinline__ uint64_t row_word64(const uint64_t *__restrict__ rw, int p) {
    const int w = p >> 6, o = p & 63;
    uint64_t v = rw[w] >> o;
    if (o) v |= rw[w + 1] << (64 - o);
    return v;
}
// row_word64 from circular column p on (0 <= p < nx, nx >= 64): across the seam where need be
__device__ __forceinline__ uint64_t row_bits64(const uint64_t *__restrict__ rw, int p, int nx) {
    if (p + 64 <= nx) return row_word64(rw, p);
    const int l1 = nx - p;                                       // 1 .. 63 columns up to the seam, the rest from column 0
    return row_bits(rw, p, l1) | (row_bits(rw, 0, 64 - l1) << l1);
}
// row_bits64 for any nx >= 1: round the seam as often as it takes
__device__ __forceinline__ uint64_t circ_bits64(const uint64_t *__restrict__ rw, int p, int nx) {
    uint64_t v = 0;
    for (int f = 0; f < 64;) {
        const int l = nx - p < 64 - f ? nx - p : 64 - f;
        if (l == 64) return row_word64(rw, p);
        v |= row_bits(rw, p, l) << f;
        f += l;
        p = 0;
    }
    return v;
}
// row_word64 without a seam: p may be negative, and columns outside 0 .. 64*nw - 1 read as 0
__device__ __forceinline__ uint64_t um_row_bits64(const uint64_t *__restrict__ rw, int p, int nw) {
    const int w0 = p >= 0 ? p >> 6 : -((63 - p) >> 6), o = p - 64 * w0;      // floor division
    const uint64_t a = (w0 >= 0 && w0 < nw) ? rw[w0] : 0ull;
    const uint64_t b = (w0 + 1 >= 0 && w0 + 1 < nw) ? rw[w0 + 1] : 0ull;
    return o ? (a >> o) | (b << (64 - o)) : a;
}

// the highest / lowest set bit of a window word (WB: uint32_t or uint64_t; 64-bit shifts and bit scans cost two to
// three 32-bit ones), and the index of the lowest
template <typename WB>
__device__ __forceinline__ WB top_bit(WB x) {
    if constexpr (sizeof(WB) == 8) return x ? 1ull << (63 - __builtin_clzll(x)) : 0ull;
    else return x ? (WB)(1u << (31 - __builtin_clz((unsigned)x))) : (WB)0;
}
template <typename WB>
__device__ __forceinline__ WB low_bit(WB x) { return (WB)(x & ((WB)0 - x)); }
template <typename WB>
__device__ __forceinline__ int low_idx(WB x) {
    if constexpr (sizeof(WB) == 8) return __builtin_ctzll((uint64_t)x);
    else return __builtin_ctz((unsigned)x);
}

// ---- distances ----
template <typename T>
struct SbDist {
    static constexpr T R = T(6370.9989);                        // ref: sobel.f90:115
    static constexpr T big = T(12000.);                          // "unreached"
    static constexpr T none = T(4);                              // a <= 1: "no source in this class"
};

// a = sin^2(dphi/2) + cos(phi_s) cos(phi_t) sin^2(dlam/2), in the reference's order    ref: sobel.f90:176, UM :566
template <typename T>
__device__ __forceinline__ T sb_hav(T sp2, T cosp, T cost, T sl) { return sp2 + (cosp * (cost * (sl * sl))); }

template <typename T>
__device__ __forceinline__ T dist_of(T a) {                      // ref: sobel.f90:177, UM :567
    return (SbDist<T>::R * T(2)) * atan2(sqrt(a), sqrt(T(1) - a)) + T(0.5);
}
// atan2(sqrt(a), sqrt(1 - a)) = asin(sqrt(a)) = sqrt(a) (1 + a/6 + 3a^2/40 + 15a^3/336 + 105a^4/3456 + 945a^5/42240 + ...):
// for a < 2^-10 (distances below 400 km: every hit of a maxdist = 180 km window) five terms are exact to 1e-20
// relative, and the result is within two or three units in the last place of the library's atan2 of the two rounded
// roots (the tests hold 1e-12) -- for a fifth of the instructions.  a = 0 gives exactly 0.5 km either way.
template <typename T>
__device__ __forceinline__ T dist_small(T a) {
    const double ad = (double)a;
    double pl = __builtin_fma(ad, 945.0 / 42240.0, 105.0 / 3456.0);
    pl = __builtin_fma(pl, ad, 15.0 / 336.0);
    pl = __builtin_fma(pl, ad, 3.0 / 40.0);
    pl = __builtin_fma(pl, ad, 1.0 / 6.0);
    pl = __builtin_fma(pl, ad, 1.0);
    return (SbDist<T>::R * T(2)) * (T)(sqrt(ad) * pl) + T(0.5);
}

// The tail every kernel shares.  m_early, m_late: the smallest distance over the sources swept at or before the target
// (rows outer, columns inner) and after it.  The reference resets cdist to 12000 when its own sweep position is reached
// and the value so far exceeds 2*maxdist (ref: sobel.f90:188, UM :578); later sources may still lower it.
template <typename T>
__device__ __forceinline__ T sb_dist_reset_min(T m_early, T m_late, T maxdist) {
    if (m_early > T(2) * maxdist) m_early = SbDist<T>::big;
    return m_early < m_late ? m_early : m_late;
}
// ... and the sign: positive over land.  (Pointers, not references: *land is loaded only for a cell that is reached, and
// a reference would let the compiler load it for every cell.)    ref: sobel.f90:179-183, UM :568-574
template <typename T>
__device__ __forceinline__ void sb_dist_write(T *out, T m, const T *land) {
    if (m >= SbDist<T>::big) *out = SbDist<T>::big;
    else *out = (*land > T(0)) ? m : -m;
}

// The distance c = 2R atan2(sqrt(a), sqrt(1-a)) + 0.5 grows with a, so the minimum of c over a class of sources is c at the
// minimum of a: the bit-plane kernels keep min(a) per sweep class and take the distance once per class and cell instead
// of once per coast hit.  Two forms, which differ in the last places of an fp64 distance -- a kernel keeps its own:
// both distances, reset, minimum ...
template <typename T>
__device__ __forceinline__ T sb_dist_finish_both(T a_early, T a_late, T maxdist) {
    const T m_early = a_early < SbDist<T>::none ? dist_of(a_early) : SbDist<T>::big;
    const T m_late = a_late < SbDist<T>::none ? dist_of(a_late) : SbDist<T>::big;
    return sb_dist_reset_min(m_early, m_late, maxdist);
}
// ... or only the smaller a's distance -- one atan2 for the whole wave, or dist_small where the whole wave's a allow it --
// unless it is the early class's and the reset throws it away: then, rarely, the late class's as well.  Every lane of the
// wave that is still running calls it (ballots).
template <typename T>
__device__ __forceinline__ T sb_dist_finish_wave(T a_early, T a_late, T maxdist) {
    const T none = SbDist<T>::none, big = SbDist<T>::big;
    const bool late_wins = a_late < a_early;
    const T a_sel = late_wins ? a_late : a_early;
    T m = big;
    if (sizeof(T) == 8 && __ballot(a_sel < none && a_sel >= T(0x1p-10)) == 0) {      // wave-uniform
        if (a_sel < none) m = dist_small(a_sel);
    } else if (a_sel < none) m = dist_of(a_sel);
    const bool again = !late_wins && m > T(2) * maxdist;         // the reset, at sweep time
    if (__ballot(again) != 0) {                                  // wave-uniform
        const T m2 = a_late < none ? dist_of(a_late) : big;
        if (again) m = m2;
    }
    return m;
}

// ---- which rows a distance launch writes ----
// A distance kernel indexes SOURCE rows 0 .. ny-1: the rows of the bit plane and of phi, the rows a window may find a coast
// cell in (a window that reaches past them finds nothing there: the reference's latitude clamp adds no new sources).
// A policy G, the kernel's last argument, says which of them are TARGETS and where a cell of the fields lies:
//   DistWhole  the whole grid: every source row is a target, fields of pitch nx.  An empty type: the whole-grid instances
//              are the kernels they were before the policy came (same registers, same occupancy).
//   DistBand   one latitude band of a multi-GPU run in its ghost-celled frame: the source rows are the band's own and the
//              kwin ghost rows on each cut side (none beyond a pole: there the source range ends as the globe's does), the
//              targets r0 .. r1-1 are the band's own rows only -- ghost rows are never computed and thrown away -- and
//              the fields have the frame's pitch.  The host hands every field pointer over at (column 0, source row 0),
//              so a cell is y * ld + x and three scalars are all the kernels carry.
// Tiling is from column 0 with one target row per wave under either policy: a wave holds the same 64 targets in a band as
// on the globe, which is what sb_dist_finish_wave's ballots need for equal bits.
//   DistDirty  the whole grid of a stream whose coast moves (sb_diag_stream_ice_*): DistWhole, but a workgroup whose target
//              rows and 256-column tile carry no mark (one byte per (row, tile), sb_ice_plan.hpp) leaves before any staging
//              or barrier and the stored cdist of its cells stands.  skip(y0, rows, ny, tile) is asked first thing, with
//              workgroup-uniform arguments; the other two policies answer false and their instances are what they were.
//   DistBandDirty  a band whose coast moves (sb_band_ice_*): DistBand's targets and pitch, DistDirty's early exit -- the marks
//              are one byte per (OWN row, tile), so a target row y is row y - r0 of the plane.
// no mark on the target rows y0 .. y0+rows-1 below `lim` in the tile's column of a plane whose row 0 is target row `off`
__device__ __forceinline__ bool sb_marks_clear(const unsigned char *mark, int ntiles, int tile, int y0, int rows, int off, int lim) {
    unsigned m = 0;
    for (int r = 0; r < rows; ++r)
        if (y0 + r < lim) m |= mark[(size_t)(y0 + r - off) * ntiles + tile];
    return m == 0;
}
struct DistWhole {
    __device__ __forceinline__ int t0() const { return 0; }
    __device__ __forceinline__ int t1(int ny) const { return ny; }
    __device__ __forceinline__ size_t at(int x, int y, int nx) const { return (size_t)y * nx + x; }
    __device__ __forceinline__ bool skip(int, int, int, int) const { return false; }
};
struct DistBand {
    int r0, r1, ld;
    __device__ __forceinline__ int t0() const { return r0; }
    __device__ __forceinline__ int t1(int) const { return r1; }
    __device__ __forceinline__ size_t at(int x, int y, int) const { return (size_t)y * ld + x; }
    __device__ __forceinline__ bool skip(int, int, int, int) const { return false; }
};
struct DistDirty {
    const unsigned char *mark;
    int ntiles;
    __device__ __forceinline__ int t0() const { return 0; }
    __device__ __forceinline__ int t1(int ny) const { return ny; }
    __device__ __forceinline__ size_t at(int x, int y, int nx) const { return (size_t)y * nx + x; }
    __device__ __forceinline__ bool skip(int y0, int rows, int ny, int tile) const {
        return sb_marks_clear(mark, ntiles, tile, y0, rows, 0, ny);
    }
};
struct DistBandDirty {
    int r0, r1, ld;
    const unsigned char *mark;
    int ntiles;
    __device__ __forceinline__ int t0() const { return r0; }
    __device__ __forceinline__ int t1(int) const { return r1; }
    __device__ __forceinline__ size_t at(int x, int y, int) const { return (size_t)y * ld + x; }
    __device__ __forceinline__ bool skip(int y0, int rows, int, int tile) const {
        return sb_marks_clear(mark, ntiles, tile, y0, rows, r0, r1);
    }
};

// ---- what the cuts rest on (SB_CUT_*, sb_dist_plan.hpp; the host sets each only where it is exact) ----
//   * within one source row a = sp^2 + cos(phis) cos(phit) sin^2(dlam/2) grows with the longitude distance when the
//     longitudes step one way round the whole circle and the window spans less than half of it (CIRCLE), so of the hits
//     left of (or at) the target column only the nearest can be the minimum, and likewise on the right: two hits per row
//     instead of up to 2k+1.  On the target's own row the sweep order splits each side once more where the window crosses
//     the seam (xs <= xx is decided on wrapped indices, ref: sobel.f90:188), so up to four there;
//   * the same holds for a target whose window xx-k .. xx+k lies inside 0 .. nx-1 when the steps j -> j+1, j < nx-1 (not
//     the closing one) go one way and k of the largest stay below 170 degrees (INNER): inside such a window the angular
//     separation grows with the column distance and stays below 180 degrees, where sin^2(dlam/2) grows with it (the fold
//     of longitudes beyond 180 shifts dlam by 2 pi: sin^2 does not see it).  A regional grid's closing step of 300-odd
//     degrees forbids CIRCLE for every target although only the windows within k of the frame's edge cross it;
//   * a >= sp^2, which grows with the row distance when the latitudes step one way (ROWS): rows above the target are swept
//     before it, rows below after it, so a walk away from the target row can stop at the first row whose sp^2 is no
//     smaller than the class's minimum so far.
// NEAREST is CIRCLE and ROWS together, for the kernels whose window fits one word.  Without a cut every hit of every row
// is visited.

// the latitude factors of the 2k+1 source rows of target row yt (rows past the grid clamped: they add no sources, the
// walk never reads them) and cos(phi) of the target row: the same for every target of the row, once per workgroup
template <typename T>
__device__ __forceinline__ void sb_stage_lat(const T *__restrict__ phi, int ny, int yt, int k, int tx, T *s_sp2, T *s_cosp,
                                             T *s_cost) {
    const T phit = phi[yt];
    if (tx <= 2 * k) {
        int ys = yt + tx - k;
        ys = ys < 0 ? 0 : (ys >= ny ? ny - 1 : ys);
        const T phis = phi[ys];
        const T dphi = phis - phit;                              // phi1(i) - phi1(yy)
        const T sp = sin(dphi / T(2));
        s_sp2[tx] = sp * sp;
        s_cosp[tx] = cos(phis);
    } else if (tx == 2 * k + 1) *s_cost = cos(phit);
}

// The walk of target (xx, yy) over a window of 2k+1 <= 63 columns that fits one word WB.  k_dist_bits_small calls it;
// k_dist_bits carries the same statements written out in its body, because through this template its code comes out
// slower (2.0 % of get_dist at 2560 x 1920 fp64, measured: profiles/coast_common_ab.json) -- change both together.
//   rowmask    bit i: source row yy - k + i lies in the grid and holds a coast cell within reach of the wave (wave-uniform:
//              scalar bit scans)
//   start      the window's first column, circular; window bit b is column xx - k + b: bits 0 .. k lie left of or at the
//              target, the rest right of it; bits below k - xx and from nx - xx + k on have wrapped round the seam
//   word(ii)   the window of source row yy + ii, from wherever the kernel keeps its bits
//   sinl(b,xs) sin((l1 - l2) / 2) of window bit b, column xs.  fp64 takes sin(l1/2) cos(l2/2) - cos(l1/2) sin(l2/2) from
//              per-column tables (the host forms them with the folded longitudes): two products and a difference per hit
//              where the library sine took some eighty instructions -- two rounded products, no fma: for the target's own
//              column they are the same product and the difference is exactly zero, so a coast cell's own distance stays
//              exactly 0.5 km (SURVEY.md section 4's anchor).  The difference carries an absolute error of 1e-16, i.e.
//              <= 4e-13 relative in the distance at the finest spacing in use (0.07 degrees); the tests hold 1e-12.
//              fp32 keeps the sine: there the same identity would cost four digits.
// Leaves min(a) of the sources swept at or before the target in a_early, of those after it in a_late.
template <typename T, typename WB, typename WORD, typename SINL>
__device__ __forceinline__ void sb_dist_walk(uint64_t rowmask, int k, int nearest, int xx, int yy, int nx, int start,
                                             const T *s_sp2, const T *s_cosp, T cost, WORD word, SINL sinl,
                                             T &a_early, T &a_late) {
    const WB one = 1;
    const WB left = (WB)((WB)(one << k) << 1) - one;
    const WB wrapl = (k - xx > 0) ? (WB)(one << (k - xx)) - one : (WB)0;
    const WB wrapr = (nx - xx + k < (int)(8 * sizeof(WB))) ? (WB)((WB)~(WB)0 << (nx - xx + k)) : (WB)0;
    auto row = [&](int ii) {
        const int ys = yy + ii;
        WB wb = word(ii);
        if (!wb) return;
        if (nearest) {
            const WB wl = wb & left, wr = wb & (WB)~left;
            if (ii != 0) wb = top_bit<WB>(wl) | low_bit<WB>(wr);
            else wb = top_bit<WB>(wl & (WB)~wrapl) | top_bit<WB>(wl & wrapl) | low_bit<WB>(wr & (WB)~wrapr) | low_bit<WB>(wr & wrapr);
        }
        const T sp2 = s_sp2[ii + k], cosp = s_cosp[ii + k];
        while (wb) {
            const int b = low_idx<WB>(wb);
            wb &= (WB)(wb - one);
            int xs = start + b;
            if (xs >= nx) xs -= nx;
            const T sl = sinl(b, xs);
            const T a = sb_hav(sp2, cosp, cost, sl);
            const bool early = (ys < yy) || (ys == yy && xs <= xx);
            if (early) a_early = a < a_early ? a : a_early;
            else a_late = a < a_late ? a : a_late;
        }
    };
    if ((rowmask >> k) & 1) row(0);
    for (WB m = (WB)(rowmask & ((1ull << k) - 1ull)); m;) {      // rows above, nearest first
        const int idx = (int)(8 * sizeof(WB)) - 1 - (sizeof(WB) == 8 ? __builtin_clzll((uint64_t)m) : __builtin_clz((unsigned)m));
        m &= (WB)~(WB)(one << idx);
        if (nearest && !(s_sp2[idx] < a_early)) break;
        row(idx - k);
    }
    for (WB m = (WB)(rowmask >> (k + 1)); m;) {                  // rows below, nearest first
        const int d = low_idx<WB>(m) + 1;
        m &= (WB)(m - one);
        if (nearest && !(s_sp2[k + d] < a_late)) break;
        row(d);
    }
}
