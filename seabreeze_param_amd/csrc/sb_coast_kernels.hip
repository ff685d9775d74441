// sb_coast_kernels.hip -- coastline detection and signed coast distance on gfx950.
//
//   k_edges  binary 3x3 Sobel of the land mask          ref: sobel.f90:19-89,
//                                                        generic/sea_breeze_diag.f90:273-373
//   k_dist   signed haversine distance to the nearest coast cell, as a GATHER: each
//            target cell scans its own window for coast cells.  The reference is a
//            racy scatter over coast cells (ref: sobel.f90:152-191);
//            the gather keeps its results, including the sweep-order reset of :188,
//            by tracking the minimum over sources swept before and after the target.
//            k_dist itself (byte probes in LDS) is left with k <= 31 on grids narrower than the
//            window; every other call takes the bit-plane kernels: k_dist_bits[_small] for
//            k <= 31, k_dist_wide for 32 <= k <= SB_DIST_MAX_WINDOW (71 and 115 times faster than
//            k_dist at k = 40 and 100 on 2560 x 1920).
// One latitude band of a multi-GPU run in its ghost-celled frame takes the same kernels: k_edges_band is the Sobel block
// over the policy EdgesBand, and every distance kernel carries a target policy (DistWhole / DistBand, sb_coast_common.hpp)
// that says which of its source rows it writes and with which pitch -- a template argument, so the whole-grid instances
// are what they were.  DistDirty is the third policy: the whole grid of a stream whose coast moves with the sea ice, where
// a workgroup without a mark on its rows and tile leaves at once (sb_launch_dist_dirty; sb_ice_kernels.hip, sb_ice_plan.hpp);
// DistBandDirty the fourth: the same for one band (sb_launch_dist_band_dirty, sb_band_ice_*).
// Which kernel runs, and what it may leave out, is decided in sb_dist_plan.hpp; what the kernels share with the UM
// layout's (the Sobel block, the bit plane, the epilogues, the one-word walk, why each cut is exact) is in
// sb_coast_common.hpp.
#include "../../include/seabreeze_hip.h"
#include "sb_device.hpp"
#include "sb_launch.hpp"
#include "sb_coast_common.hpp"

// (EdgesGrid, k_edges' layout and either flavour's land rule: sb_coast_common.hpp -- the band's moving coast takes its
// land rule from there too)

// One latitude band of the global grid in its ghost-celled frame (the band step's layout: pitch nx + 2h, interior at
// (h, h)): EdgesGrid's SB_BND_GLOBAL rule seen from a band.  Longitude is cyclic by index arithmetic (the east-west ghost
// columns are never read); at a pole side the row clamps to the band's edge row (the ghost rows there are never read);
// at a cut side the one ghost row next to the interior is read as the neighbour band's edge row.  Rows further out are
// staged only for the unwritten rows of a ragged block: they are held at that ghost row, inside the frame.
template <typename T>
struct EdgesBand {
    static constexpr bool tail_by_index = false;
    int nx, ny, h, ld, south, north, rule;
    __device__ __forceinline__ size_t src(int x, int y) const {
        int X = x % nx;
        X = X < 0 ? X + nx : X;
        const int Y = y < 0 ? (south ? 0 : -1) : (y >= ny ? (north ? ny - 1 : ny) : y);
        return (size_t)(Y + h) * ld + h + X;
    }
    __device__ __forceinline__ size_t dst(int x, int y) const { return (size_t)(y + h) * ld + h + x; }
    __device__ __forceinline__ int land(T l, T c) const { return EdgesGrid<T>{Geo{}, rule}.land(l, c); }
};

template <typename T>
__global__ __launch_bounds__(256) void k_edges(const T *__restrict__ lsm, const T *__restrict__ ci,
                                               T *__restrict__ coast, Geo g, int rule) {
    __shared__ unsigned char s_land[EDGE_LDS];
    sb_edges_block(lsm, ci, coast, s_land, g.nx, g.ny, EdgesGrid<T>{g, rule});
}

template <typename T>
__global__ __launch_bounds__(256) void k_edges_band(const T *__restrict__ lsm, const T *__restrict__ ci,
                                                    T *__restrict__ coast, EdgesBand<T> p) {
    __shared__ unsigned char s_land[EDGE_LDS];
    sb_edges_block(lsm, ci, coast, s_land, p.nx, p.ny, p);
}


// Every distance kernel takes a target policy G (DistWhole, DistBand: sb_coast_common.hpp) as its last argument: ny counts
// the SOURCE rows (coast or its bit plane, phi), G says which of them are targets and where a cell of coast (k_dist),
// mask and cdist lies.
template <typename T, typename G>
__global__ __launch_bounds__(256) void k_dist(const T *__restrict__ coast, const T *__restrict__ mask,
                                              const T *__restrict__ phi, const T *__restrict__ lamf,
                                              T *__restrict__ cdist, int nx, int ny, int k, T maxdist, const G g) {
    extern __shared__ unsigned char sflag[];   // (64+2k) x (SB_DIST_TY+2k) coast flags
    const int W = 64 + 2 * k, HT = SB_DIST_TY + 2 * k;
    const int x0 = blockIdx.x * 64, y0 = g.t0() + blockIdx.y * SB_DIST_TY;
    for (int i = threadIdx.x; i < W * HT; i += 256) {
        const int r = i / W, c = i - r * W;
        const int ys = y0 - k + r;
        int xs = (x0 - k + c) % nx;
        if (xs < 0) xs += nx;
        unsigned char f = 0;
        if (ys >= 0 && ys < ny) f = coast[g.at(xs, ys, nx)] > T(0) ? 1 : 0;
        sflag[i] = f;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int xx = x0 + lx, yy = y0 + ly;
    if (xx >= nx || yy >= g.t1(ny)) return;

    const T big = SbDist<T>::big;
    const T phit = phi[yy], lamt = lamf[xx];
    const T cost = cos(phit);
    T m_early = big, m_late = big;
    for (int ii = -k; ii <= k; ++ii) {
        const int ys = yy + ii;
        if (ys < 0 || ys >= ny) continue;      // clamped rows add no new sources
        const unsigned char *row = &sflag[(ly + k + ii) * W + lx];   // column offset c = lx + k - jj
        for (int jj = -k; jj <= k; ++jj) {
            if (!row[k - jj]) continue;
            int xs = (xx - jj) % nx;
            if (xs < 0) xs += nx;
            const T phis = phi[ys];
            const T dphi = phis - phit;                          // phi1(i) - phi1(yy)
            const T dlam = lamf[xs] - lamt;                      // l1 - l2
            const T sp = sin(dphi / T(2)), sl = sin(dlam / T(2));
            const T c = dist_of(sb_hav(sp * sp, cos(phis), cost, sl));
            const bool early = (ys < yy) || (ys == yy && xs <= xx);
            if (early) m_early = c < m_early ? c : m_early;
            else m_late = c < m_late ? c : m_late;
        }
    }
    // (the minimum over distances, not over a: one distance per hit)
    const size_t o = g.at(xx, yy, nx);
    sb_dist_write(cdist + o, sb_dist_reset_min(m_early, m_late, maxdist), mask + o);
}

// ------------------------------------------------------------------------------------
// Bit-plane form of k_dist for windows of at most 63 columns (k <= 31, every BASELINE
// grid): k_coastbits packs coast > 0 into one 64-bit word per 64-cell longitude segment
// (a wave ballot); k_dist_bits pulls the (2k+1)-column window of each source row out of at
// most four words and visits set bits only.  Nine targets in ten have an empty window and
// cost a few hundred instructions instead of (2k+1)^2 byte probes.  min(a) per sweep class and
// the cuts `nearest` stands for (SB_CUT_NEAREST): sb_coast_common.hpp.
// Same arithmetic per visited hit as k_dist, same early/late bookkeeping.
// ------------------------------------------------------------------------------------

// k_dist_bits as rounds 1-3 had it (every word and table entry from global memory, per target and row): kept for grids
// narrower than 2k + 1 + 256 columns, where the staged reach of a workgroup would wrap round the seam more than once
template <typename T, typename G>
__global__ __launch_bounds__(256) void k_dist_bits_small(const uint64_t *__restrict__ bits, const T *__restrict__ mask,
                                                   const T *__restrict__ phi, const T *__restrict__ lamf,
                                                   const T *__restrict__ shl, const T *__restrict__ chl,
                                                   T *__restrict__ cdist, int nx, int ny, int nw, int k,
                                                   T maxdist, int nearest, const G g) {
    __shared__ T s_sp2[64], s_cosp[64], s_cost;
    const int xx = blockIdx.x * 256 + threadIdx.x, yy = g.t0() + blockIdx.y;
    if (g.skip(yy, 1, ny, (int)blockIdx.x)) return;
    const T big = SbDist<T>::big;
    // the row mask of k_dist_bits, but a wave whose reach crosses the seam keeps every row
    uint64_t rowmask;
    {
        const int lane = threadIdx.x & 63, wx0 = blockIdx.x * 256 + ((int)threadIdx.x & ~63);
        const bool seam = wx0 - k < 0 || wx0 + 63 + k >= nx;
        const int ys = yy + lane - k;
        uint64_t any = 0;
        if (lane <= 2 * k && ys >= 0 && ys < ny) {
            if (seam) any = 1;
            else
                for (int w = (wx0 - k) >> 6; w <= (wx0 + 63 + k) >> 6; ++w) any |= bits[(size_t)ys * nw + w];
        }
        rowmask = __ballot(any != 0);
    }
    // no coast cell within reach of any of the 256 targets: "unreached", before any trigonometry
    if (!__syncthreads_or(rowmask != 0 ? 1 : 0)) {
        if (xx < nx) cdist[g.at(xx, yy, nx)] = big;
        return;
    }
    sb_stage_lat(phi, ny, yy, k, (int)threadIdx.x, s_sp2, s_cosp, &s_cost);
    __syncthreads();
    if (xx >= nx) return;
    if (rowmask == 0) {                                          // wave-uniform: none of this wave's targets is reached
        cdist[g.at(xx, yy, nx)] = big;
        return;
    }
    const T lamt = lamf[xx];
    T sht = T(0), cht = T(0);
    if constexpr (sizeof(T) == 8) { sht = shl[xx]; cht = chl[xx]; }
    const int L = 2 * k + 1;
    int start = (xx - k) % nx;                                   // first window column, circular
    if (start < 0) start += nx;
    const int len1 = L < nx - start ? L : nx - start;
    T a_early = SbDist<T>::none, a_late = SbDist<T>::none;
    sb_dist_walk<T, uint64_t>(
        rowmask, k, nearest, xx, yy, nx, start, s_sp2, s_cosp, s_cost,
        [&](int ii) {
            const uint64_t *rw = bits + (size_t)(yy + ii) * nw;
            uint64_t wb = row_bits(rw, start, len1);
            if (len1 < L) wb |= row_bits(rw, 0, L - len1) << len1;
            return wb;
        },
        [&](int, int xs) -> T {
            if constexpr (sizeof(T) == 8) return shl[xs] * cht - chl[xs] * sht;
            else return sin((lamf[xs] - lamt) / T(2));           // l1 - l2
        },
        a_early, a_late);
    const size_t o = g.at(xx, yy, nx);
    sb_dist_write(cdist + o, sb_dist_finish_both(a_early, a_late, maxdist), mask + o);
}

#define DIST_SPAN (256 + 2 * 31)                                 // columns a workgroup's 256 targets can reach (k <= 31)
#define DIST_WORDS 5                                             // ... in 64-bit words

#ifndef DIST_ROWS
#define DIST_ROWS 2                                               // target rows per workgroup (256 x 2 threads)
#endif
// WB: the word a target's window (2k+1 columns) and the wave's row mask (2k+1 rows) are held in: 32 bits for k <= 15 (the
// N1280 grid and coarser: the walk is bound by vector-integer issue, and 64-bit shifts and bit scans cost two to three
// 32-bit ones), 64 bits beyond
template <typename T, typename WB, typename G>
__global__ __launch_bounds__(256 * DIST_ROWS) void k_dist_bits(const uint64_t *__restrict__ bits, const T *__restrict__ mask,
                                                   const T *__restrict__ phi, const T *__restrict__ lamf,
                                                   const T *__restrict__ shl, const T *__restrict__ chl,
                                                   T *__restrict__ cdist, int nx, int ny, int nw, int k,
                                                   T maxdist, int nearest, const G g) {
    __shared__ T s_sp2a[DIST_ROWS][64], s_cospa[DIST_ROWS][64], s_costa[DIST_ROWS];
    // everything the 512 targets of this workgroup read more than once, staged ONCE (round 4: the per-target walk used to
    // fetch two words of the bit plane and two table entries per hit from global memory, row after row -- a chain of
    // dependent L2 round trips, 50 us per wave): the coast bits of the source rows over the columns in reach, as one
    // bit string per row that starts at column x0 - k (circular: the seam is dealt with here, once), and the longitude
    // tables over the same columns
    __shared__ uint64_t s_bw[63 + DIST_ROWS - 1][DIST_WORDS];
    __shared__ T s_ta[DIST_SPAN], s_tb[DIST_SPAN];               // fp64: sin, cos of half the folded longitude; fp32: the folded longitude
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 256 + tx;
    const int x0 = blockIdx.x * 256, y0 = g.t0() + blockIdx.y * DIST_ROWS;
    const int xx = x0 + tx, yy = y0 + ty;
    if (g.skip(y0, DIST_ROWS, ny, (int)blockIdx.x)) return;
    const bool rowok = yy < g.t1(ny);                            // (an odd number of rows: the last workgroup's second row)
    const T big = SbDist<T>::big;
    // Which of the 2k+1 source rows hold any coast cell within reach of this wave's 64 targets?  Lane i ORs the
    // (at most three) words of row yy - k + i that cover columns x0 - k .. x0 + 63 + k; the ballot is a row mask in
    // scalar registers, and rows without a bit are skipped by the whole wave.  Four targets in five see no coast
    // at all and end here after one load round.
    uint64_t rowmask;
    {
        const int lane = tx & 63, wx0 = x0 + (tx & ~63);
        const int ys = yy + lane - k;
        uint64_t any = 0;
        if (rowok && lane <= 2 * k && ys >= 0 && ys < ny) {
            // (whole words: an over-estimate of the reach, never an under-estimate; a reach that crosses the seam is two
            // pieces -- round 3 kept every row for such a wave, and one workgroup column in five of the N1280 grid did the
            // whole walk over empty windows)
            const uint64_t *rw = bits + (size_t)ys * nw;
            int lo = wx0 - k, hi = wx0 + 63 + k;
            hi = hi < nx + lo ? hi : nx + lo - 1;                // (at most once round the circle)
            if (lo < 0) {
                for (int w = (lo + nx) >> 6; w < nw; ++w) any |= rw[w];
                lo = 0;
            }
            if (hi >= nx) {
                for (int w = 0; w <= (hi - nx) >> 6; ++w) any |= rw[w];
                hi = nx - 1;
            }
            for (int w = lo >> 6; w <= hi >> 6; ++w) any |= rw[w];
        }
        rowmask = __ballot(any != 0);
    }
    // Four workgroups in five have no coast cell within reach of any of their targets: they write the "unreached"
    // value and leave before any trigonometry.
    if (!__syncthreads_or(rowmask != 0 ? 1 : 0)) {
        if (xx < nx && rowok) cdist[g.at(xx, yy, nx)] = big;
        return;
    }
    const int L = 2 * k + 1;
    int c0 = (x0 - k) % nx;                                      // first column in reach, circular
    if (c0 < 0) c0 += nx;
    // ---- staging ----
    sb_stage_lat(phi, ny, rowok ? yy : ny - 1, k, tx, s_sp2a[ty], s_cospa[ty], &s_costa[ty]);
    for (int i = tid; i < (L + DIST_ROWS - 1) * DIST_WORDS; i += 256 * DIST_ROWS) {
        const int r = i / DIST_WORDS, j = i - r * DIST_WORDS;
        const int ys = y0 + r - k;
        uint64_t v = 0;
        if (ys >= 0 && ys < ny) {
            int p = c0 + 64 * j;
            p -= p >= nx ? nx : 0;                               // (nx >= 2k + 1 + 256: the launcher's condition for this kernel)
            p -= p >= nx ? nx : 0;
            v = row_bits64(bits + (size_t)ys * nw, p, nx);
        }
        s_bw[r][j] = v;
    }
    for (int i = tid; i < 256 + 2 * k; i += 256 * DIST_ROWS) {
        int xs = c0 + i;
        xs -= xs >= nx ? nx : 0;
        xs -= xs >= nx ? nx : 0;
        if constexpr (sizeof(T) == 8) { s_ta[i] = shl[xs]; s_tb[i] = chl[xs]; }
        else s_ta[i] = lamf[xs];
    }
    __syncthreads();
    if (xx >= nx || !rowok) return;
    if (rowmask == 0) {                                          // wave-uniform: none of this wave's targets is reached
        cdist[g.at(xx, yy, nx)] = big;
        return;
    }
    const T *s_sp2 = s_sp2a[ty], *s_cosp = s_cospa[ty];
    const T s_cost = s_costa[ty];
    const uint64_t (*s_bwt)[DIST_WORDS] = s_bw + ty;             // row ii of this target: s_bwt[ii + k]
    // sb_dist_walk's walk (sb_coast_common.hpp: the window's bits, the sine of the longitude term, the stops), written out
    // here: through the function template this kernel's code comes out 2 to 9 instructions longer and get_dist with the
    // automatic window 2.0 % slower at 2560 x 1920 fp64, 1.2 % at 5120 x 3840 fp32 (profiles/coast_common_ab.json)
    const T cost = s_cost;
    const int t = tx;                                            // this target's window starts at bit t of the rows' bit strings
    const T ta_t = s_ta[t + k], tb_t = sizeof(T) == 8 ? s_tb[t + k] : T(0);
    int start = c0 + t;                                          // first window column, circular
    start -= start >= nx ? nx : 0;
    const WB one = 1;
    const WB left = (WB)((WB)(one << k) << 1) - one;
    const WB wrapl = (k - xx > 0) ? (WB)(one << (k - xx)) - one : (WB)0;
    const WB wrapr = (nx - xx + k < (int)(8 * sizeof(WB))) ? (WB)((WB)~(WB)0 << (nx - xx + k)) : (WB)0;
    const WB lmask = (WB)(((uint64_t)1 << L) - 1ull);
    const int tw = t >> 6, to = t & 63;
    T a_early = SbDist<T>::none, a_late = SbDist<T>::none;
    auto sinl = [&](int b, int) -> T {
        if constexpr (sizeof(T) == 8) return s_ta[t + b] * tb_t - s_tb[t + b] * ta_t;
        else return sin((s_ta[t + b] - ta_t) / T(2));
    };
    auto row = [&](int ii) {
        const int ys = yy + ii;
        uint64_t w64 = s_bwt[ii + k][tw] >> to;
        if (to) w64 |= s_bwt[ii + k][tw + 1] << (64 - to);       // (tw + 1 <= 4)
        WB wb = (WB)w64 & lmask;
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
    const size_t o = g.at(xx, yy, nx);
    sb_dist_write(cdist + o, sb_dist_finish_wave(a_early, a_late, maxdist), mask + o);
}

// ------------------------------------------------------------------------------------
// k_dist_wide: k_dist_bits for windows of 32 .. SB_DIST_MAX_WINDOW cells each way (km-scale regional grids: 113 cells
// at 0.0135 degrees).  A target's window of 2k+1 <= 511 columns no longer fits one word, and the 2k+1 source rows no
// longer fit LDS at once, so
//   * a source row's coast bits over the columns x0-k .. x0+255+k in reach of the workgroup are a bit string of up to
//     WIDE_WORDS words (bit b is column (x0 - k + b) mod nx: the seam, and a grid narrower than the reach, are dealt with
//     in the staging); the window of target t is bits t .. t+2k of it, its own column bit t+k;
//   * the source rows are staged in passes, nearest to the target rows first: pass j holds the WIDE_A rows from
//     WIDE_A*j + 1 above the workgroup's first target row, as many below its last, and (pass 0) the target rows:
//     64 slots, one lane of a wave each, so a wave's row mask is one ballot per pass;
//   * the nearest hit at or left of the own column, and right of it, is found by scanning words outwards from bit t+k.
// Everything else is k_dist_bits': rows without a coast bit in reach of the wave are skipped by the wave, a workgroup
// with nothing in reach leaves before any trigonometry, min(a) per sweep class and one distance per cell, dist_small,
// the exact zero of the own column's difference of products.
//
// `cuts` (SB_CUT_CIRCLE, _INNER, _ROWS: sb_dist_plan.hpp, sb_coast_common.hpp) says what may be left out, one by one.
// Windows that may not be cut visit every hit; so does the own row of a window across the seam (xs <= xx is decided
// on wrapped indices there, ref: sobel.f90:188).  With 2k+1 >= nx the window is the nx columns from xx-k on: every
// column once (the reference's loop meets some twice, which changes no minimum).
// ------------------------------------------------------------------------------------
#define WIDE_ROWS 2                                              // target rows per workgroup (256 x 2 threads)
#define WIDE_A 31                                                // source rows above, and below, per pass
#define WIDE_SLOTS (2 * WIDE_A + WIDE_ROWS)                      // rows resident in LDS: one per lane of a wave
#define WIDE_SPAN (256 + 2 * SB_DIST_MAX_WINDOW)                 // columns a workgroup's 256 targets can reach
#define WIDE_WORDS ((WIDE_SPAN + 63) / 64)
static_assert(WIDE_SLOTS == 64 && WIDE_ROWS == 2, "k_dist_wide: a slot per lane, and the walk names both target rows");

template <typename T, typename G>
__global__ __launch_bounds__(256 * WIDE_ROWS) void k_dist_wide(const uint64_t *__restrict__ bits, const T *__restrict__ mask,
                                                   const T *__restrict__ phi, const T *__restrict__ lamf,
                                                   const T *__restrict__ shl, const T *__restrict__ chl,
                                                   T *__restrict__ cdist, int nx, int ny, int nw, int k,
                                                   T maxdist, int cuts, const G g) {
    __shared__ uint64_t s_bw[WIDE_SLOTS][WIDE_WORDS];
    __shared__ T s_ta[WIDE_SPAN], s_tb[sizeof(T) == 8 ? WIDE_SPAN : 1];   // fp64: sin, cos of half the folded longitude; fp32: the folded longitude
    __shared__ T s_sp2[WIDE_ROWS][WIDE_SLOTS], s_cosp[WIDE_SLOTS], s_cost[WIDE_ROWS];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 256 + tx;
    const int x0 = blockIdx.x * 256, y0 = g.t0() + blockIdx.y * WIDE_ROWS;
    const int xx = x0 + tx, yy = y0 + ty;
    if (g.skip(y0, WIDE_ROWS, ny, (int)blockIdx.x)) return;
    const bool active = xx < nx && yy < g.t1(ny);                // (every thread stays for the barriers)
    const int span = 256 + 2 * k, nws = (span + 63) >> 6;
    int c0 = (x0 - k) % nx;                                      // first column in reach, circular
    if (c0 < 0) c0 += nx;
    const int t = tx, P = t + k;                                 // this target's window starts at bit t; its own column
    const int hi = t + (2 * k + 1 < nx ? 2 * k + 1 : nx) - 1;    // ... and ends at bit hi
    const bool inside = xx - k >= 0 && xx + k <= nx - 1;
    const bool colcut = (cuts & SB_CUT_CIRCLE) || ((cuts & SB_CUT_INNER) && inside);
    const bool rowcut = (cuts & SB_CUT_ROWS) != 0;
    // slot s of pass j: the row of the plane it holds (may lie outside 0 .. ny-1), and its distance from the nearer
    // target row
    auto slot_row = [&](int s, int j) {
        if (s < WIDE_A) return y0 - 1 - WIDE_A * j - s;
        if (s < 2 * WIDE_A) return y0 + WIDE_ROWS + WIDE_A * j + (s - WIDE_A);
        return j == 0 ? y0 + (s - 2 * WIDE_A) : -1;
    };
    auto slot_dist = [&](int s, int j) { return s < 2 * WIDE_A ? 1 + WIDE_A * j + (s < WIDE_A ? s : s - WIDE_A) : 0; };

    T a_early = SbDist<T>::none, a_late = SbDist<T>::none;
    T ta_t = T(0), tb_t = T(0), cost = T(0);
    bool stop_up = !active, stop_dn = !active;                   // this target's sweep class cannot improve any more
    bool tables = false;                                         // (workgroup-uniform)
    const int npass = (k - 1) / WIDE_A + 1;
    for (int j = 0; j < npass; ++j) {
        // (the barrier between the walk of the pass before and this pass's staging; with the row cut most workgroups
        // near a coast are done after pass 0)
        if (j > 0 && __syncthreads_and(stop_up && stop_dn ? 1 : 0)) break;
        int anyv = 0;
        for (int i = tid; i < WIDE_SLOTS * WIDE_WORDS; i += 256 * WIDE_ROWS) {
            const int s = i / WIDE_WORDS, w = i - s * WIDE_WORDS;
            const int ys = slot_row(s, j);
            uint64_t v = 0;
            if (w < nws && ys >= 0 && ys < ny && slot_dist(s, j) <= k)       // clamped rows add no new sources
                v = circ_bits64(bits + (size_t)ys * nw, (c0 + 64 * w) % nx, nx);
            s_bw[s][w] = v;
            anyv |= v != 0 ? 1 : 0;
        }
        if (!__syncthreads_or(anyv)) continue;                   // no coast cell in this pass's rows within reach of the workgroup
        // the latitude factors of this pass's rows, per target row; with the first pass that holds a coast cell also
        // the longitude tables over the reach -- a workgroup with nothing in reach never gets here
        if (tid < WIDE_ROWS * WIDE_SLOTS) {
            const int r = tid / WIDE_SLOTS, s = tid - r * WIDE_SLOTS;
            int ys = slot_row(s, j);
            ys = ys < 0 ? 0 : (ys >= ny ? ny - 1 : ys);
            const T phit = phi[y0 + r < ny ? y0 + r : ny - 1], phis = phi[ys];
            const T dphi = phis - phit;                          // phi1(i) - phi1(yy)
            const T sp = sin(dphi / T(2));
            s_sp2[r][s] = sp * sp;
            if (r == 0) s_cosp[s] = cos(phis);
        }
        if (!tables) {
            if (tid >= 256 && tid < 256 + WIDE_ROWS) s_cost[tid - 256] = cos(phi[y0 + tid - 256 < ny ? y0 + tid - 256 : ny - 1]);
            for (int i = tid; i < span; i += 256 * WIDE_ROWS) {
                const int xs = (c0 + i) % nx;
                if constexpr (sizeof(T) == 8) { s_ta[i] = shl[xs]; s_tb[i] = chl[xs]; }
                else s_ta[i] = lamf[xs];
            }
        }
        __syncthreads();
        if (!tables) {
            tables = true;
            ta_t = s_ta[P];
            if constexpr (sizeof(T) == 8) tb_t = s_tb[P];
            cost = s_cost[ty];
        }
        // Which of the 64 resident rows hold any coast cell within reach of this wave's 64 targets (bits 64 wv ..
        // 64 wv + 63 + 2k of the strings; whole words: never an under-estimate)?  Lane i answers for slot i.
        uint64_t rowmask;
        {
            const int lane = tx & 63, wv = tx >> 6;
            uint64_t any = 0;
            for (int w = wv; w <= (64 * wv + 63 + 2 * k) >> 6; ++w) any |= s_bw[lane][w];
            rowmask = __ballot(any != 0);
        }
        if (!active || rowmask == 0) continue;                   // (the next barrier is the loop's first statement)

        auto row = [&](int s, int ii) {                          // slot s holds row yy + ii
            const uint64_t *w = s_bw[s];
            const T sp2 = s_sp2[ty][s], cosp = s_cosp[s];
            auto visit = [&](int q, bool early) {                // the hit at bit q of the string
                T sl;
                // fp64: sin((l1 - l2) / 2) = sin(l1/2) cos(l2/2) - cos(l1/2) sin(l2/2) from the per-column tables, as in
                // k_dist_bits (two rounded products, no fma: for the own column, and for a copy of it a whole turn
                // away, they are the same product and the difference is exactly zero).  The difference carries an
                // absolute error of about 1e-16 whatever the spacing, so the distance one of 2R cos(phi) 1e-16 <= 1.3e-12
                // km: within 1e-12 of max(|distance|, 1 km), the tests' rule, although not of a distance well below
                // 1 km were there one (the smallest is 0.5).  Measured at 0.0135 degrees, 68-71 N: 1.3e-13.
                if constexpr (sizeof(T) == 8) sl = s_ta[q] * tb_t - s_tb[q] * ta_t;
                else {
                    const T dlam = s_ta[q] - ta_t;               // l1 - l2
                    sl = sin(dlam / T(2));
                }
                const T a = sb_hav(sp2, cosp, cost, sl);
                if (early) a_early = a < a_early ? a : a_early;
                else a_late = a < a_late ? a : a_late;
            };
            if (colcut && (ii != 0 || inside)) {
                // at or left of the own column: downwards from its word to the window's first
                int wi = P >> 6;
                uint64_t v = w[wi] & (~0ull >> (63 - (P & 63)));
                while (!v && wi > (t >> 6)) v = w[--wi];
                if (v) {
                    const int q = 64 * wi + 63 - __builtin_clzll(v);
                    if (q >= t) visit(q, ii <= 0);
                }
                // right of it: upwards to the window's last word
                wi = (P + 1) >> 6;
                v = w[wi] & (~0ull << ((P + 1) & 63));
                while (!v && wi < (hi >> 6)) v = w[++wi];
                if (v) {
                    const int q = 64 * wi + __builtin_ctzll(v);
                    if (q <= hi) visit(q, ii < 0);
                }
            } else {
                for (int wi = t >> 6; wi <= hi >> 6; ++wi) {
                    uint64_t v = w[wi];
                    if (wi == t >> 6) v &= ~0ull << (t & 63);
                    if (wi == hi >> 6) v &= ~0ull >> (63 - (hi & 63));
                    while (v) {
                        const int q = 64 * wi + __builtin_ctzll(v);
                        v &= v - 1;
                        bool early = ii < 0;
                        if (ii == 0) early = (c0 + q) % nx <= xx;            // xs <= xx on wrapped indices
                        visit(q, early);
                    }
                }
            }
        };
        // Rows above the target are swept before it, rows below after it; within a class nearest first, over the passes
        // too, so the row cut may end a class for good.  Only rows whose bit is set in the wave's row mask are visited
        // (scalar bit scans: the mask is wave-uniform).
        if (j == 0) {
            if ((rowmask >> (2 * WIDE_A + ty)) & 1) row(2 * WIDE_A + ty, 0);
            if (ty == 1 && ((rowmask >> (2 * WIDE_A)) & 1)) {                 // the other target row: one above ...
                if (rowcut && !(s_sp2[ty][2 * WIDE_A] < a_early)) stop_up = true;
                else row(2 * WIDE_A, -1);
            }
            if (ty == 0 && ((rowmask >> (2 * WIDE_A + 1)) & 1)) {             // ... or one below
                if (rowcut && !(s_sp2[ty][2 * WIDE_A + 1] < a_late)) stop_dn = true;
                else row(2 * WIDE_A + 1, 1);
            }
        }
        if (!stop_up)
            for (uint32_t m = (uint32_t)rowmask & ((1u << WIDE_A) - 1u); m; m &= m - 1) {
                const int s = __builtin_ctz(m), d = ty + 1 + WIDE_A * j + s;
                if (d > k) break;                                // wave-uniform
                if (rowcut && !(s_sp2[ty][s] < a_early)) { stop_up = true; break; }
                row(s, -d);
            }
        if (!stop_dn)
            for (uint32_t m = (uint32_t)(rowmask >> WIDE_A) & ((1u << WIDE_A) - 1u); m; m &= m - 1) {
                const int s = WIDE_A + __builtin_ctz(m), d = (WIDE_ROWS - 1 - ty) + 1 + WIDE_A * j + (s - WIDE_A);
                if (d > k) break;
                if (rowcut && !(s_sp2[ty][s] < a_late)) { stop_dn = true; break; }
                row(s, d);
            }
    }
    // One distance per cell, as in k_dist_bits.
    const T m = sb_dist_finish_wave(a_early, a_late, maxdist);
    if (!active) return;
    const size_t o = g.at(xx, yy, nx);
    sb_dist_write(cdist + o, m, mask + o);
}

template <typename T>
hipError_t sb_launch_edges(const T *lsm, const T *ci, T *coast, int nx, int ny, int rule, int bnd, hipStream_t st) {
    Geo g;
    g.nx = nx; g.ny = ny; g.h = 0; g.nxh = nx; g.nyh = ny; g.nw = (nx + 63) / 64; g.bnd = bnd; g.rows = ny;
    hipLaunchKernelGGL(k_edges<T>, dim3((nx + 255) / 256, (ny + EDGE_ROWS - 1) / EDGE_ROWS), dim3(256), 0, st, lsm, ci, coast, g, rule);
    return hipGetLastError();
}

template <typename T>
hipError_t sb_launch_edges_band(const T *lsm, const T *ci, T *coast, int nx, int ny, int h, int south, int north, int rule,
                                hipStream_t st) {
    const EdgesBand<T> p{nx, ny, h, nx + 2 * h, south, north, rule};
    hipLaunchKernelGGL(k_edges_band<T>, dim3((nx + 255) / 256, (ny + EDGE_ROWS - 1) / EDGE_ROWS), dim3(256), 0, st, lsm, ci, coast, p);
    return hipGetLastError();
}

// coast, mask, cdist: the cell of column 0 of source row 0, rows ld apart; ny source rows, of which g's are targets (nt
// of them: only those are launched)
template <typename T, typename G>
static hipError_t sb_launch_dist_g(const T *coast, const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl,
                                   T *cdist, int nx, int ny, int nt, int ld, int k, T maxdist, uint64_t *bits, int cuts,
                                   const G g, hipStream_t st, bool pack = true) {
    if (k > SB_DIST_MAX_WINDOW || !bits) return hipErrorInvalidValue;    // (the C ABI holds k <= SB_DIST_MAX_WINDOW)
    const SbDistKernel kern = sb_dist_kernel(nx, k);
    const int nw = (nx + 63) / 64, nearest = cuts & SB_CUT_NEAREST;
    // (pack == false: `bits` already holds the coast's bit plane and there is no coast plane -- sb_launch_dist_dirty)
    if (!pack && kern == SbDistKernel::BYTES) return hipErrorInvalidValue;
    if (pack && kern != SbDistKernel::BYTES) sb_launch_coastbits<T>(coast, bits, nx, ny, nw, ld, 0, st);
    const dim3 gr((nx + 255) / 256, (nt + DIST_ROWS - 1) / DIST_ROWS), bl(256, DIST_ROWS);
    switch (kern) {
    case SbDistKernel::BYTES:
        hipLaunchKernelGGL((k_dist<T, G>), dim3((nx + 63) / 64, (nt + SB_DIST_TY - 1) / SB_DIST_TY), dim3(256),
                           (size_t)(64 + 2 * k) * (SB_DIST_TY + 2 * k), st, coast, mask, phi, lamf, cdist, nx, ny, k, maxdist, g);
        break;
    case SbDistKernel::BITS_SMALL:
        hipLaunchKernelGGL((k_dist_bits_small<T, G>), dim3((nx + 255) / 256, nt), dim3(256), 0, st, bits, mask, phi, lamf, shl, chl, cdist,
                           nx, ny, nw, k, maxdist, nearest, g);
        break;
    case SbDistKernel::BITS32:
        hipLaunchKernelGGL((k_dist_bits<T, uint32_t, G>), gr, bl, 0, st, bits, mask, phi, lamf, shl, chl, cdist, nx, ny, nw, k, maxdist, nearest, g);
        break;
    case SbDistKernel::BITS64:
        hipLaunchKernelGGL((k_dist_bits<T, uint64_t, G>), gr, bl, 0, st, bits, mask, phi, lamf, shl, chl, cdist, nx, ny, nw, k, maxdist, nearest, g);
        break;
    case SbDistKernel::WIDE:
        hipLaunchKernelGGL((k_dist_wide<T, G>), dim3((nx + 255) / 256, (nt + WIDE_ROWS - 1) / WIDE_ROWS), dim3(256, WIDE_ROWS), 0, st, bits, mask,
                           phi, lamf, shl, chl, cdist, nx, ny, nw, k, maxdist, cuts, g);
        break;
    }
    return hipGetLastError();
}

template <typename T>
hipError_t sb_launch_dist(const T *coast, const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl, T *cdist,
                          int nx, int ny, int k, T maxdist, uint64_t *bits, int cuts, hipStream_t st) {
    return sb_launch_dist_g<T, DistWhole>(coast, mask, phi, lamf, shl, chl, cdist, nx, ny, ny, nx, k, maxdist, bits, cuts, DistWhole{}, st);
}

template <typename T>
hipError_t sb_launch_dist_band(const T *coast, const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl, T *cdist,
                               int nx, int nys, int r0, int r1, int ld, int k, T maxdist, uint64_t *bits, int cuts, hipStream_t st) {
    if (r0 < 0 || r1 > nys || r1 <= r0 || ld < nx) return hipErrorInvalidValue;
    return sb_launch_dist_g<T, DistBand>(coast, mask, phi, lamf, shl, chl, cdist, nx, nys, r1 - r0, ld, k, maxdist, bits, cuts,
                                         DistBand{r0, r1, ld}, st);
}

// The whole grid of a stream whose coast moves: `bits` is the stream's own bit plane, kept up to date by k_edge_bits_delta
// (sb_ice_kernels.hip), which also left the marks; the kernel sb_launch_dist would take, one workgroup per tile as ever --
// the clean ones leave at once.  Not for grids narrower than the window (k_dist reads a coast plane: sb_ice_plan.hpp).
template <typename T>
hipError_t sb_launch_dist_dirty(const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl, T *cdist, int nx, int ny,
                                int k, T maxdist, const uint64_t *bits, int cuts, const unsigned char *marks, hipStream_t st) {
    return sb_launch_dist_g<T, DistDirty>(nullptr, mask, phi, lamf, shl, chl, cdist, nx, ny, ny, nx, k, maxdist, (uint64_t *)bits, cuts,
                                          DistDirty{marks, (nx + 255) / 256}, st, false);
}

// One latitude band whose coast moves (sb_band_ice_*): sb_launch_dist_band's arguments without a coast plane -- `bits` is
// the band's own bit plane over its nys source rows, kept up to date by k_edge_bits_delta's band instance, which also left the marks
// (one byte per (own row, tile)).  The kernel sb_launch_dist_band would take; not k_dist (sb_ice_plan.hpp).
template <typename T>
hipError_t sb_launch_dist_band_dirty(const T *mask, const T *phi, const T *lamf, const T *shl, const T *chl, T *cdist, int nx,
                                     int nys, int r0, int r1, int ld, int k, T maxdist, const uint64_t *bits, int cuts,
                                     const unsigned char *marks, hipStream_t st) {
    if (r0 < 0 || r1 > nys || r1 <= r0 || ld < nx || !marks) return hipErrorInvalidValue;
    return sb_launch_dist_g<T, DistBandDirty>(nullptr, mask, phi, lamf, shl, chl, cdist, nx, nys, r1 - r0, ld, k, maxdist,
                                              (uint64_t *)bits, cuts, DistBandDirty{r0, r1, ld, marks, (nx + 255) / 256}, st, false);
}

template hipError_t sb_launch_edges<float>(const float *, const float *, float *, int, int, int, int, hipStream_t);
template hipError_t sb_launch_edges<double>(const double *, const double *, double *, int, int, int, int, hipStream_t);
template hipError_t sb_launch_edges_band<float>(const float *, const float *, float *, int, int, int, int, int, int, hipStream_t);
template hipError_t sb_launch_edges_band<double>(const double *, const double *, double *, int, int, int, int, int, int, hipStream_t);
template hipError_t sb_launch_dist<float>(const float *, const float *, const float *, const float *, const float *, const float *,
                                          float *, int, int, int, float, uint64_t *, int, hipStream_t);
template hipError_t sb_launch_dist<double>(const double *, const double *, const double *, const double *, const double *,
                                           const double *, double *, int, int, int, double, uint64_t *, int, hipStream_t);
template hipError_t sb_launch_dist_band<float>(const float *, const float *, const float *, const float *, const float *, const float *,
                                               float *, int, int, int, int, int, int, float, uint64_t *, int, hipStream_t);
template hipError_t sb_launch_dist_band<double>(const double *, const double *, const double *, const double *, const double *,
                                                const double *, double *, int, int, int, int, int, int, double, uint64_t *, int, hipStream_t);
template hipError_t sb_launch_dist_dirty<float>(const float *, const float *, const float *, const float *, const float *, float *, int,
                                                int, int, float, const uint64_t *, int, const unsigned char *, hipStream_t);
template hipError_t sb_launch_dist_dirty<double>(const double *, const double *, const double *, const double *, const double *, double *,
                                                 int, int, int, double, const uint64_t *, int, const unsigned char *, hipStream_t);
template hipError_t sb_launch_dist_band_dirty<float>(const float *, const float *, const float *, const float *, const float *,
                                                     float *, int, int, int, int, int, int, float, const uint64_t *, int,
                                                     const unsigned char *, hipStream_t);
template hipError_t sb_launch_dist_band_dirty<double>(const double *, const double *, const double *, const double *, const double *,
                                                      double *, int, int, int, int, int, int, double, const uint64_t *, int,
                                                      const unsigned char *, hipStream_t);
