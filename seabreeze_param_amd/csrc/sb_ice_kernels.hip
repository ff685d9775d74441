// sb_ice_kernels.hip -- the coast of a domain whose sea ice moves (sb_diag_stream_ice_*, sb_band_ice_*, sb_um_ice_*,
// sb_um_tile_ice_*): one kernel that turns the land mask and a step's ice plane into the domain's coast bit plane and says what the difference
// can reach.
//
//   k_edge_bits_delta  a Sobel block of k_edges (sb_edges_each, sb_coast_common.hpp) whose flags are balloted into the
//                      64-bit words of the bit plane straight away: no coast plane of T is written and read again, which
//                      k_edges + k_coastbits pay.  A word belongs to one wave of one workgroup, so that wave reads the
//                      stored word, and where the new one differs writes it, counts it and marks every (row, tile) of the
//                      mark plane the word can reach -- the distance kernels under a Dist*Dirty policy then compute those
//                      again and leave the rest of the resident cdist alone.  One body, four instances, which differ in
//                      the Sobel policy and in the reach (sb_ice_plan.hpp: an SbIceReach in the rows and tiles of the
//                      layout's own mark plane, from the function the host-only tests walk):
//     the whole grid   EdgesIce: the f2py flavour's cell mapping and land rule (rule 0, lsm + ci > 0.4: ref sobel.f90:51,
//                      60-69); sb_ice_reach, one byte per (target row, 256-column tile); DistDirty behind it.
//     a latitude band  EdgesBandSrc over the band's SOURCE rows in its ghost-celled frame (either land rule, SB_BND_GLOBAL
//                      seen from a band; ghost source rows are compared and stored like own rows); sb_band_ice_reach, one
//                      byte per (OWN row, tile); DistBandDirty behind it.  k_edges_band_src writes the same coast as a
//                      plane for the whole path.
//     the UM layout    EdgesUm over the interior of the tdims_l frames (the UM's ice-aware rule on the interior and the
//                      one-cell ring; 256-column blocks from interior column 0, so a 64-cell word belongs to one wave);
//                      sb_um_ice_reach (no wrap, one piece), one byte per workgroup of the UM distance kernels (row group x
//                      64-column tile); DistUmDirty behind it.  EdgesUm keeps tail_by_index: that only says how lanes past
//                      the ring are staged; lanes whose column is past nx still leave sb_edges_each before emit.
//                      k_edges_um writes the same coast as a plane for the whole path.
//     a UM tile        EdgesUmTileSrc over the tile's SOURCE rectangle in the rank's frame (EdgesUmTile's rule: the interior
//                      and e* ghost columns / rows on each side, sb_ice_plan.hpp; 256-column blocks from rectangle column
//                      0, so a word of the rectangle's bit plane belongs to one wave); sb_um_tile_ice_reach, the UM
//                      layout's mark plane over the interior; DistUmTileDirty behind it.  k_edges_um_tile writes the
//                      same coast as a plane for the whole path.
// Marks are stores of 1 into a byte plane the host cleared ahead of the launch: stores that race write the same value.
// rep[0] counts the changed words of this call (cleared with the marks); the wave that counts the first one adds one
// to rep[1], the calls whose coast differed, unless the call is the domain's first (`first`: everything is marked by the
// host and the stored plane is the empty one).
#include "../../include/seabreeze_hip.h"
#include "sb_device.hpp"
#include "sb_launch.hpp"
#include "sb_coast_common.hpp"
#include "sb_ice_plan.hpp"

template <typename T>
struct EdgesIce {
    static constexpr bool tail_by_index = false;
    Geo g;
    __device__ __forceinline__ int cols() const { return g.nx; }
    __device__ __forceinline__ int rows() const { return g.ny; }
    __device__ __forceinline__ size_t src(int x, int y) const {
        int X, Y;
        sb_map_cell(g, x, y, X, Y);
        return (size_t)Y * g.nx + X;
    }
    __device__ __forceinline__ int land(T l, T c) const { return (l + c > T(0.4)) ? 1 : 0; }     // ref: sobel.f90:51,69
};

// the reach of the word at (x0, y) of the bit plane, and the tiles per row of the mark plane it is stated in
struct ReachGrid {
    int nx, ny, k;
    __device__ __forceinline__ int tiles() const { return sb_ice_marks(nx, ny).tiles; }
    __device__ __forceinline__ SbIceReach operator()(int x0, int y) const { return sb_ice_reach(nx, ny, k, x0, y); }
};
struct ReachBand {
    int nx, r0, r1, k;
    __device__ __forceinline__ int tiles() const { return sb_ice_marks(nx, r1 - r0).tiles; }
    __device__ __forceinline__ SbIceReach operator()(int x0, int s) const { return sb_band_ice_reach(nx, r0, r1, k, x0, s); }
};
struct ReachUm {
    int nx, ny, wi, wj;
    __device__ __forceinline__ int tiles() const { return sb_um_ice_marks(nx, ny).tiles; }
    __device__ __forceinline__ SbIceReach operator()(int x0, int y) const { return sb_um_ice_reach(nx, ny, wi, wj, x0, y); }
};
struct ReachUmTile {
    int nx, ny, wi, wj, eW, eS;                                  // nx, ny: the interior; (x0, s): a word of the source rectangle
    __device__ __forceinline__ int tiles() const { return sb_um_ice_marks(nx, ny).tiles; }
    __device__ __forceinline__ SbIceReach operator()(int x0, int s) const {
        return sb_um_tile_ice_reach(nx, ny, wi, wj, eW, eS, x0, s);
    }
};

// p.cols() x p.rows(): the cells of the bit plane (a band's source rows) -- from the policy, so that the Sobel and the
// emit share one copy in registers.  lsm, ci: what p.src() indexes.
template <typename T, typename P, typename R>
__global__ __launch_bounds__(256) void k_edge_bits_delta(const T *__restrict__ lsm, const T *__restrict__ ci,
                                                         uint64_t *__restrict__ bits, unsigned char *__restrict__ marks,
                                                         unsigned *__restrict__ rep, P p, R reach, int first) {
    __shared__ unsigned char s_land[EDGE_LDS];
    const int nx = p.cols(), ny = p.rows(), nw = (nx + 63) >> 6, nt = reach.tiles();
    const int lane = threadIdx.x & 63;
    sb_edges_each(lsm, ci, s_land, nx, ny, p, [&](int x, int y, bool c) {
        // (lanes past nx have left: they add no bit, and the wave's first lane is in whenever any of them is)
        const uint64_t w = __ballot(c);
        uint64_t *word = bits + (size_t)y * nw + (x >> 6);
        const uint64_t old = *word;                              // one address per wave
        if (old == w) return;                                    // wave-uniform
        const SbIceReach r = reach(x & ~63, y);
        const int nact = nx - (x & ~63) < 64 ? nx - (x & ~63) : 64;  // lanes still here: fewer than 64 in the ragged last word
        for (int ym = r.r0 + lane; ym <= r.r1; ym += nact) {
            unsigned char *row = marks + (size_t)ym * nt;
            for (int t = r.a0; t <= r.a1; ++t) row[t] = 1;
            for (int t = r.b0; t <= r.b1; ++t) row[t] = 1;
        }
        if (lane == 0) {
            *word = w;
            if (atomicAdd(rep, 1u) == 0u && !first) atomicAdd(rep + 1, 1u);
        }
    });
}

template <typename T, typename P, typename R>
static hipError_t launch_delta(const T *lsm, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, P p, R reach, int nx,
                               int ny, int first, hipStream_t st) {
    hipLaunchKernelGGL((k_edge_bits_delta<T, P, R>), dim3((nx + 255) / 256, (ny + EDGE_ROWS - 1) / EDGE_ROWS), dim3(256), 0, st, lsm,
                       ci, bits, marks, rep, p, reach, first);
    return hipGetLastError();
}

template <typename T>
hipError_t sb_launch_edge_bits_delta(const T *lsm, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx, int ny,
                                     int k, int first, hipStream_t st) {
    Geo g;
    g.nx = nx; g.ny = ny; g.h = 0; g.nxh = nx; g.nyh = ny; g.nw = (nx + 63) / 64; g.bnd = BND_WRAPPER; g.rows = ny;
    g.band = 0;
    return launch_delta(lsm, ci, bits, marks, rep, EdgesIce<T>{g}, ReachGrid{nx, ny, k}, nx, ny, first, st);
}

// ---- one latitude band (sb_band_ice_*) ----
// lsm, ci: the frame's first cell.  The whole path: the same Sobel policy writes a coast plane over the source rows
// (scratch of the frame's pitch).
template <typename T>
__global__ __launch_bounds__(256) void k_edges_band_src(const T *__restrict__ lsm, const T *__restrict__ ci,
                                                        T *__restrict__ coast, EdgesBandSrc<T> p) {
    __shared__ unsigned char s_land[EDGE_LDS];
    sb_edges_block(lsm, ci, coast, s_land, p.nx, p.nys, p);
}

template <typename T>
static EdgesBandSrc<T> band_src_policy(int nx, int h, const SbBandRows &br, int south, int north, int rule) {
    return EdgesBandSrc<T>{nx, br.nys, h, nx + 2 * h, br.f0, south ? 0 : -1, north ? br.nys - 1 : br.nys, rule};
}

template <typename T>
hipError_t sb_launch_edge_bits_delta_band(const T *lsm, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx,
                                          int h, SbBandRows br, int south, int north, int rule, int k, int first, hipStream_t st) {
    if ((!south || !north) && k + 1 > h) return hipErrorInvalidValue;        // (the (k+1)-th ghost row lies inside the frame)
    return launch_delta(lsm, ci, bits, marks, rep, band_src_policy<T>(nx, h, br, south, north, rule), ReachBand{nx, br.r0, br.r1, k},
                        nx, br.nys, first, st);
}

template <typename T>
hipError_t sb_launch_edges_band_src(const T *lsm, const T *ci, T *coast, int nx, int h, SbBandRows br, int south, int north,
                                    int rule, int k, hipStream_t st) {
    if ((!south || !north) && k + 1 > h) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_edges_band_src<T>, dim3((nx + 255) / 256, (br.nys + EDGE_ROWS - 1) / EDGE_ROWS), dim3(256), 0, st, lsm, ci,
                       coast, band_src_policy<T>(nx, h, br, south, north, rule));
    return hipGetLastError();
}

// ---- the UM layout (sb_um_ice_*) ----
// lf, ci: the frame's first cell.
template <typename T>
hipError_t sb_launch_edge_bits_delta_um(const T *lf, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx,
                                        int ny, int hi, int hj, int wi, int wj, int first, hipStream_t st) {
    if (hi < 1 || hj < 1 || wi < 0 || wj < 0) return hipErrorInvalidValue;       // (the ring lies inside the frame)
    return launch_delta(lf, ci, bits, marks, rep, EdgesUm<T>{nx + 2 * hi, ny + 2 * hj, hi, hj}, ReachUm{nx, ny, wi, wj}, nx, ny,
                        first, st);
}

// ---- one tile of the UM layout's 2-D decomposition (sb_um_tile_ice_*) ----
// lf, ci: the frame's first cell; r: the source rectangle (sb_um_tile_ice_sources); bits: its plane.
template <typename T>
hipError_t sb_launch_edge_bits_delta_um_tile(const T *lf, const T *ci, uint64_t *bits, unsigned char *marks, unsigned *rep, int nx,
                                             int ny, int hi, int hj, int wi, int wj, SbTileReach r, int first, hipStream_t st) {
    // the ring lies inside the frame, and a changed word's reach inside the mark plane (e* <= the window: sb_ice_plan.hpp)
    if (r.eW < 0 || r.eE < 0 || r.eS < 0 || r.eN < 0 || r.eW > wi || r.eE > wi || r.eS > wj || r.eN > wj || hi < r.eW + 1 ||
        hi < r.eE + 1 || hj < r.eS + 1 || hj < r.eN + 1)
        return hipErrorInvalidValue;
    const int wx = nx + r.eW + r.eE, wy = ny + r.eS + r.eN;
    const EdgesUmTileSrc<T> p{{nx + 2 * hi, ny + 2 * hj, hi - r.eW, hj - r.eS}, wx, wy};
    return launch_delta(lf, ci, bits, marks, rep, p, ReachUmTile{nx, ny, wi, wj, r.eW, r.eS}, wx, wy, first, st);
}

template hipError_t sb_launch_edge_bits_delta_um_tile<float>(const float *, const float *, uint64_t *, unsigned char *, unsigned *,
                                                             int, int, int, int, int, int, SbTileReach, int, hipStream_t);
template hipError_t sb_launch_edge_bits_delta_um_tile<double>(const double *, const double *, uint64_t *, unsigned char *,
                                                              unsigned *, int, int, int, int, int, int, SbTileReach, int, hipStream_t);

template hipError_t sb_launch_edge_bits_delta_um<float>(const float *, const float *, uint64_t *, unsigned char *, unsigned *, int,
                                                        int, int, int, int, int, int, hipStream_t);
template hipError_t sb_launch_edge_bits_delta_um<double>(const double *, const double *, uint64_t *, unsigned char *, unsigned *,
                                                         int, int, int, int, int, int, int, hipStream_t);

template hipError_t sb_launch_edge_bits_delta_band<float>(const float *, const float *, uint64_t *, unsigned char *, unsigned *, int,
                                                          int, SbBandRows, int, int, int, int, int, hipStream_t);
template hipError_t sb_launch_edge_bits_delta_band<double>(const double *, const double *, uint64_t *, unsigned char *, unsigned *,
                                                           int, int, SbBandRows, int, int, int, int, int, hipStream_t);
template hipError_t sb_launch_edges_band_src<float>(const float *, const float *, float *, int, int, SbBandRows, int, int, int, int,
                                                    hipStream_t);
template hipError_t sb_launch_edges_band_src<double>(const double *, const double *, double *, int, int, SbBandRows, int, int, int,
                                                     int, hipStream_t);

template hipError_t sb_launch_edge_bits_delta<float>(const float *, const float *, uint64_t *, unsigned char *, unsigned *, int, int, int,
                                                     int, hipStream_t);
template hipError_t sb_launch_edge_bits_delta<double>(const double *, const double *, uint64_t *, unsigned char *, unsigned *, int, int,
                                                      int, int, hipStream_t);
