// sb_ice_plan.hpp -- what an ice call of a stream (sb_diag_stream_ice_*) decides: which path it takes, and what a changed
// word of the coast bit plane can reach.  sb_capi.hip asks for the path, k_edge_bits_delta (sb_ice_kernels.hip) marks with
// the same sb_ice_reach the host-only test walks (tests/ice_plan_dump.cpp).  Plain C++17: no HIP, no heap -- a host
// compiler builds it alone; under hipcc the functions are also device functions.
//
// The mark plane holds one byte per (target row, 256-column tile): the tiles of the distance kernels (a workgroup of
// k_dist_bits_small is one row of a tile, of k_dist_bits and k_dist_wide two).  A target (xx, yy) reads the coast bits of
// rows yy-k .. yy+k inside the grid (rows past it add no sources) and of columns xx-k .. xx+k round the circle (every
// column once where 2k+1 >= nx), so a changed cell (x, y) can move the targets of rows y-k .. y+k, clamped, and columns
// x-k .. x+k, circular, and nothing else.  A wave's targets share ballots (sb_dist_finish_wave), so what is computed again
// must be whole waves: whole tiles are.  The kernel compares whole 64-cell words, so a changed word at columns
// x0 .. x0+63 marks the tiles that cover x0-k .. x0+63+k -- at most 63 + k columns beyond a changed cell on either side --
// and the whole row where that span goes round the circle (2k + 64 >= nx).  Over-marking costs time; under-marking
// would leave a stale distance.
#pragma once
#include "sb_dist_plan.hpp"

#if defined(__HIPCC__)
#define SB_ICE_HD __host__ __device__ inline
#else
#define SB_ICE_HD inline
#endif

#define SB_ICE_TILE 256                                          // columns of a tile: the distance kernels' workgroup width

SB_ICE_HD int sb_ice_tiles(int nx) { return (nx + SB_ICE_TILE - 1) / SB_ICE_TILE; }

// the target rows r0 .. r1 and the tile columns a0 .. a1 and b0 .. b1 (the second piece is empty, b1 < b0, unless the span
// crosses the seam) that the word at columns x0 .. x0+63 (x0 a multiple of 64, < nx) of row y can reach
struct SbIceReach {
    int r0, r1, a0, a1, b0, b1;
};

SB_ICE_HD SbIceReach sb_ice_reach(int nx, int ny, int k, int x0, int y) {
    SbIceReach r;
    r.r0 = y - k < 0 ? 0 : y - k;
    r.r1 = y + k > ny - 1 ? ny - 1 : y + k;
    const int nt = sb_ice_tiles(nx), len = 2 * k + 64;
    r.b0 = 0; r.b1 = -1;
    if (len >= nx) { r.a0 = 0; r.a1 = nt - 1; return r; }        // once round the circle: the whole row
    int c = x0 - k;                                              // first column in reach, circular (k < nx here)
    if (c < 0) c += nx;
    const int e = c + len - 1;                                   // last one, not yet wrapped
    r.a0 = c / SB_ICE_TILE;
    if (e < nx) { r.a1 = e / SB_ICE_TILE; return r; }
    r.a1 = nt - 1;
    r.b1 = (e - nx) / SB_ICE_TILE;
    return r;
}

// WHOLE: k_edges into a scratch plane and the whole-grid distance launch (sb_launch_dist), for a stream opened with
// incremental = 0 and for grids narrower than the window, where the distance kernel is k_dist (byte probes of a coast
// plane: it has no bit plane to compare).  DELTA: k_edge_bits_delta and the distance kernel under DistDirty.
enum class SbIcePath { WHOLE, DELTA };

inline SbIcePath sb_ice_path(int nx, int k, int incremental) {
    if (!incremental || sb_dist_kernel(nx, k) == SbDistKernel::BYTES) return SbIcePath::WHOLE;
    return SbIcePath::DELTA;
}
