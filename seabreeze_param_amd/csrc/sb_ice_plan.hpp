// sb_ice_plan.hpp -- what an ice call of a stream (sb_diag_stream_ice_*), of a latitude band (sb_band_ice_*) or of the UM
// layout (sb_um_ice_*) or of one tile of its 2-D decomposition (sb_um_tile_ice_*) decides: which path it takes, and what a
// changed word of the coast bit plane can reach.
// sb_capi_stream.hip and sb_capi_coast.hip ask for the path, the four instances of k_edge_bits_delta (sb_ice_kernels.hip)
// mark with the same sb_ice_reach / sb_band_ice_reach / sb_um_ice_reach / sb_um_tile_ice_reach the host-only tests walk
// (tests/plan_dump.cpp, tests/um_tile_ice_plan_dump.cpp).
// Every layout states its mark plane as one SbIceMarks (rows x tiles bytes) and its reach as one SbIceReach in the rows and
// tiles OF THAT PLANE, so the kernel's mark loop, the distance kernels' early exit and the report read any of them alike.
// Plain C++17: no HIP, no heap -- a host compiler builds it alone; under hipcc the functions are also device functions.
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

// a mark plane: rows x tiles bytes, row by row
struct SbIceMarks {
    int rows, tiles;
};

SB_ICE_HD SbIceMarks sb_ice_marks(int nx, int ny) { return SbIceMarks{ny, sb_ice_tiles(nx)}; }

// what the word at columns x0 .. x0+63 (x0 a multiple of 64, < nx) of one row of the bit plane can reach, in any layout:
// rows r0 .. r1 of the mark plane and its tiles a0 .. a1 and b0 .. b1 (all inclusive; the second piece is empty, b1 < b0,
// unless the span crosses the seam of a circular grid)
struct SbIceReach {
    int r0, r1, a0, a1, b0, b1;
};

// the whole grid: the mark plane's rows are the target rows

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

// ---- one latitude band in its ghost-celled frame (sb_band_ice_*; sb_capi_coast.hip) ----
// The bit plane covers the band's SOURCE rows 0 .. nys-1 (sb_band_rows, sb_dist_plan.hpp: the band's own rows and k ghost
// rows on each cut side), the targets are source rows r0 .. r1-1, the mark plane holds one byte per (own row, tile): row
// yt - r0.  The argument above holds with "rows inside the grid" read as "source rows of the band": a target (xx, yy)
// under DistBand reads the bit plane's rows yy-k .. yy+k inside 0 .. nys-1 and nothing else of the coast (rows past a pole
// add no sources, rows past a cut side's k-th ghost row lie beyond the window of every own row), and the columns xx-k ..
// xx+k round the circle.  So a changed word at source row s, columns x0 .. x0+63, can move the targets of rows
// max(s-k, r0) .. min(s+k, r1-1) -- never an empty range: r0 <= k and r1-1 >= nys-1-k -- and of sb_ice_reach's tile columns.
// DistBand tiles from column 0 with one target row per wave, as on the globe, so a tile holds whole waves here too.
// Ghost source rows are compared and stored like own rows: their bits are what the neighbour band holds for its own
// rows, formed here from the k+1 ghost rows of lsm and ci (the Sobel of the k-th ghost row reads the (k+1)-th).
// r0, r1 of the result are OWN rows, the rows of the mark plane: the band's row offset is applied here and nowhere else.
// Counted from the first own row that is the whole grid's rule for a plane of r1 - r0 rows and the row s - r0 (negative
// south of the band, beyond the plane north of it: the clamp serves both): rows max(s-r0-k, 0) .. min(s-r0+k, r1-r0-1).
SB_ICE_HD SbIceReach sb_band_ice_reach(int nx, int r0, int r1, int k, int x0, int s) {
    return sb_ice_reach(nx, r1 - r0, k, x0, s - r0);
}

// WHOLE: k_edges into a scratch plane and the whole-grid distance launch (sb_launch_dist), for a stream opened with
// incremental = 0 and for grids narrower than the window, where the distance kernel is k_dist (byte probes of a coast
// plane: it has no bit plane to compare).  DELTA: k_edge_bits_delta and the distance kernel under DistDirty.
enum class SbIcePath { WHOLE, DELTA };

inline SbIcePath sb_ice_path(int nx, int k, int incremental) {
    if (!incremental || sb_dist_kernel(nx, k) == SbDistKernel::BYTES) return SbIcePath::WHOLE;
    return SbIcePath::DELTA;
}

// What sb_band_coast_open_* decides for a band of ny own rows with `halo` ghost cells: ok == false where a cut side lacks
// the (k+1)-th ghost row of lsm and ci -- frame rows f0-1 and f0+nys, which the Sobel of the outermost ghost source rows
// reads (a pole side reads nothing beyond the band's edge row, so south and north both set needs no ghost row at all);
// else the source rows, the path (the whole grid's rule: the kernels are the same) and the sizes of the planes.
struct SbBandIcePlan {
    bool ok;
    SbBandRows rows;
    SbIcePath path;
    int nw;                  // words per row of the bit plane (rows.nys rows)
    SbIceMarks marks;        // ny own rows x tiles
};

inline SbBandIcePlan sb_band_ice_plan(int nx, int ny, int halo, bool south, bool north, int k, int incremental) {
    SbBandIcePlan p{};
    p.ok = k >= 0 && halo >= 0 && ((south && north) || k + 1 <= halo);
    if (!p.ok) return p;
    p.rows = sb_band_rows(ny, halo, south, north, k);
    p.path = sb_ice_path(nx, k, incremental);
    p.nw = (nx + 63) / 64;
    p.marks = sb_ice_marks(nx, ny);
    return p;
}

// ---- the UM layout (sb_um_coast_open_*, sb_um_ice_*; sb_capi_coast.hip) ----
// The mark plane holds one byte per WORKGROUP of the UM distance kernels (k_dist_um, k_dist_um_wide:
// sb_um_coast_kernels.hip): SB_UM_ICE_ROWS target rows x SB_UM_ICE_COLS columns, tiled from interior cell (0, 0).  The
// granularity can be the workgroup, finer than a stream's tiles of whole waves, because these two kernels have no coupling
// between targets: no ballot over targets decides a value (sb_dist_finish_both is per lane; __syncthreads_or only asks
// whether the reach holds a coast bit at all), and the early exits -- a reach, a pass, a chunk or a row without a coast
// bit, the wide kernel's per-pair latitude cut -- skip work that cannot lower a minimum: they are value-neutral.  So a
// target's value is a function of its own window and nothing its neighbours do.
// A target (xx, yy) reads the coast bits of interior rows yy-wj .. yy+wj and interior columns xx-wi .. xx+wi that exist --
// no wrap, no clamp: a window that reaches past the interior finds nothing there -- and nothing else of the coast;
// landfrac, the coordinates and maxdist stand while the coast is open, and both sweep classes and the reset are
// functions of those bits alone.  So the changed word at columns x0 .. x0+63 of interior row y can move the targets of
// rows max(y-wj, 0) .. min(y+wj, ny-1) and columns max(x0-wi, 0) .. min(x0+63+wi, nx-1), one piece, and nothing else.
// Over-marking costs time and comes from whole words, whole row groups and whole tiles; under-marking would leave a
// stale distance.
#define SB_UM_ICE_ROWS 4                                         // target rows of a workgroup (UM_DIST_TY, UMW_TY)
#define SB_UM_ICE_COLS 64                                        // its columns: one wave per row

// row groups x tiles
SB_ICE_HD SbIceMarks sb_um_ice_marks(int nx, int ny) {
    return SbIceMarks{(ny + SB_UM_ICE_ROWS - 1) / SB_UM_ICE_ROWS, (nx + SB_UM_ICE_COLS - 1) / SB_UM_ICE_COLS};
}

// the row groups r0 .. r1 and the tiles a0 .. a1 (never empty; no second piece: nothing wraps) whose workgroups hold a
// target the word at columns x0 .. x0+63 (x0 a multiple of 64, < nx) of interior row y (< ny) can move.  (A UM tile's words
// lie elsewhere -- x0 and y may be negative or beyond the interior: sb_um_tile_ice_reach below says why the clamps serve.)
SB_ICE_HD SbIceReach sb_um_ice_reach(int nx, int ny, int wi, int wj, int x0, int y) {
    SbIceReach r;
    const int ra = y - wj < 0 ? 0 : y - wj, rb = y + wj > ny - 1 ? ny - 1 : y + wj;
    const int ca = x0 - wi < 0 ? 0 : x0 - wi, cb = x0 + 63 + wi > nx - 1 ? nx - 1 : x0 + 63 + wi;
    r.r0 = ra / SB_UM_ICE_ROWS; r.r1 = rb / SB_UM_ICE_ROWS;
    r.a0 = ca / SB_UM_ICE_COLS; r.a1 = cb / SB_UM_ICE_COLS;
    r.b0 = 0; r.b1 = -1;
    return r;
}

// The UM layout has no byte-probe kernel -- both distance kernels read the bit plane -- so `incremental` alone decides.
// WHOLE: k_edges_um into a scratch frame and sb_launch_dist_um_win; DELTA: k_edge_bits_delta's UM instance and the distance kernel
// under DistUmDirty.
inline SbIcePath sb_um_ice_path(int incremental) { return incremental ? SbIcePath::DELTA : SbIcePath::WHOLE; }

// What sb_um_coast_open_* decides: ok == false for sizes, halos (the Sobel reads the one-cell ring) or windows it refuses;
// else the path and the sizes of the planes.
struct SbUmIcePlan {
    bool ok;
    SbIcePath path;
    int nw;                      // words per row of the bit plane (ny rows)
    SbIceMarks marks;            // row groups x tiles per group
};

inline SbUmIcePlan sb_um_ice_plan(int nx, int ny, int hi, int hj, int wi, int wj, int incremental) {
    SbUmIcePlan p{};
    p.ok = nx >= 1 && ny >= 1 && hi >= 1 && hj >= 1 && wi >= 0 && wi <= 255 && wj >= 0 && wj <= 255;
    if (!p.ok) return p;
    p.path = sb_um_ice_path(incremental);
    p.nw = (nx + 63) / 64;
    p.marks = sb_um_ice_marks(nx, ny);
    return p;
}

// ---- one tile of the UM layout's 2-D decomposition (sb_um_tile_coast_open_*, sb_um_tile_ice_*; sb_capi_coast.hip) ----
// Every field is the rank's frame of (nx + 2hi) x (ny + 2hj) cells with the interior at (hi, hj).  beyond[4]: the domain
// cells beyond the tile's west, east, south and north side (0: that side is the domain's edge).  Sources are the coast
// cells of the rectangle [-eW, nx+eE) x [-eS, ny+eN) in interior coordinates, e* = min(window, beyond*): sb_tile_reach
// (sb_um_coast_kernels.hip) with the domain's end stated, so a neighbour narrower than the window needs nothing of the
// caller (the setup calls leave that to a zeroed coast_l; an ice call has no coast_l).
struct SbTileReach { int eW, eE, eS, eN; };

inline SbTileReach sb_um_tile_ice_sources(int wi, int wj, const int beyond[4]) {
    return SbTileReach{beyond[0] < wi ? beyond[0] : wi, beyond[1] < wi ? beyond[1] : wi, beyond[2] < wj ? beyond[2] : wj,
                       beyond[3] < wj ? beyond[3] : wj};
}

// The bit plane spans exactly the source rectangle -- pitch ceil((nx+eW+eE)/64) words, origin (-eW, -eS), so a word is
// aligned to the rectangle and may straddle the interior's west edge -- and the mark plane is sb_um_ice_marks(nx, ny): one
// byte per workgroup of k_dist_um_tile, tiled from interior cell (0, 0).  k_dist_um_tile is um_dist_wide_body, whose
// targets are as uncoupled as sb_um_ice_reach's argument needs (no ballot over targets, value-neutral exits).  A target
// (xx, yy) of the interior reads the coast bits of rows yy-wj .. yy+wj and columns xx-wi .. xx+wi that lie inside the
// rectangle (src_rows clips the rows, um_row_bits64's zeros beyond the plane the columns) and nothing else of the coast.
// The word at rectangle columns x0 .. x0+63 of rectangle row s holds interior columns x0-eW .. x0-eW+63 of interior row
// s-eS, so it can move the targets of rows max(s-eS-wj, 0) .. min(s-eS+wj, ny-1) and columns max(x0-eW-wi, 0) ..
// min(x0-eW+63+wi, nx-1) and nothing else: sb_um_ice_reach of (x0-eW, s-eS), whose two clamps serve arguments that are
// negative (a ghost word west or south of the interior) or beyond the interior (east, north) as they stand.  Neither
// range is empty: e* <= the window gives x0-eW+63+wi >= 63 and s-eS+wj >= 0; x0 < nx+eW+eE gives x0-eW-wi < nx+eE-wi <= nx,
// and s < ny+eS+eN gives s-eS-wj < ny likewise.  The same relation holds between sb_band_ice_reach and sb_ice_reach.
SB_ICE_HD SbIceReach sb_um_tile_ice_reach(int nx, int ny, int wi, int wj, int eW, int eS, int x0, int s) {
    return sb_um_ice_reach(nx, ny, wi, wj, x0 - eW, s - eS);
}

// What sb_um_tile_coast_open_* decides: ok == false for sizes, windows or a negative beyond it refuses and for a halo
// below e* + 1 on any side (the Sobel of the outermost source cell reads one cell further; on an edge side, e* = 0, that
// is the ring sb_get_edges_um_* reads); else the path (`incremental` alone, as sb_um_ice_path), the source rectangle and
// the sizes of the planes.
struct SbUmTileIcePlan {
    bool ok;
    SbIcePath path;
    SbTileReach reach;
    int nw;                      // words per row of the bit plane (ny + eS + eN rows)
    SbIceMarks marks;            // row groups x tiles per group of the interior
};

inline SbUmTileIcePlan sb_um_tile_ice_plan(int nx, int ny, int hi, int hj, int wi, int wj, const int beyond[4], int incremental) {
    SbUmTileIcePlan p{};
    p.ok = nx >= 1 && ny >= 1 && wi >= 0 && wi <= 255 && wj >= 0 && wj <= 255 && beyond[0] >= 0 && beyond[1] >= 0 &&
           beyond[2] >= 0 && beyond[3] >= 0;
    if (!p.ok) return p;
    const SbTileReach r = sb_um_tile_ice_sources(wi, wj, beyond);
    p.ok = hi >= r.eW + 1 && hi >= r.eE + 1 && hj >= r.eS + 1 && hj >= r.eN + 1;
    if (!p.ok) return p;
    p.path = sb_um_ice_path(incremental);
    p.reach = r;
    p.nw = (nx + r.eW + r.eE + 63) / 64;
    p.marks = sb_um_ice_marks(nx, ny);
    return p;
}
