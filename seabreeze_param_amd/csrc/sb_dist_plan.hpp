// sb_dist_plan.hpp -- what get_dist decides before it launches: what the coordinates allow the kernels to leave out, and
// which kernel runs.  get_dist_dev (sb_capi.hip) keeps the traits with its coordinate tables and forms the cuts per call,
// sb_launch_dist (sb_coast_kernels.hip) switches over the kernel, the kernels read the cut bits.  Plain C++17: no HIP, no
// heap -- a host compiler builds it alone (tests/dist_plan_dump.cpp).
#pragma once
#include <cmath>

// What a distance kernel may leave out; each cut is exact (sb_coast_common.hpp says why).
//   NEAREST  k_dist_bits[_small]: only the nearest hit on each side of a source row, and a walk over the rows that stops
//            at the first row that cannot lower its class's minimum (CIRCLE and ROWS together)
//   CIRCLE   k_dist_wide: the nearest hit per side in every row
//   INNER    k_dist_wide: the same for a target whose window lies inside 0 .. nx-1
//   ROWS     k_dist_wide: a sweep class stops at the first row that cannot lower its minimum
enum { SB_CUT_NEAREST = 1, SB_CUT_CIRCLE = 2, SB_CUT_INNER = 4, SB_CUT_ROWS = 8 };

// What the host finds out about the coordinates' order, each true only with every latitude within +-90 degrees
// (cos >= 0): longitudes in order round the whole circle, and the largest step | the steps j -> j+1, j < nx-1 (without
// the closing one) all one way, and the largest of them | latitudes stepping one way.
struct SbDistTraits {
    bool circle = false, inner = false, latmono = false;
    double maxstep = 0.0, maxstep_inner = 0.0;
};

template <typename T>
SbDistTraits sb_dist_traits(const T *lon, const T *lat, int nx, int ny) {
    SbDistTraits t;
    // k_dist_bits may keep only the nearest hit on each side of a source row when the haversine term grows with
    // the index distance inside the window: longitudes that step strictly eastwards once round the circle (the
    // closing step from the last column to the first included); and may stop its walk over the rows early when the
    // latitudes step one way.  (Whether the window stays short of half the circle depends on k: sb_dist_cuts.)
    double turn = 0.0, maxstep = 0.0;
    bool mono = nx > 1;
    for (int j = 0; j < nx && mono; ++j) {
        double d = std::fmod((double)lon[(j + 1) % nx] - (double)lon[j], 360.0);
        if (d < 0) d += 360.0;
        mono = d > 1.0e-6;
        turn += d;
        maxstep = d > maxstep ? d : maxstep;
    }
    bool latin = true;                        // cos(phi) >= 0: the haversine term grows with sin^2 of either difference
    for (int i = 0; i < ny && latin; ++i) latin = std::fabs((double)lat[i]) <= 90.0;
    bool latmono = latin;                     // sp^2 grows with the row distance: latitudes step one way
    for (int i = 0; i + 2 < ny && latmono; ++i)
        latmono = ((double)lat[i + 1] - (double)lat[i]) * ((double)lat[i + 2] - (double)lat[i + 1]) > 0.0;
    t.circle = latin && mono && turn < 360.0 + 1.0e-3;
    t.latmono = latmono;
    t.maxstep = maxstep;
    // k_dist_wide decides the column cut per target: a window that stays inside the frame never meets the closing
    // step, so for it the steps inside the frame decide (eastwards or westwards, folded to +-180 degrees)
    bool east = nx > 1, west = nx > 1;
    double maxin = 0.0;
    for (int j = 0; j + 1 < nx && (east || west); ++j) {
        double d = std::fmod((double)lon[j + 1] - (double)lon[j], 360.0);
        if (d > 180.0) d -= 360.0;
        if (d <= -180.0) d += 360.0;
        east = east && d > 1.0e-6;
        west = west && d < -1.0e-6;
        maxin = std::fabs(d) > maxin ? std::fabs(d) : maxin;
    }
    t.inner = latin && (east || west);
    t.maxstep_inner = maxin;
    return t;
}

// the cuts of a call with window half-width k: a column cut needs the window to span less than half the circle
inline int sb_dist_cuts(const SbDistTraits &t, int k) {
    const bool circle = t.circle && (double)k * t.maxstep < 170.0;
    int cuts = (circle && t.latmono) ? SB_CUT_NEAREST : 0;
    if (circle) cuts |= SB_CUT_CIRCLE;
#ifndef SB_DIST_NO_INNER_CUT                                     // (A/B builds: what the per-target rule buys, tools/dist_wide_cost.py)
    if (t.inner && (double)k * t.maxstep_inner < 170.0) cuts |= SB_CUT_INNER;
#endif
    if (t.latmono) cuts |= SB_CUT_ROWS;
    return cuts;
}

// BYTES: k_dist (byte probes in LDS; a grid narrower than the window).  BITS_SMALL: k_dist_bits_small (a grid narrower than
// 2k + 257 columns, where the staged reach of k_dist_bits' workgroup would wrap round the seam more than once).
// BITS32, BITS64: k_dist_bits with its window in a 32-bit word (k <= 15) or a 64-bit one.  WIDE: k_dist_wide, any nx.
enum class SbDistKernel { BYTES, BITS_SMALL, BITS32, BITS64, WIDE };

inline SbDistKernel sb_dist_kernel(int nx, int k) {
    if (k >= 32) return SbDistKernel::WIDE;
    if (2 * k + 1 > nx) return SbDistKernel::BYTES;
    if (nx < 2 * k + 257) return SbDistKernel::BITS_SMALL;
    return k <= 15 ? SbDistKernel::BITS32 : SbDistKernel::BITS64;
}

// One latitude band of a multi-GPU run in its ghost-celled frame (sb_band_get_dist_*: ny own rows, halo ghost rows on each
// side, frame row halo is the band's first): which frame rows may hold a SOURCE of a window of half-width k -- the band's
// own rows and k ghost rows on each cut side; none beyond a pole, where the globe's source range ends too -- and which of
// those source rows are the targets.  Rows are counted from the first source row on: the kernels, the bit plane, the
// latitude table and sb_dist_traits see source rows 0 .. nys-1 (frame rows f0 .. f0+nys-1) and nothing else of the frame,
// so ghost rows beyond a pole and their latitudes are never read.  The caller holds k <= halo wherever a side is a cut.
struct SbBandRows {
    int f0, nys;     // first source row in the frame, number of source rows
    int r0, r1;      // the targets: source rows r0 .. r1-1
};

inline SbBandRows sb_band_rows(int ny, int halo, bool south, bool north, int k) {
    SbBandRows b;
    b.f0 = south ? halo : halo - k;
    const int f1 = north ? halo + ny : halo + ny + k;
    b.nys = f1 - b.f0;
    b.r0 = halo - b.f0;
    b.r1 = b.r0 + ny;
    return b;
}
