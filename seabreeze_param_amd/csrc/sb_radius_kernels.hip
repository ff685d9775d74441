// sb_radius_kernels.hip -- search_radius: the radius nn at which a band cell's expanding window first holds both a
// land-side and a sea-side cell (ref: generic/sea_breeze_diag.f90:188-214), from mask, maxdist and the boundary rule alone.
// It is contrast_global's nn_used (sb_thc_common.hpp) for every band cell, without its O(nn^3) ring walk: a window is a
// stack of row intervals of one half-width, so
//   k_radius_bits   mask -> land-side and band bit planes in window coordinates (SbRadiusGeo), two device-wide flags, and
//                   per row which words of the land-side plane hold a cell of each class
//   k_radius_rows   per cell of every row a window may read: the column distance to the nearest cell of the other class
//   k_radius_cols   per band cell, nn = 1, 2, ..: rows y-nn and y+nn folded into the nearest land-side and the nearest
//                   sea-side column distance; the first nn that is no smaller than both is the radius
// All three take one wave per 64-cell longitude segment, lanes along longitude.
#include "sb_thc_common.hpp"

#define SB_RADIUS_NT 256
#define SB_RADIUS_HB 1024            // histogram bins a workgroup keeps in LDS; bins beyond go to memory one by one
#define SB_RADIUS_FAR (1 << 28)      // "no such cell": above every radius and every sum of a radius and a lane

namespace {

__device__ __forceinline__ int rad_nbits(const SbRadiusGeo &g, int k) {
    const int n = g.W - k * 64;
    return n > 64 ? 64 : n;
}
__device__ __forceinline__ uint64_t rad_valid(const SbRadiusGeo &g, int k) {
    const int n = rad_nbits(g, k);
    return n == 64 ? ~0ull : ((1ull << n) - 1ull);
}

// A row's word summary: bit k of B (nws words, bits from nw on are zero) says that word k of the row holds a cell of the
// class.  The first such word after word w -- w+1 .. nw-1, then, round the circle, 0 .. w itself -- or -1.
__device__ __forceinline__ int rad_next_word(const uint64_t *B, int nws, int w, int periodic) {
    const int a = w + 1;
    for (int q = a >> 6; q < nws; ++q) {
        uint64_t m = B[q];
        if (q == (a >> 6)) m &= ~0ull << (a & 63);
        if (m) return q * 64 + __builtin_ctzll(m);
    }
    if (periodic)
        for (int q = 0; q <= (w >> 6); ++q) {
            uint64_t m = B[q];
            if (q == (w >> 6) && (w & 63) != 63) m &= (2ull << (w & 63)) - 1ull;
            if (m) return q * 64 + __builtin_ctzll(m);
        }
    return -1;
}
// ... and the last one before word w: w-1 .. 0, then nw-1 .. w itself
__device__ __forceinline__ int rad_prev_word(const uint64_t *B, int nws, int w, int periodic) {
    for (int q = w >> 6; q >= 0; --q) {
        uint64_t m = B[q];
        if (q == (w >> 6)) m &= (1ull << (w & 63)) - 1ull;
        if (m) return q * 64 + 63 - __builtin_clzll(m);
    }
    if (periodic)
        for (int q = nws - 1; q >= (w >> 6); --q) {
            uint64_t m = B[q];
            if (q == (w >> 6)) m &= ~0ull << (w & 63);
            if (m) return q * 64 + 63 - __builtin_clzll(m);
        }
    return -1;
}

// (row, word) of the wave's segment s among the rows [r0, r0 + nrow)
struct RadSeg {
    int Y, w;
};
__device__ __forceinline__ RadSeg rad_seg(const SbRadiusGeo &g, unsigned s, int r0) {
    RadSeg q;
    const unsigned r = s / (unsigned)g.nw;
    q.Y = r0 + (int)r;
    q.w = (int)(s - r * (unsigned)g.nw);
    return q;
}

template <typename T>
__global__ void __launch_bounds__(SB_RADIUS_NT) k_radius_bits(const T *__restrict__ mask, T maxdist, SbRadiusGeo g, int *flags,
                                                              uint64_t *__restrict__ clsp, uint64_t *__restrict__ bandp,
                                                              unsigned long long *sumL, unsigned long long *sumS) {
    const int nws = (g.nw + 63) / 64;
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SB_RADIUS_NT / 64) + (threadIdx.x >> 6));
    const unsigned nwaves = gridDim.x * (SB_RADIUS_NT / 64);
    const unsigned nseg = (unsigned)(g.Y1 - g.Y0) * (unsigned)g.nw;
    for (unsigned s = wave; s < nseg; s += nwaves) {
        const RadSeg q = rad_seg(g, s, g.Y0);
        const int xe = q.w * 64 + lane;
        const bool in = xe < g.W;
        const int X = g.coff + xe, xi = X - g.h, yi = q.Y - g.h;
        const size_t row = (size_t)q.Y * g.ld;
        const T m = mask[row + (in ? X : g.coff)];
        // the wrapper rule never sees its last column: window offsets that land there map to column 0 (sb_map_cell), the
        // centre of a cell in the last column included.  Its band bit is its own.
        T mc = m;
        if (g.bnd == BND_WRAPPER && xe == g.nx - 1) mc = mask[row];
        const bool cls = in && mc >= T(0);                                   // ref :182,200; NaN is sea side
        const bool interior = in && xi >= 0 && xi < g.nx && yi >= 0 && yi < g.ny;
        const bool band = interior && yi < g.rows && !(fabs(m) > maxdist);   // ref :174; NaN is a band cell
        const uint64_t wc = __ballot(cls), wb = __ballot(band);
        if (lane == 0) {
            const size_t o = (size_t)q.Y * g.nw + q.w;
            clsp[o] = wc;
            bandp[o] = wb;
            // the row's word summaries (k_radius_rows finds the nearest word with a cell of a class in them)
            const size_t os = (size_t)q.Y * nws + (q.w >> 6);
            if (wc) { flags[0] = 1; atomicOr(&sumL[os], 1ull << (q.w & 63)); }                 // (flags: benign duplicates)
            if (~wc & rad_valid(g, q.w)) { flags[1] = 1; atomicOr(&sumS[os], 1ull << (q.w & 63)); }
        }
    }
}

__global__ void __launch_bounds__(SB_RADIUS_NT) k_radius_rows(SbRadiusGeo g, const int *__restrict__ flags,
                                                              const uint64_t *__restrict__ clsp, const uint64_t *__restrict__ sumL,
                                                              const uint64_t *__restrict__ sumS, uint16_t *__restrict__ dist) {
    const int nws = (g.nw + 63) / 64;
    if (!(flags[0] && flags[1])) return;             // one class only: k_radius_cols answers from the flags
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SB_RADIUS_NT / 64) + (threadIdx.x >> 6));
    const unsigned nwaves = gridDim.x * (SB_RADIUS_NT / 64);
    const unsigned nseg = (unsigned)(g.Y1 - g.Y0) * (unsigned)g.nw;
    for (unsigned s = wave; s < nseg; s += nwaves) {
        const RadSeg q = rad_seg(g, s, g.Y0);
        const uint64_t *row = clsp + (size_t)q.Y * g.nw;
        const int w = q.w;
        const uint64_t own = row[w], L = own, S = ~own & rad_valid(g, w);
        // wave-uniform: distances from lane 0 of this word to the nearest land-side / sea-side cell in the words to the
        // right and to the left -- round the circle and back into this word where the row is periodic
        int dRL = SB_RADIUS_FAR, dRS = SB_RADIUS_FAR, dLL = SB_RADIUS_FAR, dLS = SB_RADIUS_FAR;
        // the nearest word with such a cell from the rows' word summaries (64 words per step), then that one word
        const uint64_t *bl = sumL + (size_t)q.Y * nws, *bs = sumS + (size_t)q.Y * nws;
        int k;
        if ((k = rad_next_word(bl, nws, w, g.periodic)) >= 0) {
            const int col = k * 64 + __builtin_ctzll(row[k]);
            dRL = k > w ? col - w * 64 : col + g.W - w * 64;
        }
        if ((k = rad_next_word(bs, nws, w, g.periodic)) >= 0) {
            const int col = k * 64 + __builtin_ctzll(~row[k] & rad_valid(g, k));
            dRS = k > w ? col - w * 64 : col + g.W - w * 64;
        }
        if ((k = rad_prev_word(bl, nws, w, g.periodic)) >= 0) {
            const int col = k * 64 + 63 - __builtin_clzll(row[k]);
            dLL = k < w ? w * 64 - col : w * 64 + g.W - col;
        }
        if ((k = rad_prev_word(bs, nws, w, g.periodic)) >= 0) {
            const int col = k * 64 + 63 - __builtin_clzll(~row[k] & rad_valid(g, k));
            dLS = k < w ? w * 64 - col : w * 64 + g.W - col;
        }
        const int xe = w * 64 + lane;
        const bool c = (own >> lane) & 1ull;
        const uint64_t t = c ? S : L;                // the other class in this word
        int dr = SB_RADIUS_FAR, dl = SB_RADIUS_FAR;
        const uint64_t hi = lane == 63 ? 0ull : (t >> (lane + 1));
        if (hi) dr = __builtin_ctzll(hi) + 1;
        else {
            const int far = c ? dRS : dRL;
            if (far != SB_RADIUS_FAR) dr = far - lane;
        }
        const uint64_t lo = t & ((1ull << lane) - 1ull);
        if (lo) dl = lane - (63 - __builtin_clzll(lo));
        else {
            const int far = c ? dLS : dLL;
            if (far != SB_RADIUS_FAR) dl = far + lane;
        }
        const int d = min(min(dr, dl), 65535);
        if (xe < g.W) dist[(size_t)q.Y * g.W + xe] = (uint16_t)d;
    }
}

__global__ void __launch_bounds__(SB_RADIUS_NT) k_radius_cols(SbRadiusGeo g, const int *__restrict__ flags,
                                                              const uint64_t *__restrict__ clsp, const uint64_t *__restrict__ bandp,
                                                              const uint16_t *__restrict__ dist, int *__restrict__ radius,
                                                              unsigned long long *summary, unsigned long long *hist, int nhist) {
    __shared__ unsigned s_hist[SB_RADIUS_HB];
    __shared__ unsigned s_cnt[4];                    // band cells, with a radius, without a window, the largest radius
    for (int i = threadIdx.x; i < SB_RADIUS_HB; i += SB_RADIUS_NT) s_hist[i] = 0;
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const bool both = flags[0] && flags[1];
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (SB_RADIUS_NT / 64) + (threadIdx.x >> 6));
    const unsigned nwaves = gridDim.x * (SB_RADIUS_NT / 64);
    const unsigned nseg = (unsigned)g.ny * (unsigned)g.nw;
    for (unsigned s = wave; s < nseg; s += nwaves) {
        const RadSeg q = rad_seg(g, s, g.h);
        const int w = q.w, xe = w * 64 + lane, x = xe - g.ioff, y = q.Y - g.h;
        const bool interior = xe < g.W && x >= 0 && x < g.nx;
        const uint64_t bw = bandp[(size_t)q.Y * g.nw + w];
        const bool band = interior && ((bw >> lane) & 1ull);
        int r = 0;
        if (band) {
            r = -1;
            int cap = g.nx + g.ny;
            if (g.bnd == BND_HALO) {                 // strip_frame_reach: the ghost width beyond the interior on the sides that are edges
                const int big = 1 << 20;
                const int rx = (g.band & GEO_BAND_EW) ? big : min(x + g.h, g.nx - 1 - x + g.h);
                const int rs = (g.band & GEO_BAND_SOUTH) ? big : y + g.h, rn = (g.band & GEO_BAND_NORTH) ? big : g.ny - 1 - y + g.h;
                cap = min(cap, min(rx, min(rs, rn)));
            }
            if (both && cap >= 1) {
                const size_t col = (size_t)xe;
                const bool c0 = (clsp[(size_t)q.Y * g.nw + w] >> lane) & 1ull;
                int d0 = dist[(size_t)q.Y * g.W + col];
                d0 = d0 == 65535 ? SB_RADIUS_FAR : d0;
                int ml = c0 ? 0 : d0, ms = c0 ? d0 : 0;     // nearest land-side / sea-side column over the rows folded so far
                for (int nn = 1; nn <= cap; ++nn) {
                    // a row beyond a pole is the pole row again (sb_map_cell's clamp), folded when the window reached it;
                    // a row beyond the frame does not exist: both are skipped
                    const int Ya = q.Y - nn, Yb = q.Y + nn;
                    const bool ea = Ya >= g.Y0, eb = Yb < g.Y1;
                    if (!ea && !eb) {                       // every row is in: the window only widens from here on
                        const int need = max(nn, max(ml, ms));
                        if (need <= cap) r = need;
                        break;
                    }
                    if (ea) {
                        const bool cb = (clsp[(size_t)Ya * g.nw + w] >> lane) & 1ull;
                        int dd = dist[(size_t)Ya * g.W + col];
                        dd = dd == 65535 ? SB_RADIUS_FAR : dd;
                        ml = min(ml, cb ? 0 : dd); ms = min(ms, cb ? dd : 0);
                    }
                    if (eb) {
                        const bool cb = (clsp[(size_t)Yb * g.nw + w] >> lane) & 1ull;
                        int dd = dist[(size_t)Yb * g.W + col];
                        dd = dd == 65535 ? SB_RADIUS_FAR : dd;
                        ml = min(ml, cb ? 0 : dd); ms = min(ms, cb ? dd : 0);
                    }
                    if (ml <= nn && ms <= nn) { r = nn; break; }
                }
            }
        }
        if (interior && radius) radius[(size_t)y * g.nx + x] = r;
        const uint64_t mb = __ballot(band);
        if (mb) {                                    // wave-uniform
            const uint64_t mf = __ballot(band && r > 0);
            const int mx = sb_wave_max_to_last(band && r > 0 ? r : 0);
            if (lane == 63) {
                atomicAdd(&s_cnt[0], (unsigned)__popcll(mb));
                atomicAdd(&s_cnt[1], (unsigned)__popcll(mf));
                atomicAdd(&s_cnt[2], (unsigned)__popcll(mb & ~mf));
                atomicMax(&s_cnt[3], (unsigned)mx);
            }
            if (band && hist) {
                const int b = r < 0 ? 0 : min(r, nhist - 1);
                if (b < SB_RADIUS_HB) atomicAdd(&s_hist[b], 1u);
                else atomicAdd(&hist[b], 1ull);
            }
        }
    }
    __syncthreads();
    if (summary && threadIdx.x < 4 && s_cnt[threadIdx.x]) {
        if (threadIdx.x < 3) atomicAdd(&summary[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
        else atomicMax(&summary[3], (unsigned long long)s_cnt[3]);
    }
    if (hist) {
        const int nb = nhist < SB_RADIUS_HB ? nhist : SB_RADIUS_HB;
        for (int b = threadIdx.x; b < nb; b += SB_RADIUS_NT)
            if (s_hist[b]) atomicAdd(&hist[b], (unsigned long long)s_hist[b]);     // one device atomic per non-empty bin
    }
}

inline int rad_grid(unsigned nseg) {
    const unsigned per = SB_RADIUS_NT / 64, nblk = (nseg + per - 1) / per;
    return nblk < 1 ? 1 : nblk > 2048 ? 2048 : (int)nblk;
}

}  // namespace

template <typename T>
hipError_t sb_launch_search_radius(const T *mask, T maxdist, const SbRadiusGeo &g, void *ws, int *radius, long long *summary,
                                   long long *hist, int nhist, hipStream_t st) {
    const size_t nyh = (size_t)g.ny + 2 * (size_t)g.h, plane = nyh * g.nw, sums = nyh * ((g.nw + 63) / 64);
    int *flags = (int *)ws;
    uint64_t *sumL = (uint64_t *)((char *)ws + SB_RADIUS_WS_HDR), *sumS = sumL + sums;
    uint64_t *clsp = sumS + sums, *bandp = clsp + plane;
    uint16_t *dist = (uint16_t *)(bandp + plane);
    hipError_t e;
    if ((e = hipMemsetAsync(ws, 0, SB_RADIUS_WS_HDR + 2 * sums * sizeof(uint64_t), st)) != hipSuccess) return e;   // flags, summaries
    if (summary && (e = hipMemsetAsync(summary, 0, 4 * sizeof(long long), st)) != hipSuccess) return e;
    if (hist && (e = hipMemsetAsync(hist, 0, (size_t)nhist * sizeof(long long), st)) != hipSuccess) return e;
    const unsigned nseg_f = (unsigned)(g.Y1 - g.Y0) * (unsigned)g.nw, nseg_i = (unsigned)g.ny * (unsigned)g.nw;
    k_radius_bits<T><<<rad_grid(nseg_f), SB_RADIUS_NT, 0, st>>>(mask, maxdist, g, flags, clsp, bandp, (unsigned long long *)sumL,
                                                                (unsigned long long *)sumS);
    k_radius_rows<<<rad_grid(nseg_f), SB_RADIUS_NT, 0, st>>>(g, flags, clsp, sumL, sumS, dist);
    k_radius_cols<<<rad_grid(nseg_i), SB_RADIUS_NT, 0, st>>>(g, flags, clsp, bandp, dist, radius, (unsigned long long *)summary,
                                                             (unsigned long long *)hist, hist ? nhist : 0);
    return hipGetLastError();
}

template hipError_t sb_launch_search_radius<float>(const float *, float, const SbRadiusGeo &, void *, int *, long long *,
                                                   long long *, int, hipStream_t);
template hipError_t sb_launch_search_radius<double>(const double *, double, const SbRadiusGeo &, void *, int *, long long *,
                                                    long long *, int, hipStream_t);
