// sb_guard_kernels.hip -- the opt-in guard for missing and non-finite temperatures (sb_set_nonfinite_guard) on gfx950.
//
// Every contrast kernel but the global-memory search assumes |t0| < 2048 K: the strip kernels and the tables put t0 into
// 64-bit fixed point, the tile kernel keeps fp64 prefix sums about a per-tile offset.  A NaN, an Inf or the 2.0e20 missing
// value in theta (or z) leaves garbage in exactly the windows that hold the cell -- the fixed-point sums wrap, so whatever
// bits the cell turns into cancel in the corner difference of a window that does not hold it; the tile kernel's
// floating-point sums do not cancel, so there the whole tile that staged the cell is lost.  The reference
// (generic/sea_breeze_diag.f90:198-216) lets the value flow into the window means.  With the guard on, a whole call
// finds the band cells whose contrast may be wrong and computes those again the reference's way, between the contrast
// kernel and k_wind.  Four launches, all unconditional, no host synchronisation; without a bad cell three of them leave at once.
//
//   k_guard_bits    one coalesced pass over theta and z on the whole ghost-celled frame, ahead of everything else of the
//                   call: a cell is bad iff !(|theta| + gmma |z| < 2048) -- the smoothed sigma lies in [0, 1], so this bounds
//                   |t0| without the sigmoid scalars, and it holds for NaN.  One ballot word per 64-cell segment (the layout
//                   of bandbits / clsbits); the number of bad cells by one ticket per workgroup, summed by the last arriver.
//   k_guard_taint   <0>: along longitude.  Per frame row, bit x of the result: the cells a window of reach R round interior
//                   column x reads in this row (the call's boundary rule, exactly) hold a bad cell.  <1>: along latitude.
//                   Per segment, band cells only: one of the rows a window round row y reads has its bit set in <0>'s
//                   result -- the windows are squares and the boundary rules map columns and rows apart, so the two
//                   passes give exactly "the window of reach R holds a bad cell".  By tile (k_thc3): the span of a
//                   cell is that of its tile plus the LDS halo in both passes, the tile's staged rectangle.  <1> writes
//                   over the bad plane (nobody reads it any more) and counts the tainted band cells.
//   k_guard_repair  walks the tainted plane in chunks of 128 segments, compacts the set cells in LDS so that every lane
//                   has one, and per cell searches nn as contrast_global does (same cap, same geometry), sums plain t0 per
//                   class in double -- NOT about the centre cell: with a centre of +Inf every term of contrast_global's sum
//                   is NaN where the reference gives +-Inf -- and writes mul (T)(sl/nl - ss/ns) to thc.
//
// sb_set_nonfinite_guard_bands beside it: the calls in which the contrast kernel applies thresholds and state update itself
// (phase 2 of a band step, a call with gathered moments).  That update overwrites ws / wd, the state of the step before, so
// nothing behind it can form sb_con again from what is left.  The taint needs theta, z, the band plane and the reach only:
// there the three passes above run AHEAD of the contrast kernel, the latitude pass in a second instance (STASH) that copies
// ws / wd of every tainted band cell into two stash planes, and k_guard_repair<T, true> behind the contrast kernel hands the
// contrast of a cell to sb_trigger_update with the stashed state and the winds k_wind left in the scratch planes: thc and
// sb_con are written over, ws / wd come out as the contrast kernel left them (they do not depend on thc).
#include "sb_thc_common.hpp"
#include <type_traits>

static_assert(SB_GUARD_REACH_TABLE == SB_TAB_REACH, "the guard dilates by the tables' reach");

#define GUARD_NT 256
#define GUARD_CHUNK 128             // segments of the tainted plane a repair workgroup compacts at a time

// `cnt` of this workgroup (thread 0's) -> partials; the last workgroup to arrive returns true in all its threads, with the
// total in `total`.  Hand-over as in k_stats: write-through stores, drained, then the ticket; read past the caches.
__device__ __forceinline__ bool guard_last_total(unsigned cnt, unsigned *partials, unsigned *ticket, unsigned *s_red, unsigned &total) {
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __hip_atomic_store(&partials[blockIdx.x], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1 ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return false;
    unsigned a = 0;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += GUARD_NT) a += __hip_atomic_load(&partials[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_red[threadIdx.x] = a;
    __syncthreads();
    for (int s = GUARD_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
        __syncthreads();
    }
    total = s_red[0];
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (zeroed at allocation; every launch leaves it zero)
    return true;
}

template <typename T>
__global__ __launch_bounds__(GUARD_NT) void k_guard_bits(const T *__restrict__ theta, const T *__restrict__ z, int nxh, int nyh, int nw,
                                                        uint64_t *__restrict__ bad, unsigned *__restrict__ rep, int rep_reset) {
    __shared__ unsigned s_red[GUARD_NT];
    const int lane = threadIdx.x & 63;
    const unsigned nseg = (unsigned)nyh * (unsigned)nw;
    const unsigned wave = blockIdx.x * (GUARD_NT / SB_WAVE) + (threadIdx.x >> 6), nwave = gridDim.x * (GUARD_NT / SB_WAVE);
    unsigned cnt = 0;                                    // (wave-uniform)
    for (unsigned sg0 = wave; sg0 < nseg; sg0 += 4 * nwave) {       // four segments' loads in flight per wave
        T th[4], zz[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned sg = sg0 + (unsigned)q * nwave, Y = sg / (unsigned)nw, X = (sg - Y * (unsigned)nw) * 64u + (unsigned)lane;
            const bool live = sg < nseg && X < (unsigned)nxh;
            const size_t i = live ? (size_t)Y * nxh + X : 0;
            th[q] = live ? theta[i] : T(0);
            zz[q] = live ? z[i] : T(0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned sg = sg0 + (unsigned)q * nwave;
            if (sg >= nseg) break;                       // (wave-uniform)
            const uint64_t w = __ballot(!(fabs(th[q]) + T(0.0060956) * fabs(zz[q]) < T(2048)));
            if (lane == 0) bad[sg] = w;
            cnt += (unsigned)__popcll(w);
        }
    }
    s_red[threadIdx.x] = lane == 0 ? cnt : 0u;
    __syncthreads();
    if (threadIdx.x == 0) cnt = s_red[0] + s_red[64] + s_red[128] + s_red[192];
    __syncthreads();
    unsigned total;
    if (!guard_last_total(cnt, rep + SB_GUARD_REP_PART, rep + SB_GUARD_REP_TICKET, s_red, total)) return;
    if (threadIdx.x == 0) {
        rep[0] = total;
        const unsigned found = total ? 1u : 0u;
        rep[2] = rep_reset ? found : rep[2] + found;
    }
}

// does row `row` of the bad plane hold a set bit among frame columns a .. b (0 <= a, b < 64 nw)?
__device__ __forceinline__ bool guard_range_any(const uint64_t *__restrict__ row, int a, int b) {
    if (a > b) return false;
    const int wa = a >> 6, wb = b >> 6;
    bool any = false;
    for (int w = wa; w <= wb; ++w) {
        uint64_t m = ~0ull;
        if (w == wa) m &= ~0ull << (a & 63);
        if (w == wb) m &= ~0ull >> (63 - (b & 63));
        any = any || (row[w] & m) != 0;
    }
    return any;
}

// the span of a window (reach R) round cell c along one axis, or of the staged rectangle of c's tile (tile > 1)
__device__ __forceinline__ void guard_span(int c, int R, int tile, int &lo, int &hi) {
    const int c0 = tile > 1 ? c - c % tile : c;
    lo = c0 - R;
    hi = c0 + (tile > 1 ? tile - 1 : 0) + R;
}

// PASS 0: bad -> out, along longitude, one wave per frame row.  PASS 1: hd (pass 0's result) -> out, along latitude, one wave
// per segment, band cells only; counts them.  R: the reach; tile: the tiles' width (pass 0) or rows (pass 1), 1: by cell.
// STASH (pass 1 only): every lane whose bit is set puts ws / wd of its cell aside (T: the planes' type; void: no stash).
template <typename T>
struct GuardStash {
    const T *ws, *wd;               // the carried state, (nx, ny)
    T *sws, *swd;                   // the stash planes, (nx, ny)
};
template <>
struct GuardStash<void> {};

template <int PASS, typename T>
__device__ __forceinline__ void guard_taint_body(const Geo &g, const uint64_t *__restrict__ src, uint64_t *__restrict__ out,
                                                 const uint64_t *__restrict__ bandbits, int R, int tile, unsigned *__restrict__ rep,
                                                 const GuardStash<T> &stash) {
    __shared__ unsigned s_red[GUARD_NT];
    if (rep[0] == 0) {                                   // no bad cell in the frame: nothing is read, nothing repaired
        if (PASS == 1 && blockIdx.x == 0 && threadIdx.x == 0) rep[1] = 0;
        return;
    }
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * (GUARD_NT / SB_WAVE) + (threadIdx.x >> 6), nwave = gridDim.x * (GUARD_NT / SB_WAVE);
    if constexpr (PASS == 0) {
        for (unsigned Y = wave; Y < (unsigned)g.nyh; Y += nwave) {
            const uint64_t *row = src + (size_t)Y * g.nw;
            uint64_t acc = 0;
            for (int w = lane; w < g.nw; w += 64) acc |= row[w];
            const bool dirty = __ballot(acc != 0) != 0;
            for (int w = 0; w < g.nw; ++w) {
                bool t = false;
                const int x = w * 64 + lane - g.h;       // interior column of this lane's bit
                if (dirty && x >= 0 && x < g.nx) {
                    int lo, hi;
                    guard_span(x, R, tile, lo, hi);
                    if (g.bnd == BND_HALO) t = guard_range_any(row, max(lo + g.h, 0), min(hi + g.h, g.nxh - 1));
                    else {
                        // periodic over the effective row: the frame's nx columns, or (the wrapper's index rule, sb_map_cell) its
                        // columns 0 .. nx-2 with column 0 once more in the last place -- that rule never reads column nx-1
                        const int last = g.bnd == BND_WRAPPER ? max(g.nx - 2, 0) : g.nx - 1;
                        if (hi - lo + 1 >= g.nx) t = guard_range_any(row, 0, last);
                        else {
                            int a = lo % g.nx, b = hi % g.nx;
                            if (a < 0) a += g.nx;
                            if (b < 0) b += g.nx;
                            if (a <= b) t = guard_range_any(row, a, min(b, last)) || (b > last && (row[0] & 1ull));
                            else t = guard_range_any(row, a, last) || (g.nx - 1 > last && (row[0] & 1ull)) || guard_range_any(row, 0, min(b, last));
                        }
                    }
                }
                const uint64_t m = __ballot(t);
                if (lane == 0) out[(size_t)Y * g.nw + w] = m;
            }
        }
    } else {
        const unsigned nseg = (unsigned)g.nyh * (unsigned)g.nw;
        unsigned cnt = 0;
        for (unsigned sg = wave; sg < nseg; sg += nwave) {
            const uint64_t band = bandbits[sg];
            uint64_t acc = 0;
            if (band) {                                  // (wave-uniform)
                const int Y = (int)(sg / (unsigned)g.nw), w = (int)(sg - (unsigned)Y * (unsigned)g.nw);
                int lo, hi;
                guard_span(Y - g.h, R, tile, lo, hi);
                for (int ys = lo + lane; ys <= hi; ys += 64) {
                    int Ys;
                    if (g.bnd == BND_HALO) { Ys = ys + g.h; if (Ys < 0 || Ys >= g.nyh) continue; }
                    else Ys = ys < 0 ? 0 : (ys >= g.ny ? g.ny - 1 : ys);
                    acc |= src[(size_t)Ys * g.nw + w];
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned lo32 = __shfl_xor((unsigned)acc, off), hi32 = __shfl_xor((unsigned)(acc >> 32), off);
                    acc |= ((uint64_t)hi32 << 32) | lo32;
                }
                acc &= band;
                if constexpr (!std::is_void<T>::value) {
                    if ((acc >> lane) & 1ull) {          // (band cells are interior cells)
                        const size_t o = (size_t)(Y - g.h) * g.nx + (size_t)(w * 64 + lane - g.h);
                        stash.sws[o] = stash.ws[o];
                        stash.swd[o] = stash.wd[o];
                    }
                }
            }
            if (lane == 0) out[sg] = acc;
            cnt += (unsigned)__popcll(acc);
        }
        s_red[threadIdx.x] = lane == 0 ? cnt : 0u;
        __syncthreads();
        if (threadIdx.x == 0) cnt = s_red[0] + s_red[64] + s_red[128] + s_red[192];
        __syncthreads();
        unsigned total;
        if (!guard_last_total(cnt, rep + SB_GUARD_REP_PART, rep + SB_GUARD_REP_TICKET, s_red, total)) return;
        if (threadIdx.x == 0) rep[1] = total;
    }
}

template <int PASS>
__global__ __launch_bounds__(GUARD_NT) void k_guard_taint(Geo g, const uint64_t *__restrict__ src, uint64_t *__restrict__ out,
                                                         const uint64_t *__restrict__ bandbits, int R, int tile, unsigned *__restrict__ rep) {
    guard_taint_body<PASS, void>(g, src, out, bandbits, R, tile, rep, GuardStash<void>{});
}
// the latitude pass ahead of a contrast kernel that applies the update itself
template <typename T>
__global__ __launch_bounds__(GUARD_NT) void k_guard_taint_stash(Geo g, const uint64_t *__restrict__ src, uint64_t *__restrict__ out,
                                                               const uint64_t *__restrict__ bandbits, int R, int tile,
                                                               unsigned *__restrict__ rep, GuardStash<T> stash) {
    guard_taint_body<1, T>(g, src, out, bandbits, R, tile, rep, stash);
}

// one tainted band cell, the reference's way: generic/sea_breeze_diag.f90:188-216.  -> its contrast
template <typename T>
__device__ __forceinline__ T guard_repair_cell(const DiagJob<T> &job, int x, int y, T sd, T rr) {
    const Geo &g = job.g;
    int cap = g.nx + g.ny;                               // (contrast_global's callers: strip_slow_cell, k_thc3, k_table_query)
    if (g.bnd == BND_HALO) cap = min(cap, min(min(x + g.h, g.nx - 1 - x + g.h), min(y + g.h, g.ny - 1 - y + g.h)));
    int X, Y;
    bool has_l = false, has_s = false;
    if (sb_map_cell(g, x, y, X, Y)) {
        if (sb_bit(job.clsbits, g.nw, X, Y)) has_l = true; else has_s = true;
    }
    int nn = 0;
    while (nn < cap) {
        ++nn;
        for (int e = -nn; e <= nn; ++e) {
            const int xs[4] = {x + e, x + e, x - nn, x + nn};
            const int ys[4] = {y - nn, y + nn, y + e, y + e};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (sb_map_cell(g, xs[q], ys[q], X, Y)) {
                    if (sb_bit(job.clsbits, g.nw, X, Y)) has_l = true; else has_s = true;
                }
        }
        if (has_l && has_s) break;
    }
    double sl = 0.0, ss = 0.0, nl = 0.0, ns = 0.0;
    for (int yy = y - nn; yy <= y + nn; ++yy)
        for (int xx = x - nn; xx <= x + nn; ++xx) {
            if (!sb_map_cell(g, xx, yy, X, Y)) continue;
            const double t = (double)cell_t0(job, (size_t)Y * g.nxh + X, sd, rr);
            if (sb_bit(job.clsbits, g.nw, X, Y)) { sl += t; nl += 1.0; } else { ss += t; ns += 1.0; }
        }
    const T mul = sb_bit(job.clsbits, g.nw, x + g.h, y + g.h) ? T(1) : T(-1);
    return mul * (T)(sl / nl - ss / ns);                 // 0/0 -> NaN when a class is missing
}

// UPD: the contrast kernel applied thresholds and state update (and wrote over ws / wd): apply them again with the state the
// latitude pass put aside and this call's winds in the scratch planes -- ws / wd come out as they are, thc and sb_con anew
template <typename T, bool UPD>
__global__ __launch_bounds__(GUARD_NT) void k_guard_repair(DiagJob<T> job, const uint64_t *__restrict__ taint, const unsigned *__restrict__ rep,
                                                          const T *__restrict__ sws, const T *__restrict__ swd) {
    if (rep[0] == 0) return;
    __shared__ int s_scan[GUARD_NT / SB_WAVE];
    __shared__ unsigned short s_list[GUARD_CHUNK * 64];
    const Geo &g = job.g;
    const unsigned nseg = (unsigned)g.nyh * (unsigned)g.nw, nchunk = (nseg + GUARD_CHUNK - 1) / GUARD_CHUNK;
    const T sd = job.t0_fly ? job.stats[0] : T(0), rr = job.t0_fly ? job.stats[1] : T(0);
    for (unsigned ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const unsigned sg0 = ch * GUARD_CHUNK, mine = sg0 + threadIdx.x;
        const uint64_t w = threadIdx.x < GUARD_CHUNK && mine < nseg ? taint[mine] : 0ull;
        int total;
        int at = thc_block_excl_scan<GUARD_NT>(__popcll(w), s_scan, total);
        for (uint64_t r = w; r; r &= r - 1) s_list[at++] = (unsigned short)((threadIdx.x << 6) | (unsigned)__builtin_ctzll(r));
        __syncthreads();
        for (int i = threadIdx.x; i < total; i += GUARD_NT) {
            const unsigned code = s_list[i], sg = sg0 + (code >> 6);
            const int Y = (int)(sg / (unsigned)g.nw), X = (int)(sg - (unsigned)Y * (unsigned)g.nw) * 64 + (int)(code & 63u);
            const int x = X - g.h, y = Y - g.h;
            const size_t o = (size_t)y * g.nx + x;
            const T n_thc = guard_repair_cell<T>(job, x, y, sd, rr);
            if constexpr (UPD) sb_trigger_update<T>(job, o, n_thc, SbCellState<T>{job.nws[o], job.nwd[o], sws[o], swd[o]});
            else job.thc[o] = n_thc;
        }
        __syncthreads();                                 // (s_list is written again)
    }
}

static int guard_grid(unsigned nwaves_of_work, int ncu) {
    const unsigned per = GUARD_NT / SB_WAVE, want = (nwaves_of_work + per - 1) / per, cap = (unsigned)min(ncu * 8, SB_GUARD_MAX_WGS);
    return (int)(want < 1 ? 1 : want > cap ? cap : want);
}

template <typename T>
hipError_t sb_launch_guard_bits(const DiagJob<T> &job, const SbGuard &gd, int ncu, hipStream_t st) {
    const Geo &g = job.g;
    const unsigned nseg = (unsigned)g.nyh * (unsigned)g.nw;
    hipLaunchKernelGGL(k_guard_bits<T>, dim3(guard_grid((nseg + 3) / 4, ncu)), dim3(GUARD_NT), 0, st, job.theta, job.z, g.nxh, g.nyh, g.nw,
                       gd.bad, gd.rep, gd.rep_reset);
    return hipGetLastError();
}

// the two taint passes; gp.taint_before >= 0: ahead of the contrast kernel, with the stash
template <typename T>
hipError_t sb_launch_guard_taint(const DiagJob<T> &job, const SbGuardPlan &gp, const SbGuard &gd, int ncu, hipStream_t st) {
    const Geo &g = job.g;
    const bool by_tile = gp.reach == SB_GUARD_BY_TILE;
    const int R = by_tile ? gp.halo : gp.reach;
    const unsigned nseg = (unsigned)g.nyh * (unsigned)g.nw;
    hipLaunchKernelGGL(k_guard_taint<0>, dim3(guard_grid((unsigned)g.nyh, ncu)), dim3(GUARD_NT), 0, st, g, (const uint64_t *)gd.bad, gd.taint,
                       (const uint64_t *)job.bandbits, R, by_tile ? gp.tile_w : 1, gd.rep);
    if (gp.taint_before >= 0) {
        if (!gd.stash_ws || !gd.stash_wd) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_guard_taint_stash<T>, dim3(guard_grid(nseg, ncu)), dim3(GUARD_NT), 0, st, g, (const uint64_t *)gd.taint, gd.bad,
                           (const uint64_t *)job.bandbits, R, by_tile ? gp.tile_rows : 1, gd.rep,
                           GuardStash<T>{job.ws, job.wd, (T *)gd.stash_ws, (T *)gd.stash_wd});
    } else
        hipLaunchKernelGGL(k_guard_taint<1>, dim3(guard_grid(nseg, ncu)), dim3(GUARD_NT), 0, st, g, (const uint64_t *)gd.taint, gd.bad,
                           (const uint64_t *)job.bandbits, R, by_tile ? gp.tile_rows : 1, gd.rep);
    return hipGetLastError();
}

template <typename T>
hipError_t sb_launch_guard_repair(const DiagJob<T> &job, const SbGuardPlan &gp, const SbGuard &gd, int ncu, hipStream_t st) {
    const Geo &g = job.g;
    const unsigned nseg = (unsigned)g.nyh * (unsigned)g.nw, nchunk = (nseg + GUARD_CHUNK - 1) / GUARD_CHUNK;
    const dim3 grid((int)min(nchunk, (unsigned)(ncu * 4)));
    if (gp.update) {
        if (!gd.stash_ws || !gd.stash_wd || !job.nws || !job.nwd) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_guard_repair<T, true>), grid, dim3(GUARD_NT), 0, st, job, (const uint64_t *)gd.bad, (const unsigned *)gd.rep,
                           (const T *)gd.stash_ws, (const T *)gd.stash_wd);
    } else
        hipLaunchKernelGGL((k_guard_repair<T, false>), grid, dim3(GUARD_NT), 0, st, job, (const uint64_t *)gd.bad, (const unsigned *)gd.rep,
                           (const T *)nullptr, (const T *)nullptr);
    return hipGetLastError();
}

template hipError_t sb_launch_guard_bits<float>(const DiagJob<float> &, const SbGuard &, int, hipStream_t);
template hipError_t sb_launch_guard_bits<double>(const DiagJob<double> &, const SbGuard &, int, hipStream_t);
template hipError_t sb_launch_guard_taint<float>(const DiagJob<float> &, const SbGuardPlan &, const SbGuard &, int, hipStream_t);
template hipError_t sb_launch_guard_taint<double>(const DiagJob<double> &, const SbGuardPlan &, const SbGuard &, int, hipStream_t);
template hipError_t sb_launch_guard_repair<float>(const DiagJob<float> &, const SbGuardPlan &, const SbGuard &, int, hipStream_t);
template hipError_t sb_launch_guard_repair<double>(const DiagJob<double> &, const SbGuardPlan &, const SbGuard &, int, hipStream_t);
