// sb_table_kernels.hip -- the land-sea contrast from DEVICE-WIDE summed-area tables (sb_set_table_contrast): the strip
// kernels' idea -- exact fixed-point tables of t0, of land-side t0 and of the land-side count, four reads per table
// per window -- lifted from LDS to device memory, so that the cost of a band cell does not depend on the radius of its
// window.   ref: generic/sea_breeze_diag.f90:188-216
//
//   k_table_rows   one wave per frame row: t0 (the one sequence, sb_t0) -> fixed point, rounded once (SB_TAB_FB, sb_launch.hpp)
//                  -> inclusive prefix along longitude of {all, land side, land-side count} by DPP scans with a carry
//                  between the 64-cell segments of the row.  The SB_TAB_RB waves of a workgroup add their prefixed rows
//                  up per column (LDS atomics, 1024 columns at a time): S, the block sums the column pass starts from.
//                  A second form for the f2py flavour (sb_set_table_contrast_f2py): the tables over the wrapper rule's
//                  effective row, and the t0 plane written here (no k_t0 in such a call).
//   k_table_cols   prefix along latitude, in place, BLOCKED: a workgroup takes 256 columns x 64 rows, starts from the sum of
//                  the blocks of S above it (independent loads, a few dozen) and walks its rows with eight rows of loads
//                  in flight.  Lanes run along longitude: every access is a whole line.  (One chain per column over all
//                  rows would leave nxh threads alive; a march of whole column strips a few hundred waves.)
//   k_table_query  one wave per listed 64-cell segment (k_prep's lists, as k_wind), band lanes active: the smallest radius
//                  whose square holds both classes by galloping and bisection on the count table alone, then the two
//                  window sums, the means, thc.  Cells the tables cannot answer take contrast_global, here.  Two
//                  instances: where k_wind follows with the update (a whole call) the query leaves thc; where k_wind ran
//                  ahead and left its winds in the scratch planes (a band step, gathered moments:
//                  sb_set_table_contrast_bands) it applies thresholds and state update to every band cell itself, the
//                  four state loads issued ahead of the count probes.
// The sums are wrapping unsigned adds: a window sum is the exact sum of once-rounded values, whatever the launch geometry.
//
// sb_set_table_window_cache: the radius of a band cell's window and the land-side cells in it follow from the land-side
// plane and the geometry alone, so a call that searches ("fills") leaves them in plane W and the calls after it, while
// k_scan finds both planes standing, neither build nor read the count table: the two passes move 16 instead of 20 bytes
// per frame cell, the query one word of W instead of about ten dependent probes of C.  Fill or not is one predicate
// (sb_tab_fill, sb_launch.hpp), uniform over each launch and the same in all three.  The row and the column pass are
// compiled in both forms and pick one at their top -- with the switch off, the form that builds C is the code as it was.
// The query has one form: a launch-uniform branch in the band-cell body takes the search or the word of W, and both
// meet again at tab_window (four to five registers more than without the switch, the same occupancy, no scratch).
#include "sb_thc_common.hpp"
#include "sb_strip_common.hpp"

#define TAB_ROWS_NT (SB_TAB_RB * SB_WAVE)
#define TAB_CH 16                  // segments of a row between two hand-overs of block sums (TAB_CH * 64 == TAB_ROWS_NT columns)
#define TAB_COLS_NT 256
#define TAB_CB 64                  // rows of a block of the column pass
#define TAB_QUERY_NT 256
static_assert(TAB_CH * SB_WAVE == TAB_ROWS_NT, "one thread per column of a chunk");
static_assert(TAB_CB % SB_TAB_RB == 0 && (TAB_CB / SB_TAB_RB) % 4 == 0, "a block of the column pass is whole blocks of S, four at a time");

// t0 (K) -> fixed point: fma rounds x * 2^F + 1.5 * 2^52 to an integer held in the mantissa (|x| < 2048 K; beyond, and for
// NaN, the windows that hold the cell are garbage, not a fault -- and only those: the sums wrap); the bias is taken out here
__device__ __forceinline__ u64 tab_fixed(double x) {
    return (u64)__double_as_longlong(__builtin_fma(x, (double)(1ll << SB_TAB_FB), 0x1.8p52)) - 0x4338000000000000ull;
}
__device__ __forceinline__ u64 tab_readlane63(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((u64)hi << 32) | lo;
}

// ---- the row pass
// WR, the f2py flavour's form (sb_set_table_contrast_f2py; SB_BND_WRAPPER, no ghost cells): the wrapper's column rule
// max(1, modulo(jj, nlons)) never reads its last column -- an offset that lands there, the centre of a last-column cell
// included, reads column 0 (sb_map_cell) -- so a window is a truly periodic one over the EFFECTIVE row, whose last column
// holds column 0's value and land-side bit: those enter the three sums at frame column nx - 1 (one more load of theta, z,
// sigma per row, the same address in every lane), and tab_window's periodic branch serves the rule unchanged.  t0 is an
// output of this flavour: the pass forms it itself (the one sequence, sb_t0) and writes the plane k_t0 would -- the whole
// frame for contrast_global, rows 1 .. nlats - 1 of `output`, the REAL value at column nx - 1 -- so such a call launches no k_t0.
template <typename T, bool WC, bool WR>                  // WC: with the count table
__device__ __forceinline__ void tab_rows_body(const DiagJob<T> &job, const SbTables &tb, u64 *sA, u64 *sL, unsigned *sC) {
    const Geo g = job.g;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Y = __builtin_amdgcn_readfirstlane((int)blockIdx.x * SB_TAB_RB + wv);
    const bool rowok = Y < g.nyh;                        // (wave-uniform; the waves beyond the frame only keep the barriers)
    const size_t row = (size_t)(rowok ? Y : g.nyh - 1) * g.nxh;
    const uint64_t *cls = job.clsbits + (size_t)(rowok ? Y : g.nyh - 1) * g.nw;
    const T sd = job.stats[0], rr = job.stats[1];
    u64 carA = 0, carL = 0;
    unsigned carC = 0;
    // (WR) what the effective row holds in its last column: column 0's value and bit
    u64 eff_a = 0;
    bool eff_land = false;
    if constexpr (WR) {
        eff_a = tab_fixed((double)sb_t0<T>(job.theta[row], job.z[row], job.sigma[row], sd, rr));
        eff_land = (cls[0] & 1ull) != 0ull;
    }
    struct In { T th, zz, sg; uint64_t word; };
    auto issue = [&](int w) {                            // every load unconditional, from a clamped address
        const int X = min(w * 64 + lane, g.nxh - 1);
        In r;
        r.th = (WR || job.t0_fly) ? job.theta[row + X] : job.t0[row + X];
        r.zz = job.z[row + X]; r.sg = job.sigma[row + X];
        r.word = cls[min(w, g.nw - 1)];
        return r;
    };
    auto segment = [&](int w, const In &r) {
        const int X = w * 64 + lane;
        const bool in = X < g.nxh;
        const T t0v = (WR || job.t0_fly) ? sb_t0<T>(r.th, r.zz, r.sg, sd, rr) : r.th;
        bool land = ((r.word >> lane) & 1ull) != 0ull;                // (no bits beyond the frame: k_scan)
        u64 a = in ? tab_fixed((double)t0v) : 0ull;
        if constexpr (WR) {
            if (in) {                                                 // (k_t0's two stores: no ghost cells, g.nxh == g.nx)
                job.t0[row + X] = t0v;
                if (job.out && Y < g.rows) job.out[(size_t)g.nx * g.ny + row + X] = t0v;
            }
            if (X == g.nx - 1) { a = eff_a; land = eff_land; }
        }
        u64 l = land ? a : 0ull;
        int c = land ? 1 : 0;
        sb_scan2_u64(a, l);                              // (all 64 lanes)
        if (WC) c = sb_wave_scan_add(c);
        a += carA; l += carL;
        const unsigned cc = (unsigned)c + carC;
        carA = tab_readlane63(a); carL = tab_readlane63(l);
        if (WC) carC = (unsigned)__builtin_amdgcn_readlane((int)cc, 63);
        if (in) {
            tb.A[row + X] = a; tb.L[row + X] = l;
            if (WC) tb.C[row + X] = cc;
            const int k = X & (TAB_ROWS_NT - 1);
            atomicAdd((unsigned long long *)&sA[k], (unsigned long long)a);
            atomicAdd((unsigned long long *)&sL[k], (unsigned long long)l);
            if (WC) atomicAdd(&sC[k], cc);
        }
    };
    for (int w0 = 0; w0 < g.nw; w0 += TAB_CH) {
        sA[tid] = 0; sL[tid] = 0;                        // (this thread read its column of the chunk before: see below)
        if (WC) sC[tid] = 0;
        __syncthreads();
        if (rowok) {
            const int w1 = min(w0 + TAB_CH, g.nw);
            In cur = issue(w0);
            for (int w = w0; w < w1; ++w) {
                const In nxt = issue(min(w + 1, w1 - 1));        // the next segment travels under this one's logistic
                segment(w, cur);
                cur = nxt;
            }
        }
        __syncthreads();
        const int X = w0 * 64 + tid;
        if (X < g.nxh) {
            const size_t si = (size_t)blockIdx.x * g.nxh + X;
            tb.SA[si] = sA[tid]; tb.SL[si] = sL[tid];
            if (WC) tb.SC[si] = sC[tid];
        }
    }
}
template <typename T, bool WR>                           // (the host picks the form: the host-model instances are the code as it was)
__global__ __launch_bounds__(TAB_ROWS_NT) void k_table_rows(DiagJob<T> job, SbTables tb) {
    __shared__ u64 sA[TAB_ROWS_NT], sL[TAB_ROWS_NT];
    __shared__ unsigned sC[TAB_ROWS_NT];
    const bool fill = sb_tab_fill(tb);                   // (k_scan of this call has finished: uniform over the launch)
    // sb_table_cache_report [2]: calls that searched
    if (tb.W && blockIdx.x == 0 && threadIdx.x == 0) tb.rep[0] = (tb.rep_reset ? 0u : tb.rep[0]) + (fill ? 1u : 0u);
    if (fill) tab_rows_body<T, true, WR>(job, tb, sA, sL, sC);
    else tab_rows_body<T, false, WR>(job, tb, sA, sL, sC);
}

// ---- the column pass
template <bool WC>
__device__ __forceinline__ void tab_cols_body(int nxh, int nyh, int nbx, const SbTables &tb) {
    const int bx = (int)(blockIdx.x % (unsigned)nbx), b = (int)(blockIdx.x / (unsigned)nbx);
    const int X = bx * TAB_COLS_NT + (int)threadIdx.x;
    if (X >= nxh) return;
    u64 ra = 0, rl = 0;
    unsigned rc = 0;
    const int nsb = b * (TAB_CB / SB_TAB_RB);            // blocks of S above this block: a multiple of four
    for (int j = 0; j < nsb; j += 4) {
        u64 a[4], l[4];
        unsigned c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t si = (size_t)(j + q) * nxh + X;
            a[q] = tb.SA[si]; l[q] = tb.SL[si];
            c[q] = WC ? tb.SC[si] : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { ra += a[q]; rl += l[q]; rc += c[q]; }
    }
    const int Y0 = b * TAB_CB, Y1 = min(Y0 + TAB_CB, nyh);
    for (int Ys = Y0; Ys < Y1; Ys += 8) {
        u64 a[8], l[8];
        unsigned c[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const size_t i = (size_t)min(Ys + q, Y1 - 1) * nxh + X;
            a[q] = tb.A[i]; l[q] = tb.L[i];
            c[q] = WC ? tb.C[i] : 0u;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (Ys + q < Y1) {
                const size_t i = (size_t)(Ys + q) * nxh + X;
                ra += a[q]; rl += l[q]; rc += c[q];
                tb.A[i] = ra; tb.L[i] = rl;
                if (WC) tb.C[i] = rc;
            }
        }
    }
}
__global__ __launch_bounds__(TAB_COLS_NT) void k_table_cols(int nxh, int nyh, int nbx, SbTables tb) {
    if (sb_tab_fill(tb)) tab_cols_body<true>(nxh, nyh, nbx, tb);
    else tab_cols_body<false>(nxh, nyh, nbx, tb);
}

// ---- the query
// The square of radius nn round interior cell (x, y) as rectangles of the frame -- sb_map_cell's rule for the two boundary
// modes the tables serve.  SB_BND_HALO (Geo::band == 0): no wrap, no clamp, the caller keeps nn within the frame reach.
// SB_BND_GLOBAL: longitude periodic, at most two column ranges while 2 nn + 1 <= nx; latitude clamped, a row beyond a
// pole is the edge row again, once per repetition: the rows in range plus `below` times row 0 plus `above` times row ny - 1.
// SB_BND_WRAPPER (the f2py flavour's form of the row pass) takes the periodic branch as it stands: the tables hold the
// effective row, the cap (nx - 1) / 2 keeps a window narrower than the circle, and g.ny - 1 is the real last row nlats --
// read with multiplicity by the clamp, never processed (band bits exist for rows 1 .. nlats - 1 only: k_scan).
struct TabWin { int xa0, xb0, xa1, xb1, ya, yb, below, above; };      // (xa1 > xb1: one column range)
__device__ __forceinline__ TabWin tab_window(const Geo &g, int x, int y, int nn) {
    TabWin w;
    w.xa1 = 1; w.xb1 = 0; w.below = w.above = 0;
    if (g.bnd == BND_HALO) {
        w.xa0 = x + g.h - nn; w.xb0 = x + g.h + nn; w.ya = y + g.h - nn; w.yb = y + g.h + nn;
        return w;
    }
    const int lo = x - nn, hi = x + nn;
    if (lo < 0) { w.xa0 = lo + g.nx; w.xb0 = g.nx - 1; w.xa1 = 0; w.xb1 = hi; }
    else if (hi >= g.nx) { w.xa0 = lo; w.xb0 = g.nx - 1; w.xa1 = 0; w.xb1 = hi - g.nx; }
    else { w.xa0 = lo; w.xb0 = hi; }
    w.ya = max(y - nn, 0); w.yb = min(y + nn, g.ny - 1);
    w.below = max(nn - y, 0); w.above = max(y + nn - (g.ny - 1), 0);
    return w;
}
// P(Y, X), zero in front of the frame (every address clamped into it)
template <typename V>
__device__ __forceinline__ V tab_at(const V *t, const Geo &g, int Y, int X) {
    const V v = t[(size_t)min(max(Y, 0), g.nyh - 1) * g.nxh + min(max(X, 0), g.nxh - 1)];
    return (X < 0 || Y < 0) ? V(0) : v;
}
template <typename V>
__device__ __forceinline__ V tab_rect(const V *t, const Geo &g, int xa, int xb, int ya, int yb) {
    return (tab_at(t, g, yb, xb) - tab_at(t, g, ya - 1, xb)) - (tab_at(t, g, yb, xa - 1) - tab_at(t, g, ya - 1, xa - 1));
}
template <typename V>
__device__ __forceinline__ V tab_cols(const V *t, const Geo &g, const TabWin &w, int xa, int xb) {
    V s = tab_rect(t, g, xa, xb, w.ya, w.yb);
    if (w.below) s += (V)w.below * tab_rect(t, g, xa, xb, 0, 0);
    if (w.above) s += (V)w.above * tab_rect(t, g, xa, xb, g.ny - 1, g.ny - 1);
    return s;
}
template <typename V>
__device__ __forceinline__ V tab_sum(const V *t, const Geo &g, const TabWin &w) {
    V s = tab_cols(t, g, w, w.xa0, w.xb0);
    if (w.xa1 <= w.xb1) s += tab_cols(t, g, w, w.xa1, w.xb1);
    return s;
}

template <typename T, bool UPD>                          // UPD: the query applies the update (!job.wind_final)
__global__ __launch_bounds__(TAB_QUERY_NT) void k_table_query(DiagJob<T> job, SbTables tb) {
    const Geo g = job.g;
    const int lane = threadIdx.x & 63;
    // the sub-lists' sizes -> position of an entry, as k_wind
    const int cnt = lane < SB_SEG_PARTS ? job.seg_count[lane] : 0;
    const int incl = sb_wave_scan_add(cnt);
    const int total = __builtin_amdgcn_readlane(incl, SB_SEG_PARTS - 1);
    const int nwaves = gridDim.x * (TAB_QUERY_NT / SB_WAVE);
    const int gw = __builtin_amdgcn_readfirstlane(blockIdx.x * (TAB_QUERY_NT / SB_WAVE) + (threadIdx.x >> 6));
    auto entry = [&](int e) {
        const uint64_t hit = __ballot(lane < SB_SEG_PARTS && e < incl);
        const int part = hit ? __ffsll((unsigned long long)hit) - 1 : 0;
        const int base = __shfl(incl, part) - __shfl(cnt, part);
        return job.seg_list[(size_t)part * job.seg_cap + (e < total ? e - base : 0)];
    };
    const T sd = job.stats[0], rr = job.stats[1];
    const bool limited = g.bnd == BND_HALO;
    const bool fill = sb_tab_fill(tb);                       // (uniform over the launch)
    unsigned ncell = 0;                                      // (wave-uniform) this wave's cells of the report
    for (int e = gw; e < total; e += nwaves) {               // (wave-uniform)
        const SbSegEntry cur = entry(e);
        const unsigned Y = cur.seg / (unsigned)g.nw, Xw = cur.seg - Y * (unsigned)g.nw;
        const int x = (int)(Xw * 64u) + lane - g.h, y = (int)Y - g.h;
        int nnmax = 0, flag = -1;
        bool stored = false;                                 // this lane's cell is answered from its stored window
        if ((cur.word >> lane) & 1ull) {                     // band bits are set for interior cells of processed rows only
            const unsigned o = (unsigned)y * (unsigned)g.nx + (unsigned)x;
            // this call's winds (k_wind left them) and the carried state travel under the gallop and the bisection
            SbCellState<T> cst{};
            if constexpr (UPD) cst = sb_trigger_load<T>(job, (size_t)o);
            // the largest radius the tables answer for this cell: the reach of the format; the frame (no wrap, no clamp:
            // strip_frame_reach) or the circle (2 nn + 1 <= nx)
            const int cap = min(SB_TAB_REACH, limited ? strip_frame_reach(g, x, y) : (g.nx - 1) / 2);
            auto count = [&](int rad) { return (int)tab_sum<unsigned>(tb.C, g, tab_window(g, x, y, rad)); };
            auto mixed = [](int nl, int rad) { return nl > 0 && nl < (2 * rad + 1) * (2 * rad + 1); };
            // "the square of radius nn holds both classes" is monotone in nn: gallop to the first radius that does, bisect
            // between it and the last that did not
            bool found = false;
            int hi = 0, nl = 0, below = 0;
            if (!fill) {
                // the window the last fill left: one coalesced load, and the reads of L and A below depend on nothing else
                const unsigned w = tb.W[o];
                found = stored = w != 0u; hi = sb_tab_radius(w); nl = sb_tab_nl(w);
            } else if (cap >= 1) {
                for (int r = 1;;) {
                    const int c = count(r);
                    if (mixed(c, r)) { found = true; hi = r; nl = c; break; }
                    if (r >= cap) break;
                    below = r;
                    r = min(2 * r, cap);
                }
                for (int lo = below + 1; found && lo < hi;) {
                    const int mid = (lo + hi) >> 1, c = count(mid);
                    if (mixed(c, mid)) { hi = mid; nl = c; } else lo = mid + 1;
                }
            }
            if (fill && tb.W) tb.W[o] = found ? sb_tab_pack(hi, nl) : 0u;
            const T mul = sb_bit(job.clsbits, g.nw, x + g.h, y + g.h) ? T(1) : T(-1);
            if (found) {
                const TabWin w = tab_window(g, x, y, hi);
                const long long TL = (long long)tab_sum<u64>(tb.L, g, w), TS = (long long)(tab_sum<u64>(tb.A, g, w) - (u64)TL);
                auto to_f64 = [](long long v) { return __builtin_fma((double)(int)(v >> 32), 0x1p32, (double)(unsigned)v); };
                const double dnl = (double)nl, dns = (double)((2 * hi + 1) * (2 * hi + 1) - nl);
                const double ml = to_f64(TL) * sb_inv(dnl), ms = to_f64(TS) * sb_inv(dns);
                const T n_thc = mul * (T)((ml - ms) * (1.0 / (double)(1ll << SB_TAB_FB)));        // ref :216
                if constexpr (UPD) sb_trigger_update<T>(job, (size_t)o, n_thc, cst);               // ref :235-266
                else job.thc[o] = n_thc;                                                           // (k_wind applies them)
                nnmax = hi;
            } else {
                // beyond the reach, wider than the circle, or one class as far as the search may go: the global-memory
                // search, with the bound and the counters of a marked cell of the strip kernels (strip_slow_cell)
                int capg = g.nx + g.ny;
                if (limited) capg = min(capg, strip_frame_reach(g, x, y));
                bool one_class;
                const T cg = contrast_global(job, x, y, capg, sd, rr, nnmax, one_class);
                atomicAdd(&job.counters[0], 1);
                if (one_class) atomicAdd(&job.counters[1], 1);
                if constexpr (UPD) sb_trigger_update<T>(job, (size_t)o, mul * cg, cst);
                else job.thc[o] = mul * cg;
            }
            flag = (x >> job.thc_txs) * job.tile_sx + (y / job.thc_ty) * job.tile_sy + job.tile_off;
        }
        // sb_table_cache_report: the band cells searched (found or not), or those a stored window answered
        if (tb.W) ncell += (unsigned)__popcll((unsigned long long)(fill ? cur.word : __ballot(stored)));
        // the largest radius per block / tile (diagnostic, read by sb_last_counters; the flag k_scan raised is 1): one atomic
        // per flag the segment's cells fall under
        for (uint64_t todo = __ballot(nnmax > 1); todo;) {
            const int f = __builtin_amdgcn_readlane(flag, __ffsll((unsigned long long)todo) - 1);
            const bool mine = nnmax > 1 && flag == f;
            const int v = sb_wave_max_to_last(mine ? nnmax : 0);
            if (lane == SB_WAVE - 1) atomicMax(&job.tile_nnmax[f], v);
            todo &= ~__ballot(mine);
        }
    }
    // Every wave leaves its count in a slot of its own and the host adds them up: no atomics (atomics on one word are
    // served one after the other, and there would be one per segment or per wave, most of them at the kernel's end)
    if (tb.W && lane == 0) {
        unsigned *slot = tb.rep + SB_TAB_REP_HDR + 2 * gw;
        slot[0] = fill ? 0u : ncell; slot[1] = fill ? ncell : 0u;
    }
}

// ---- launchers
template <typename T>
hipError_t sb_launch_table_rows(const DiagJob<T> &job, const SbTables &tb, hipStream_t st) {
    const int nblk = (job.g.nyh + SB_TAB_RB - 1) / SB_TAB_RB;
    if (job.flavour == SB_FLAVOUR_WRAPPER) {
        // the f2py flavour's form writes the t0 plane and knows the wrapper's frame alone
        if (job.g.bnd != BND_WRAPPER || job.g.h != 0 || !job.t0) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_table_rows<T, true>), dim3(nblk), dim3(TAB_ROWS_NT), 0, st, job, tb);
    } else hipLaunchKernelGGL((k_table_rows<T, false>), dim3(nblk), dim3(TAB_ROWS_NT), 0, st, job, tb);
    return hipGetLastError();
}
hipError_t sb_launch_table_cols(const Geo &g, const SbTables &tb, hipStream_t st) {
    const int nbx = (g.nxh + TAB_COLS_NT - 1) / TAB_COLS_NT, nby = (g.nyh + TAB_CB - 1) / TAB_CB;
    hipLaunchKernelGGL(k_table_cols, dim3((unsigned)nbx * (unsigned)nby), dim3(TAB_COLS_NT), 0, st, g.nxh, g.nyh, nbx, tb);
    return hipGetLastError();
}
template <typename T>
hipError_t sb_launch_table_query(const DiagJob<T> &job, const SbTables &tb, int ncu, hipStream_t st) {
    static_assert(4 * (TAB_QUERY_NT / SB_WAVE) == SB_TAB_QUERY_WAVES_PER_CU, "the report has a slot per wave");
    // (the plan decides whose the update is: k_wind's behind the query, or the query's from the winds k_wind left)
    if (job.wind_final) hipLaunchKernelGGL((k_table_query<T, false>), dim3(ncu * 4), dim3(TAB_QUERY_NT), 0, st, job, tb);
    else if (job.nws && job.nwd) hipLaunchKernelGGL((k_table_query<T, true>), dim3(ncu * 4), dim3(TAB_QUERY_NT), 0, st, job, tb);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
template hipError_t sb_launch_table_rows<float>(const DiagJob<float> &, const SbTables &, hipStream_t);
template hipError_t sb_launch_table_rows<double>(const DiagJob<double> &, const SbTables &, hipStream_t);
template hipError_t sb_launch_table_query<float>(const DiagJob<float> &, const SbTables &, int, hipStream_t);
template hipError_t sb_launch_table_query<double>(const DiagJob<double> &, const SbTables &, int, hipStream_t);
