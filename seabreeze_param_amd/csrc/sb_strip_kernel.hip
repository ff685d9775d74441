// sb_strip_kernel.hip -- thermal heating contrast (the expanding-window land/sea mean difference of t0)
// on gfx950 for search radii up to 16 cells: marching strips.
// ref: generic/sea_breeze_diag.f90:166-167 (t0), :188-216 (window search and contrast),
//      python_wrapper/seabreezediag/seabreeze_diag_python.f90:187-221
//
// The reference re-sums a (2nn+1)^2 window from scratch at every radius nn until it holds both classes; only the
// last square matters, and "holds both classes" is monotone in nn.  So summed-area tables (all cells, land-side
// cells, land-side count) answer any square with four reads per table and a bisection on the count table finds nn.
//
// Layout.  The grid is cut into strips of 32 owned longitudes; with the halo of 16 cells either side a staged row
// is exactly one 64-lane wave (lane = column).  A strip is cut into blocks of 16 rows (one row per wave of the
// 1024-thread workgroup).  k_scan raises a flag per (strip, block) that holds a coastal-band cell; the flags are laid
// out strip-major with one virtual block above and below every strip, so that "the blocks before and after an
// active block" is plain bit arithmetic on a bit plane.  Every workgroup takes an equal share of the active blocks
// in that order -- consecutive blocks down a strip -- and MARCHES: it stages block after block into a ring of 128
// table rows in LDS, queries the band cells of block j once block j+1 is in the ring, and never stages a row twice
// inside a run (where the tile kernel re-staged a 16-row halo above and below every 48-row tile).
//
// Arithmetic.  t0 is turned into 64-bit fixed point (2^-40 K: below the spacing of doubles near 300 K by 16, so
// window sums are EXACT integer sums of values rounded once) -- the prefix sums are then integer adds, which
// (a) wrap harmlessly, so the tables need no per-tile offset and the ring never has to be re-based,
// (b) take two full-rate DPP instructions per scan step (v_add_co / v_addc with the lane shift fused), where the
//     fp64 scan took two DPP moves and a half-rate v_add_f64,
// (c) make the result independent of how the grid is cut into strips, blocks, bands or GPUs, bit for bit.
//
// Per block (one barrier, LDS only: the prefetched global loads stay in flight):
//   S1  every wave: its row's inputs (prefetched three blocks ahead into registers) -> t0 -> fixed point ->
//       prefix along longitude of {all, land-side, land-side count} -> ring row (not yet summed along latitude);
//       without a stored plan waves 8-15 also list the band cells of the block that is queried in this step
//   --- barrier ---
//   S2  waves 5-7: one table each, prefix along latitude of the 16 new rows (running column totals in registers)
//       waves 0-7: 64 band cells each of the block staged two steps ago: window radius, contrast -> thc
//       (the other waves go straight on to S1 of the next block)
//
// The plan -- shares, order of steps, cell lists with every window's radius, count and class -- is stored in device
// memory and used again for as long as k_scan finds the band and land-side planes unchanged (strip_load_plan).  Statistics,
// planner, cell lists and what follows the march are shared with k_strip32: sb_strip_common.hpp.
// DESIGN.md section 2.4 has the measurements behind the choices, and what hipcc does with loads kept in flight.
#include "sb_thc_common.hpp"
#include "sb_strip_common.hpp"

#define STRIP_HB 1                // halo of the tables in blocks
#define STRIP_H 16                // ... in cells = largest radius answered from LDS
#define STRIP_W 64                // staged columns = lanes
#define STRIP_SW (STRIP_W - 2 * STRIP_H)
#define STRIP_C 16                // rows per block = waves per workgroup
#define STRIP_NT 1024
#define STRIP_RING 128            // ring rows (8 blocks): a query of block j reads rows of blocks j-2 .. j+1 while
                                  // block j+3 may already be written
#define STRIP_P (STRIP_W + 1)     // table pitch: column 0 is the zero column
#define STRIP_MAXW 768            // 64-bit words of the position plane a workgroup can hold (49,151 positions)
#define STRIP_SCHED 384           // steps of one round of a workgroup
#define STRIP_ROUND 90            // active blocks of one round (at most 3 x 90 staged blocks + 90 drain + 3 warm-up + 2 padding steps)
#define STRIP_FB 40               // fractional bits of the fixed-point t0
#define STRIP_DEPTH 3             // blocks of inputs in flight per wave

// The fp64 constants of a staged row -- the logistic's argument reduction and Taylor coefficients, the fixed-point
// conversion -- live in constant memory and are fetched by scalar loads where they are used (two s_load_dwordx16 per
// row, from the scalar cache).  As literals they are loop invariants the compiler keeps in some 40 scalar registers for
// the whole march, and the registers it then has to spill cost the staging code a quarter of its vector instructions
// (v_readlane reloads).  The pointer is made opaque per use so that the loads are not hoisted.
__constant__ double sb_strip_k[20] = {
    1.4426950408889634, 0.6931471805599453, 2.3190468138462996e-17, -708.0, 700.0,            // 0..4: log2(e), ln2 hi, lo, clamps
    1.6666666666666666e-01, 4.1666666666666664e-02, 8.333333333333333e-03, 1.388888888888889e-03,     // 5..8: 1/3! .. 1/6!
    1.984126984126984e-04, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07,     // 9..12: 1/7! .. 1/10!
    2.505210838544172e-08,                                                                         // 13: 1/11!
    -1024.0, 1024.0, 0x1p40, 0x1.8p52,                                                               // 14..17: fixed point
    -0.0060956, 0.0};                                                                               // 18: gmma (ref :138)
typedef const __attribute__((address_space(4))) double *sb_cdp;
#ifndef STRIP_KTAB
#define STRIP_KTAB 0              // 0: the constants as literals (measured faster by 1.6 us: the scalar loads stall the row);
                                  // 1: by scalar loads from the table
#endif
#if STRIP_KTAB
#define SB_K(i, lit) k[i]
#else
#define SB_K(i, lit) (lit)
#endif

// 1 / (1 + exp(y)): sb_logistic_of_neg<double> (sb_device.hpp) operation for operation -- the same bits --, its
// constants optionally from the table
__device__ __forceinline__ double strip_logistic_of_neg(double y, sb_cdp k) {
    y = fmin(fmax(y, -708.0), 700.0);                         // (literals: known not to be NaN, no canonicalisation)
    const double n = __builtin_rint(y * SB_K(0, 1.4426950408889634));
    double r = __builtin_fma(-n, SB_K(1, 0.6931471805599453), y);
    r = __builtin_fma(-n, SB_K(2, 2.3190468138462996e-17), r);                           // |r| <= ln2/2
    // exp(r), degree 11, as E(r^2) + r O(r^2): two Horner chains of five, every multiply-add with ONE constant (a
    // scalar operand; a second one would have to be copied to vector registers first)
    const double r2 = r * r;
    double e = __builtin_fma(r2, SB_K(12, 2.755731922398589e-07), SB_K(10, 2.48015873015873e-05));               // 1/10!, 1/8!
    double o = __builtin_fma(r2, SB_K(13, 2.505210838544172e-08), SB_K(11, 2.7557319223985893e-06));               // 1/11!, 1/9!
    e = __builtin_fma(e, r2, SB_K(8, 1.388888888888889e-03));  o = __builtin_fma(o, r2, SB_K(9, 1.984126984126984e-04));      // 1/6!, 1/7!
    e = __builtin_fma(e, r2, SB_K(6, 4.1666666666666664e-02));  o = __builtin_fma(o, r2, SB_K(7, 8.333333333333333e-03));      // 1/4!, 1/5!
    e = __builtin_fma(e, r2, 0.5);   o = __builtin_fma(o, r2, SB_K(5, 1.6666666666666666e-01));      // 1/2!, 1/3!
    e = __builtin_fma(e, r2, 1.0);   o = __builtin_fma(o, r2, 1.0);
    const double p = __builtin_fma(o, r, e);
    const double x = 1.0 + ldexp(p, (int)n);
    double q = __builtin_amdgcn_rcp(x);                       // v_rcp_f64 (2^-24 relative) and two Newton steps, as sb_logistic_of_neg
    q = __builtin_fma(q, __builtin_fma(-x, q, 1.0), q);
    q = __builtin_fma(q, __builtin_fma(-x, q, 1.0), q);
    return q;
}
// t0 = theta - (gmma*z)*sigmoid(sigma)   ref: generic/sea_breeze_diag.f90:166-167,478-480 (as sb_t0)
// (no branch for sea level: there gmma * z is a signed zero, the product with the -- finite or NaN -- sigmoid too, and
// theta comes back bit for bit, or NaN exactly where the reference's expression gives NaN)
__device__ __forceinline__ double strip_t0(double theta, double z, double sigma, double sd, double r, sb_cdp k) {
    return theta - ((SB_K(18, -0.0060956) * z) * strip_logistic_of_neg(-sd * (sigma - r), k));
}
__device__ __forceinline__ float strip_t0(float theta, float z, float sigma, float sd, float r, sb_cdp) {
    return sb_t0<float>(theta, z, sigma, sd, r);
}

// t0 (K) -> fixed point, BIASED: fma rounds x * 2^40 + 1.5 * 2^52 to an integer held in the mantissa (|x| < 2048 K:
// anything a temperature can be; beyond, the sums are garbage, not a fault), and the bits of that double are the value
// plus the constant SB_FIX_BIAS.  The bias stays in the tables -- a window of n cells holds n of them, which the
// query takes out again -- so a staged cell costs one instruction here instead of five (clamps, 64-bit subtraction).
#define SB_FIX_BIAS 0x4338000000000000ull
__device__ __forceinline__ u64 sb_to_fixed(double x, sb_cdp k) {
    return (u64)__double_as_longlong(__builtin_fma(x, SB_K(16, 0x1p40), SB_K(17, 0x1.8p52)));
}

// what a lane holds of one staged row between the issue of its loads and S1
template <typename T, bool FLY>
struct StripRegs {
    T th;                          // theta (FLY) or t0
    T zz, sg;                      // z, sigma (FLY only)
    uint32_t lw;                   // the 32-bit half of the land-side word that holds the cell
    uint32_t lbit;                 // the cell's bit in lw; 0: no such cell
};

// FLY: t0 from theta, z, sigma while staging.  The contrast goes to thc; thresholds and state update are k_wind's (a
// cell's winds and state loaded here, next to the prefetched blocks of the march, would drain them at every step).
template <typename T, bool FLY>
__global__ __launch_bounds__(STRIP_NT) void k_strip(char *plan, const int *plan_gen, const Moments *fold_partials, int G, StripJob<T> job) {
    // (the three pointers the first loads of the kernel hang on come as leading arguments: with
    // -amdgpu-kernarg-preload-count=7 they are in scalar registers when the wave starts, and the plan header, the
    // change counter and k_scan's partial sums are requested without waiting for a load of the argument block)
    constexpr int HB = STRIP_HB, H = STRIP_H, W = STRIP_W, SW = STRIP_SW, C = STRIP_C, P = STRIP_P, NWV = STRIP_NT / SB_WAVE;
    constexpr int RM = STRIP_RING - 1;
    static_assert(NWV == C && H == HB * C, "one staged row per wave, a halo of whole blocks");
    static_assert(SW == SBS_SW && C == SBS_C && STRIP_SCHED == SBS_SCHED && STRIP_DEPTH == SBS_DEPTH, "the shared skeleton (sb_strip_common.hpp)");
    __shared__ u64 sA[STRIP_RING * P];                 // prefix sums of t0 (fixed point), every cell
    __shared__ u64 sL[STRIP_RING * P];                 // ... land-side cells
    __shared__ unsigned short sC[STRIP_RING * P];      // ... land-side count (modulo 2^16: a window holds < 2^16 cells)
    __shared__ u64 s_land[STRIP_RING];                 // land-side bits of every ring row
    __shared__ u64 s_bits[STRIP_MAXW];                 // the active blocks as a bit plane
    __shared__ uint2 s_ent[STRIP_SCHED];               // steps of the round: x = position | flags, y = strip << 16 | block
                                                       // within the padded strip
    __shared__ unsigned short s_cell[3][SW * C];       // the band cells of the block a step queries, compacted (three steps in flight)
    __shared__ Moments s_wpart[NWV];
    __shared__ int s_scan[NWV];
    __shared__ int s_misc[12];                         // (see StripView::misc)
    __shared__ T s_sdr[2];
    static_assert(sizeof(u64) * (2 * STRIP_RING * P + STRIP_RING + STRIP_MAXW) + 2 * STRIP_RING * P + 8 * STRIP_SCHED +
                          6 * SW * C + sizeof(Moments) * NWV + 4 * NWV + 48 + 16 <= 160 * 1024,
                  "k_strip: LDS of one workgroup");

    const Geo g = job.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int npad = job.nty + 2 * HB;                 // blocks of a strip incl. the virtual ones above and below
    const int npos = job.ntx * npad;
    const int nch = (npos + STRIP_NT - 1) / STRIP_NT;            // <= STRIP_MAXW / 16 (host)
    char *const plan_wg = plan + (size_t)blockIdx.x * SB_PLAN_STRIDE;
    unsigned *const plan_lists = (unsigned *)(plan_wg + SB_PLAN_LIST_OFF);
    static_assert(sizeof(s_cell) >= sizeof(unsigned) * STRIP_MAXW, "the planner's prefix array fits where the cell lists lie");
    StripView<T> v = {job, g, tid, lane, wv, npad, 0xffffffffu / (unsigned)npad + 1u, nch * NWV, plan_wg, plan_lists,
                      s_bits, s_ent, &s_cell[0][0], (unsigned *)&sA[0], s_misc, s_wpart, s_scan, s_sdr, 0, 0};

    SB_T(0);                                             // start
    // ---- prologue 1: statistics; the stored plan, or the flags k_scan raised as a bit plane ----
    T sd = T(0), rr = T(0);
    Moments pm = moments_empty();
    double shift_c = 0.0;
    const bool fold_stats = strip_begin_stats<FLY>(v, fold_partials, sd, rr, pm, shift_c);
    const bool cached = strip_load_plan<STRIP_NT>(v, plan_gen, npos, nch);      // uniform
    // the zero column of the three tables (never written again) while the flags travel
    for (int i = tid; i < STRIP_RING; i += STRIP_NT) { sA[i * P] = 0; sL[i * P] = 0; sC[i * P] = 0; }
    if (tid == 0) s_misc[4] = 0;
    if (fold_stats) wave_total_shifted_store(pm, s_wpart);
    SB_T(1);                                             // first barrier reached
    __syncthreads();
    SB_T(2);                                             // ... passed
    // ---- prologue 2: wave 0 alone plans this workgroup's share and the schedule of its first round (strip_plan) ----
    if (__builtin_expect(!cached, 0)) {
        if (wv == 0) strip_plan<HB, STRIP_ROUND>(v, G);
        __syncthreads();
        if (tid < 8) sA[tid * P] = 0;                    // (the cost array lay over the first rows' zero column)
        SB_T(3);                                         // planned
    }
    const bool store_lists = __builtin_amdgcn_readfirstlane(s_misc[8]) != 0;
    // the cell list of the next step's query, from the stored plan (one entry per lane of the eight querying waves)
    unsigned qc = ~0u;
    const unsigned qc_off = (unsigned)(min(wv, C / 2 - 1) * SB_WAVE + lane);
    const int r_begin = __builtin_amdgcn_readfirstlane(s_misc[5]), r_end = __builtin_amdgcn_readfirstlane(s_misc[6]);

    const bool fastx = g.nx > W + 2;                   // one conditional add wraps every column of a staged row
    const bool limited = g.bnd == BND_HALO;

    // the lane's column of the strip the loads are issued for: byte offsets in a field row and in a row of the
    // land-side plane, bit in the 32-bit word (-1: no such cell); recomputed when the strip changes
    int cc_strip = -1;
    unsigned cc_colb = 0, cc_clsb = 0, cc_lbit = 0;

    // loads of row wv of block jp of `strip`
    // (always four loads, also behind the end of the schedule and for a drain step, from clamped addresses: the
    // compiler counts the loads in flight per program point, and a path without them would make it drain the queue)
    auto issue = [&](StripRegs<T, FLY> &R, unsigned sj) __attribute__((always_inline)) {
        const int strip = (int)(sj >> 16), jp = (int)(sj & 0xffffu);
        if (strip != cc_strip) {                         // wave-uniform
            cc_strip = strip;
            strip_column(g, fastx, (unsigned)sizeof(T), strip * SW - H + lane, true, cc_colb, cc_clsb, cc_lbit);
        }
        bool rowok;
        const int Yr = strip_row(g, (jp - HB) * C + wv, rowok);      // (the interior row may lie outside the grid: clamped or absent)
        // (a scalar base -- field pointer plus the row's offset -- and the lane's 32-bit column offset: two scalar
        // registers per field where a buffer descriptor takes four)
        const size_t rowb = (size_t)((unsigned)Yr * (unsigned)g.nxh) * sizeof(T), wordb = (size_t)((unsigned)Yr * (unsigned)g.nw) * 8u;
        R.th = *(const T *)((const char *)job.theta + rowb + cc_colb);                 // (theta is the t0 plane unless FLY)
        if constexpr (FLY) {
            R.zz = *(const T *)((const char *)job.z + rowb + cc_colb);
            R.sg = *(const T *)((const char *)job.sigma + rowb + cc_colb);
        }
        R.lw = *(const uint32_t *)((const char *)job.clsbits + wordb + cc_clsb);
        R.lbit = rowok ? cc_lbit : 0u;
    };

    // running column totals of the table this wave sums along latitude (waves 5, 6: 64 bit; wave 7: the count)
    u64 carry = 0;

    // S1: the row's registers -> ring row (prefix along longitude only)
    auto stage = [&](StripRegs<T, FLY> &R, unsigned ent, int jp) __attribute__((always_inline)) {
        sb_cdp kt = (sb_cdp)sb_strip_k;
        asm volatile("" : "+s"(kt));                      // (opaque: with STRIP_KTAB the constants are loaded here, every time)
        // This block's loads were issued three steps ago, and the two steps since have each issued a block's loads of their
        // own (`issue` is unconditional) besides lists and stores: once at most two blocks' loads are outstanding -- the
        // counter is in order -- this block's have landed.  Said explicitly, tied to the registers: hipcc's own count of the
        // loads in flight has been seen to go wrong at this very place (see the step), and a wait that is missing here
        // goes unnoticed by every test, three steps being longer than the latency of memory.
        if constexpr (FLY) asm volatile("s_waitcnt vmcnt(8)" : "+v"(R.th), "+v"(R.zz), "+v"(R.sg), "+v"(R.lw) : : "memory");
        else asm volatile("s_waitcnt vmcnt(4)" : "+v"(R.th), "+v"(R.lw) : : "memory");
        // Predicates as one compare each, straight into a lane mask (an `a && b` of two of them costs two more vector
        // instructions to re-form the mask): the land-side bit is tested against a per-lane bit that is zero where the
        // cell does not exist.
        const u64 lm = __builtin_amdgcn_ballot_w64((R.lw & R.lbit) != 0u);
        T t0v = R.th;
        if constexpr (FLY) {
            // the sigmoid only where a lane of the wave stands above sea level (z == 0 -> t0 = theta exactly)   ref :166-167
            if (__builtin_amdgcn_ballot_w64(R.zz != T(0)) != 0) t0v = strip_t0(R.th, R.zz, R.sg, sd, rr, kt);
        }
        u64 qa = sb_to_fixed((double)t0v, kt);
        if (limited) { if (R.lbit == 0u) qa = 0ull; }    // (ghost-celled frames only: columns and rows beyond the frame)
        u64 ql = ((R.lw & R.lbit) != 0u) ? qa : 0ull;
        // (a row on one side of the coast needs one scan: its land-side sums are zero, or the sums over all cells)
        if (lm == 0ull) sb_scan1_u64(qa);                // wave-uniform; ql is zero everywhere
        else if (lm == ~0ull) { sb_scan1_u64(qa); ql = qa; }
        else sb_scan2_u64(qa, ql);
        const unsigned slot = (unsigned)(jp * C + wv) & RM;
        const unsigned o = __umul24(slot, P) + lane + 1;
        sA[o] = qa;
        sL[o] = ql;
        if (__builtin_expect(!cached, 0)) {              // (a stored plan knows every window's radius, count and class)
            // land-side cells up to and including the lane's: those of lanes 1 .. lane by mbcnt on the mask shifted down, lane 0's added
            const u64 lm1 = lm >> 1;
            const unsigned cnt = __builtin_amdgcn_mbcnt_hi((unsigned)(lm1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)lm1, (unsigned)(lm & 1ull)));
            sC[o] = (unsigned short)cnt;
            if (lane == 0) s_land[slot] = lm;
        }
        if (ent & SCH_RESTART) {
            // the tables start afresh: the row above the first one reads as zero, the running totals start at zero
            if (wv == NWV - 1) {
                const unsigned z = __umul24((unsigned)(jp * C - 1) & RM, P) + lane + 1;
                sA[z] = 0; sL[z] = 0; sC[z] = 0;
            }
            carry = 0;
        }
    };

    // S2, waves 5-7: prefix along latitude of the 16 rows of the block at ring position jp
    auto vertical = [&](int jp) __attribute__((always_inline)) {
        const unsigned r0 = (unsigned)(jp * C) & RM;     // a block never straddles the end of the ring (128 = 8 x 16)
        const unsigned o = __umul24(r0, P) + lane + 1;
        if (wv < 7) {
            u64 *tab = (wv == 5 ? sA : sL) + o;
#pragma unroll
            for (int h0 = 0; h0 < C; h0 += 8) {          // eight rows of reads in flight
                u64 v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = tab[(h0 + i) * P];
#pragma unroll
                for (int i = 0; i < 8; ++i) { carry += v[i]; tab[(h0 + i) * P] = carry; }
            }
        } else if (!cached) {
            unsigned short *tab = sC + o;
            unsigned v[C];
#pragma unroll
            for (int i = 0; i < C; ++i) v[i] = tab[i * P];
            unsigned cc = (unsigned)carry;
#pragma unroll
            for (int i = 0; i < C; ++i) { cc += v[i]; tab[i * P] = (unsigned short)cc; }
            carry = cc;
        }
    };

    const unsigned cell_code = strip_cell_code(wv, lane);   // of the band cell this lane lists (waves 8-15: strip_list_cells)

    // S2, waves 0 ..: 64 entries of the list per wave: bisection for the radius, contrast, result
    auto query = [&](int qpos, int strip, int jp, int buf, unsigned qi) __attribute__((always_inline)) {
        // A cell's entry in the stored plan: bits 0-8 row << 5 | column, bit 9 its own class, bits 10-14 the radius of its
        // window (0: it outgrows the tables), bits 15-25 the land-side cells in it; all ones: no cell.  Radius, count
        // and class follow from the land-side plane, which stands as long as the plan does (k_scan watches it too).
        unsigned code;
        bool valid, found, own;
        int nn, nl;
        if (cached) {                                    // uniform: the list of the stored plan (loaded one step ahead)
            code = qc;
            valid = code != ~0u;
            if (__builtin_amdgcn_ballot_w64(valid) == 0ull) return;
            nn = (int)((code >> 10) & 31u);
            nl = (int)((code >> 15) & 2047u);
            own = ((code >> 9) & 1u) != 0u;
            found = valid && nn != 0;
            nn = max(nn, 1);                             // (reads in bounds; the result is not used)
        }
        if (__builtin_expect(!cached, 0)) {
            const int ncell = __builtin_amdgcn_readfirstlane(s_misc[1 + buf]);
            const int e = wv * SB_WAVE + lane;
            valid = e < ncell;
            code = s_cell[buf][valid ? e : 0];
            if (wv * SB_WAVE >= ncell) {                 // wave-uniform
                if (store_lists) plan_lists[qi * (unsigned)(SW * C) + (unsigned)e] = ~0u;
                return;
            }
        }
        const int lx = (int)(code & 31u), ly = (int)((code >> 5) & 15u);
        const int x = strip * SW + lx, y = (jp - 1) * C + ly;
        const unsigned o = (unsigned)y * (unsigned)g.nx + (unsigned)x;     // (fewer than 2^31 cells: check_dims)
        const unsigned rho = (unsigned)(jp * C + ly);    // ring row of the cell
        const unsigned cx = (unsigned)(lx + H + 1);      // its table column
        if (__builtin_expect(!cached, 0)) {
            int lim = H;
            if (limited) lim = min(lim, strip_frame_reach(g, x, y));   // uniform branch
            const int limc = max(lim, 1);
            // land-side count of the square of radius rad: C(r1,a1) - C(r0,a1) - C(r1,a0) + C(r0,a0),
            // r0 = rho-rad-1, r1 = rho+rad, a0 = cx-rad-1, a1 = cx+rad
            auto count = [&](int rad) __attribute__((always_inline)) {
                const unsigned r1 = __umul24((rho + rad) & RM, P) + cx, r0 = __umul24((rho - rad - 1) & RM, P) + cx;
                return (int)(unsigned short)((unsigned)sC[r1 + rad] - (unsigned)sC[r0 + rad] - (unsigned)sC[r1 - rad - 1] + (unsigned)sC[r0 - rad - 1]);
            };
            // Two rounds of independent probes -- radii 4, 8, 12, 16, then the three radii below the smallest of those that
            // holds both classes: 28 reads in two LDS round trips, where a bisection makes 20 reads in five.  The march is
            // bound by the length of its dependent chains, not by LDS issue.
            int nl1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) nl1[k] = count(limited ? min(4 * (k + 1), limc) : 4 * (k + 1));
            int lo = 1, hi = limc;
            nl = 0;
            bool got = false;
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                const int rad = limited ? min(4 * (k + 1), limc) : 4 * (k + 1);
                const bool mixed = nl1[k] > 0 && nl1[k] < (2 * rad + 1) * (2 * rad + 1);
                if (mixed) { hi = rad; nl = nl1[k]; got = true; }
                else if (rad < hi) lo = max(lo, rad + 1);
            }
            found = valid && lim >= 1 && got;
            if (!got) lo = max(1, hi - 3);                   // (probes in bounds; their results are not used)
            int nl2[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) nl2[m] = count(min(lo + m, hi));
#pragma unroll
            for (int m = 2; m >= 0; --m) {
                const int rad = lo + m;
                if (rad < hi && nl2[m] > 0 && nl2[m] < (2 * rad + 1) * (2 * rad + 1)) { hi = rad; nl = nl2[m]; }
            }
            nn = hi;
            // the cell's own class: the table's centre, except that the f2py boundary rule maps the centre of the window at
            // the last longitude to column 1 (there the list entry carries the bit)   ref :182-186, seabreeze_diag_python.f90:202
            const u64 ownw = s_land[rho & RM];
            own = (code >> 10) & 1u ? ((code >> 9) & 1u) != 0u : ((ownw >> (lx + H)) & 1ull) != 0ull;
            if (store_lists)
                plan_lists[qi * (unsigned)(SW * C) + (unsigned)(wv * SB_WAVE + lane)] =
                    valid ? (code & 511u) | (own ? 1u << 9 : 0u) | (found ? (unsigned)nn << 10 : 0u) | (unsigned)nl << 15 : ~0u;
        }
        const int area = (2 * nn + 1) * (2 * nn + 1);
        const unsigned r1 = __umul24((rho + nn) & RM, P) + cx, r0 = __umul24((rho - nn - 1) & RM, P) + cx;
        const u64 l11 = sL[r1 + nn], l01 = sL[r0 + nn], l10 = sL[r1 - nn - 1], l00 = sL[r0 - nn - 1];
        const u64 q11 = sA[r1 + nn], q01 = sA[r0 + nn], q10 = sA[r1 - nn - 1], q00 = sA[r0 - nn - 1];
        // exact: the tables wrap, the window sum does not; every cell of the window carries the fixed-point bias
        const long long RL = (long long)((l11 - l01) - (l10 - l00) - (u64)nl * SB_FIX_BIAS);
        const long long RS = (long long)((q11 - q01) - (q10 - q00) - (u64)area * SB_FIX_BIAS) - RL;      // sea side
        // land mean - sea mean = (RL ns - RS nl) / (nl ns): one reciprocal of an exact small integer (v_rcp_f64 + two
        // Newton steps: within an ulp of the quotient)
        auto to_f64 = [](long long v) { return __builtin_fma((double)(int)(v >> 32), 0x1p32, (double)(unsigned)v); };
        const double dnl = (double)nl, dns = (double)(area - nl);
        const double num = to_f64(RL) * dns - to_f64(RS) * dnl;
        const T contrast = (T)(num * sb_inv(dnl * dns) * 0x1p-40);
        const T mul = own ? T(1) : T(-1);
        int nnmax = 0;
        if (found) { nnmax = nn; job.thc[o] = mul * contrast; }              // ref :216; k_wind applies :235-266
        // cells whose window outgrows the tables: marked, handled behind the march
        if (valid && !found) { job.thc[o] = strip_mark<T>(); s_misc[4] = 1; }
        // per-block largest radius (diagnostic, read by sb_last_counters); the flag k_scan raised is 1
        nnmax = sb_wave_max_to_last(nnmax);
        if (lane == SB_WAVE - 1 && nnmax > 1) atomicMax(&job.flags[qpos], nnmax);
    };

    if (fold_stats && r_begin >= r_end && blockIdx.x == 0) strip_finish_stats<NWV>(v, shift_c);
    // ---- rounds: at most STRIP_ROUND active blocks each (one round on every grid the plane holds with >= 256 workgroups) ----
    for (int ra = r_begin; ra < r_end; ra += STRIP_ROUND) {
        if (ra > r_begin) {                              // (a further round: wave 0 plans it; the cell lists lay over the prefix array)
            if (wv == 0) { strip_make_prefix<HB>(v, false); strip_make_schedule<HB>(v, ra, min(ra + STRIP_ROUND, r_end)); }
            __syncthreads();
        }
        const int nst = __builtin_amdgcn_readfirstlane(s_misc[0]);
        if (nst == 0) break;
        // The first three steps of a round are its warm-up steps: all they do is issue the loads of steps 3, 4, 5 -- here,
        // ahead of the loop, so that the statistics below are finished while those loads travel.
        unsigned E0, J0, E1, J1, E2, J2;
        SB_T(28);
        strip_entry(s_ent, nst, STRIP_DEPTH, E0, J0); strip_entry(s_ent, nst, STRIP_DEPTH + 1, E1, J1); strip_entry(s_ent, nst, STRIP_DEPTH + 2, E2, J2);
        StripRegs<T, FLY> R0, R1, R2;
        SB_T(29);
        issue(R0, J0);
        SB_T(30);
        issue(R1, J1); issue(R2, J2);
        SB_T(31);
        if (fold_stats && ra == r_begin) strip_finish_stats<NWV>(v, shift_c);
        SB_T(4);                                         // march begins
        // A step: S1 of block i (and the list of the band cells to query), barrier, S2 (sums along latitude || queries
        // of the block two up); a drain step (behind the last block of a run) has no block and queries the block one
        // up.  The three register sets take turns -- as three copies of the step in the loop body, not as a switch, an
        // inner loop or a loop with an early exit: the compiler counts the loads in flight per program point, and only
        // straight-line rotation with the same loads on every path lets it wait for block i's loads alone while those
        // of blocks i + 1 and i + 2 stay in flight.  The set just consumed receives the loads of block i + 3.
        auto step = [&](StripRegs<T, FLY> &R, unsigned &E, unsigned &J, const unsigned &En, int i, int buf) __attribute__((always_inline)) {
            const unsigned ent = E, sj = J;
#if defined(SB_STAMPS) && !defined(SB_STAMPS_WIND)
            if (i < SB_NSTAMP - 5) SB_T(5 + i);          // step i begins (i >= 3)
#endif
            strip_entry(s_ent, nst, i + STRIP_DEPTH, E, J);   // (consumed by `issue` below: the read travels under S1)
            const int pos = (int)(ent & 0xffffu);
            const int strip = (int)(sj >> 16), jp = (int)(sj & 0xffffu);
            const bool drain = (ent & SCH_DRAIN) != 0, idle = (ent & SCH_IDLE) != 0;
            const int qoff = drain ? HB : HB + 1;
            const bool qany = (ent & (drain ? SCH_Q1 : SCH_Q2)) != 0;
            if (!idle) {
                if (ent & SCH_RESTART) {
                    lds_barrier();                                // the queries of the run before have left the ring
                    if (FLY && (fold_stats || job.ngath > 0)) { sd = s_sdr[0]; rr = s_sdr[1]; }
                }
                BandWords bwd;
                const bool lister = qany && wv >= C / 2 && !cached;
                if (lister) bwd = strip_band_issue<HB>(job, g, wv, strip, jp - qoff);
                if (tid == STRIP_NT - 1) s_misc[1 + (buf == 2 ? 0 : buf + 1)] = 0;   // the next step's list starts empty
                if (!drain) stage(R, ent, jp);
                if (lister) strip_list_cells<HB>(job, g, wv, lane, cell_code, strip, jp - qoff, bwd, s_cell[buf], &s_misc[1 + buf]);
            }
            // The stored list of the NEXT step's query, loaded AHEAD of this step's block loads: the vector-memory counter is
            // in order, and a list loaded behind them could only be waited for together with them -- a query step then sat
            // out what was left of the latency of loads meant for three steps later (k_strip32: 1.4 us per query step).
            unsigned qn = ~0u;
            if (cached) qn = plan_lists[((En >> SCH_QI_SHIFT) & (SB_PLAN_NQ - 1)) * (unsigned)(SW * C) + qc_off];
            issue(R, J);                                          // (the one place of this copy of the step that loads blocks)
            if (!idle) {
                lds_barrier();
                if (qany && wv < C / 2) query(pos - qoff, strip, jp - qoff, buf, (ent >> SCH_QI_SHIFT) & (SB_PLAN_NQ - 1));
                if (!drain && wv >= 5 && wv < 8) vertical(jp);
            }
            // (Under the uniform condition, although every other load of the march is unconditional: with this load on
            // every path hipcc 7.2 emitted NO wait at all for the staged blocks' loads in the fp64 kernels -- the
            // results then hang on timing.  tools/check_waits.py (run by tests/test_abi_and_host.py) checks the waits of every variant in the built library.)
            if (cached) qc = qn;
        };
        for (int i = STRIP_DEPTH; i < nst; i += STRIP_DEPTH) {       // nst is a multiple of three
            step(R0, E0, J0, E1, i, 0);
            step(R1, E1, J1, E2, i + 1, 1);
            step(R2, E2, J2, E0, i + 2, 2);
        }
        __syncthreads();                                 // the schedule and the ring are free for the next round
    }

    SB_T(5);                                             // march done
    strip_marked_cells<HB, STRIP_NT>(v, cached, limited, sd, rr, r_begin, r_end);
    SB_T(6);                                             // marked cells done
    if (job.update) strip_band_update<HB, STRIP_NT>(v, cached || store_lists, r_begin, r_end);
    // k_wind's segment lists: compacted when the plan is made, and again only when it is made again (they follow from the
    // band plane, as the plan does)
    if (job.fold && !(cached && job.lists_stand))
        sb_compact_segments<STRIP_NT>(g, job.bandbits, job.seg_list, job.seg_count, job.seg_cap, G, s_scan);
    SB_T(7);                                             // end
}

template <typename T>
hipError_t sb_launch_strip(const DiagJob<T> &job, int ncu, hipStream_t st) {
    const dim3 gr(ncu), bl(STRIP_NT);                   // one persistent workgroup per CU
    const StripJob<T> sj = strip_job<T>(job);
    if (!job.wind_final) return hipErrorInvalidValue;   // (the update is k_wind's: sb_launch_diag sees to it)
    if (job.t0_fly) hipLaunchKernelGGL((k_strip<T, true>), gr, bl, 0, st, sj.plan, sj.plan_gen, sj.fold_partials, ncu, sj);
    else hipLaunchKernelGGL((k_strip<T, false>), gr, bl, 0, st, sj.plan, sj.plan_gen, sj.fold_partials, ncu, sj);
    return hipGetLastError();
}
template hipError_t sb_launch_strip<float>(const DiagJob<float> &, int, hipStream_t);
template hipError_t sb_launch_strip<double>(const DiagJob<double> &, int, hipStream_t);

// the strip kernel's block grid for a domain of nx x rows interior cells; false: the position plane cannot hold it
bool sb_strip_shape(int nx, int rows, int *ntx, int *nty) {
    *ntx = (nx + STRIP_SW - 1) / STRIP_SW;
    *nty = (rows + STRIP_C - 1) / STRIP_C;
    return (long long)*ntx * (*nty + 2) < (long long)STRIP_MAXW * 64;
}
