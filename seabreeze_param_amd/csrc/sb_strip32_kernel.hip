// sb_strip32_kernel.hip -- thermal heating contrast on gfx950 for search radii up to 31 cells in SINGLE precision:
// marching strips with 96-column rows (the N2560 grid of BASELINE configs[3]: its distance field is made with a window
// of 30 cells, so a land/sea window reaches at most 31).
// ref: generic/sea_breeze_diag.f90:166-167 (t0), :188-216 (window search and contrast),
//      python_wrapper/seabreezediag/seabreeze_diag_python.f90:187-221
//
// The march is k_strip's (sb_strip_kernel.hip; read that header first): strips of 32 owned longitudes, blocks of 16 rows,
// summed-area tables in a ring in LDS, every row staged once per run, a stored plan.  What a halo of 32 cells changes:
//
// * A staged row is 96 columns -- 32 owned, 32 either side -- i.e. one and a half waves.  Every wave stages TWO pieces
//   of its row: segment A (columns 0..63, lane = column) and segment B (columns 64..95, lanes 0..31), each with a
//   prefix sum of its own: no carry crosses from one wave's registers to another's.  A window that straddles column 64
//   is the A part up to column 63 plus the B part: six table reads per corner pair instead of four.
// * The tables must hold 2 x 31 + 1 rows round a cell plus the block being staged; what 160 KB of LDS hold is a ring of
//   SIX blocks (96 rows) of 97 entries of 16 bytes -- and that only because an entry is two words, not three: single
//   precision leaves room to PACK.  t0 goes to fixed point with 24 fractional bits (exact for every fp32 value >= 0.5 K
//   in magnitude; 2^-25 K otherwise), |t0| < 2048 K, a window holds < 2^13 cells, so a window sum needs 48 bits: the
//   land-side table holds (sum << 16 | count) in one 64-bit word, sums and counts wrap independently, and the four-
//   (six-)corner combination gives the window's sum and its land-side count at once -- there is no count table.
//   (Double precision needs all 64 bits for the sum alone: radii beyond 16 stay with the tile kernel there.)
// * With six blocks in the ring the block being staged may not be written while the block three up is queried (its
//   window's first row lies five blocks back): a step has TWO barriers, stage | sums along latitude + queries.
//   A window of radius 32 would reach one row further back still: radii beyond 31 are marked and take the global path.
// * An active block needs two staged blocks either side; the flags carry two virtual blocks above and below a strip;
//   a block is queried when the block three positions down has been staged.
#include "sb_strip_common.hpp"

#define S32_HB 2                  // halo of the tables in blocks
#define S32_HMAX 31               // largest radius answered from LDS
#define S32_W 96                  // staged columns
#define S32_SW 32                 // owned columns
#define S32_C 16                  // rows per block = waves per workgroup
#define S32_NT 1024
#define S32_NBLK 6                // blocks in the ring
#define S32_RING (S32_NBLK * S32_C)
#define S32_P 97                  // table pitch: 64 entries of segment A, 32 of segment B, one of padding (odd: no bank conflicts down a column)
#define S32_MAXW 768              // 64-bit words of the position plane a workgroup can hold (49,151 positions)
#define S32_SCHED 384             // steps of one round of a workgroup
#define S32_ROUND 60              // active blocks of one round (at most 5 x 60 staged blocks + 60 drain + 3 warm-up + 2 padding steps)
#define S32_FB 24                 // fractional bits of the fixed-point t0
#define S32_DEPTH 3               // blocks of inputs in flight per wave
#define S32_QOFF (S32_HB + 1)     // a block is queried in the step that stages the block this many positions down

// t0 (K) -> fixed point with 24 fractional bits, BIASED (as k_strip's sb_to_fixed: the bits of fma(x, 2^24, 1.5 * 2^52))
#define S32_FIX_BIAS 0x4338000000000000ull
__device__ __forceinline__ u64 s32_to_fixed(double x) {
    return (u64)__double_as_longlong(__builtin_fma(x, 0x1p24, 0x1.8p52));
}

// what a lane holds of one piece (segment A or B) of a staged row between the issue of its loads and S1
template <bool FLY>
struct S32Regs {
    float th;                      // theta (FLY) or t0
    float zz, sg;                  // z, sigma (FLY only)
    uint32_t lw;                   // the 32-bit half of the land-side word that holds the cell
    uint32_t lbit;                 // the cell's bit in lw; 0: no such cell
};

// The LDS of one workgroup.
struct S32Lds {
    u64 sA[S32_RING * S32_P];      // prefix sums of t0 (fixed point, biased), every cell
    u64 sL[S32_RING * S32_P];      // land-side cells: (sum << 16) | count
    u64 s_land[S32_RING];          // land-side bits of segment A of every ring row
    u64 s_bits[S32_MAXW];          // the active blocks as a bit plane
    uint2 s_ent[S32_SCHED];        // steps of the round: x = position | flags, y = strip << 16 | block within the padded strip
    Moments s_wpart[S32_NT / SB_WAVE];
    float s_sdr[2];
    int s_scan[S32_NT / SB_WAVE];
    int s_misc[12];
    unsigned short s_cell[3][S32_SW * S32_C];
};
static_assert(sizeof(S32Lds) <= 160 * 1024, "k_strip32: LDS of one workgroup");

// FLY: t0 from theta, z, sigma while staging.  The contrast goes to thc; thresholds and state update are k_wind's, or --
// a band step -- applied behind the march (job.update), as in k_strip.
template <bool FLY>
__global__ __launch_bounds__(S32_NT) void k_strip32(char *plan, const int *plan_gen, const Moments *fold_partials, int G, StripJob<float> job) {
    typedef float T;
    constexpr int HB = S32_HB, SW = S32_SW, C = S32_C, P = S32_P, NWV = S32_NT / SB_WAVE, RING = S32_RING;
    static_assert(NWV == C, "one staged row per wave");
    static_assert(SW == SBS_SW && C == SBS_C && S32_SCHED == SBS_SCHED && S32_DEPTH == SBS_DEPTH, "the shared skeleton (sb_strip_common.hpp)");
    __shared__ S32Lds L;
    u64 (&sA)[S32_RING * S32_P] = L.sA;
    u64 (&sL)[S32_RING * S32_P] = L.sL;
    u64 (&s_land)[S32_RING] = L.s_land;
    u64 (&s_bits)[S32_MAXW] = L.s_bits;
    uint2 (&s_ent)[S32_SCHED] = L.s_ent;
    unsigned short (&s_cell)[3][S32_SW * S32_C] = L.s_cell;
    Moments (&s_wpart)[S32_NT / SB_WAVE] = L.s_wpart;
    int (&s_scan)[S32_NT / SB_WAVE] = L.s_scan;
    int (&s_misc)[12] = L.s_misc;                      // (see StripView::misc)
    float (&s_sdr)[2] = L.s_sdr;

    const Geo g = job.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int npad = job.nty + 2 * HB;                 // blocks of a strip incl. the virtual ones above and below
    const int npos = job.ntx * npad;
    const int nch = (npos + S32_NT - 1) / S32_NT;            // <= S32_MAXW / 16 (host)
    char *const plan_wg = plan + (size_t)blockIdx.x * SB_PLAN_STRIDE;
    unsigned *const plan_lists = (unsigned *)(plan_wg + SB_PLAN_LIST_OFF);
    static_assert(sizeof(L.s_cell) >= sizeof(unsigned) * S32_MAXW, "the planner's prefix array fits where the cell lists lie");
    StripView<T> v = {job, g, tid, lane, wv, npad, 0xffffffffu / (unsigned)npad + 1u, nch * NWV, plan_wg, plan_lists,
                      s_bits, s_ent, &s_cell[0][0], (unsigned *)&sA[0], s_misc, s_wpart, s_scan, s_sdr, 0, 0};

    SB_T(0);                                             // start
    // ---- prologue 1: statistics; the stored plan, or the flags k_scan raised as a bit plane ----
    T sd = T(0), rr = T(0);
    Moments pm = moments_empty();
    double shift_c = 0.0;
    const bool fold_stats = strip_begin_stats<FLY>(v, fold_partials, sd, rr, pm, shift_c);
    const bool cached = strip_load_plan<S32_NT>(v, plan_gen, npos, nch);      // uniform
    if (tid == 0) s_misc[4] = 0;
    if (fold_stats) wave_total_shifted_store(pm, s_wpart);
    SB_T(1);                                             // first barrier reached
    __syncthreads();
    SB_T(2);                                             // ... passed
    // ---- prologue 2: wave 0 alone plans this workgroup's share and the schedule of its first round (strip_plan) ----
    if (__builtin_expect(!cached, 0)) {
        if (wv == 0) strip_plan<HB, S32_ROUND>(v, G);
        __syncthreads();
        SB_T(3);                                         // planned
    }
    const bool store_lists = __builtin_amdgcn_readfirstlane(s_misc[8]) != 0;
    unsigned qc = ~0u;                                   // the cell list entry of the next step's query, from the stored plan
    const unsigned qc_off = (unsigned)(min(wv, C / 2 - 1) * SB_WAVE + lane);
    const int r_begin = __builtin_amdgcn_readfirstlane(s_misc[5]), r_end = __builtin_amdgcn_readfirstlane(s_misc[6]);

    const bool fastx = g.nx > S32_W + 2;               // one conditional add wraps every column of a staged row
    const bool limited = g.bnd == BND_HALO;

    // the lane's columns of the strip the loads are issued for (segment A: column lane; segment B: column 64 + lane, lanes
    // 0 .. 31): byte offsets in a field row and in a row of the land-side plane, bit in the 32-bit word (0: no such cell)
    int cc_strip = -1;
    unsigned cc_colA = 0, cc_clsA = 0, cc_bitA = 0, cc_colB = 0, cc_clsB = 0, cc_bitB = 0;

    // loads of row wv of block jp of `strip`: both pieces.  Always the same loads, also behind the end of the schedule and
    // for a drain step, from clamped addresses (see k_strip: the compiler counts the loads in flight per program point).
    auto issue = [&](S32Regs<FLY> &RA, S32Regs<FLY> &RB, unsigned sj) __attribute__((always_inline)) {
        const int strip = (int)(sj >> 16), jp = (int)(sj & 0xffffu);
        if (strip != cc_strip) {                         // wave-uniform
            cc_strip = strip;
            strip_column(g, fastx, (unsigned)sizeof(T), strip * SW - 32 + lane, true, cc_colA, cc_clsA, cc_bitA);
            strip_column(g, fastx, (unsigned)sizeof(T), strip * SW + 32 + (lane & 31), lane < 32, cc_colB, cc_clsB, cc_bitB);
        }
        bool rowok;
        const int Yr = strip_row(g, (jp - HB) * C + wv, rowok);      // (the interior row may lie outside the grid: clamped or absent)
        const size_t rowb = (size_t)((unsigned)Yr * (unsigned)g.nxh) * sizeof(T), wordb = (size_t)((unsigned)Yr * (unsigned)g.nw) * 8u;
        RA.th = *(const T *)((const char *)job.theta + rowb + cc_colA);                 // (theta is the t0 plane unless FLY)
        RB.th = *(const T *)((const char *)job.theta + rowb + cc_colB);
        if constexpr (FLY) {
            RA.zz = *(const T *)((const char *)job.z + rowb + cc_colA);
            RB.zz = *(const T *)((const char *)job.z + rowb + cc_colB);
            RA.sg = *(const T *)((const char *)job.sigma + rowb + cc_colA);
            RB.sg = *(const T *)((const char *)job.sigma + rowb + cc_colB);
        }
        RA.lw = *(const uint32_t *)((const char *)job.clsbits + wordb + cc_clsA);
        RB.lw = *(const uint32_t *)((const char *)job.clsbits + wordb + cc_clsB);
        RA.lbit = rowok ? cc_bitA : 0u;
        RB.lbit = rowok ? cc_bitB : 0u;
    };

    // running column totals of the table this wave sums along latitude (waves 8, 9, 10)
    u64 carry = 0;

    // ring row of row r of the block at padded position jp (blocks never straddle the end of the ring)
    auto slot_of = [&](int jp, int r) __attribute__((always_inline)) -> unsigned {
        return (unsigned)((jp % S32_NBLK) * C + r);
    };

    // S1: one piece of the row -> its ring row (prefix along longitude only).  SEG 0: columns 0 .. 63; 1: columns 64 .. 95
    // (lanes 0 .. 31; the upper lanes carry zeros through the scan and write nothing).
    auto stage = [&](S32Regs<FLY> &R, unsigned slot, int seg) __attribute__((always_inline)) {
        // (the block's loads have landed once at most two blocks' loads -- two pieces each -- are outstanding: see k_strip)
        if constexpr (FLY) asm volatile("s_waitcnt vmcnt(16)" : "+v"(R.th), "+v"(R.zz), "+v"(R.sg), "+v"(R.lw) : : "memory");
        else asm volatile("s_waitcnt vmcnt(8)" : "+v"(R.th), "+v"(R.lw) : : "memory");
        const bool live = seg == 0 || lane < 32;
        const bool land = live && (R.lw & R.lbit) != 0u;
        const u64 lm = __builtin_amdgcn_ballot_w64(land);
        T t0v = R.th;
        if constexpr (FLY) {
            // the sigmoid only where a lane of the wave stands above sea level (z == 0 -> t0 = theta exactly)   ref :166-167
            if (__builtin_amdgcn_ballot_w64(R.zz != T(0)) != 0) t0v = sb_t0<T>(R.th, R.zz, R.sg, sd, rr);
        }
        u64 qa = s32_to_fixed((double)t0v);
        if (!live || (limited && R.lbit == 0u)) qa = 0ull;   // (the upper half of a B wave; ghost-celled frames: cells beyond the frame)
        u64 ql = land ? (qa << 16) | 1ull : 0ull;            // (the bias leaves by the shift: its low 48 bits are zero)
        const u64 all = seg == 0 ? ~0ull : 0xffffffffull;
        if (lm == 0ull) sb_scan1_u64(qa);                // wave-uniform; ql is zero everywhere
        else if (lm == all) { sb_scan1_u64(qa); ql = (qa << 16) + (u64)(lane + 1); }      // every cell land side: sums and counts follow
        else sb_scan2_u64(qa, ql);
        const unsigned o = __umul24(slot, P) + (seg == 0 ? 0u : 64u) + (unsigned)lane;
        if (live) { sA[o] = qa; sL[o] = ql; }
        if (seg == 0 && !cached && lane == 0) s_land[slot] = lm;
    };

    // S2, waves 8 .. 10: prefix along latitude of the 16 rows of the block at padded position jp: wave 8 the all-cells table's
    // segment A, wave 9 the land-side table's, wave 10 both tables' segment B (lanes 0 .. 31 | 32 .. 63)
    auto vertical = [&](int jp) __attribute__((always_inline)) {
        const unsigned r0 = slot_of(jp, 0);
        u64 *tab;
        if (wv == 8) tab = sA + __umul24(r0, P) + lane;
        else if (wv == 9) tab = sL + __umul24(r0, P) + lane;
        else tab = (lane < 32 ? sA : sL) + __umul24(r0, P) + 64 + (lane & 31);
#pragma unroll
        for (int h0 = 0; h0 < C; h0 += 8) {              // eight rows of reads in flight
            u64 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = tab[(h0 + i) * P];
#pragma unroll
            for (int i = 0; i < 8; ++i) { carry += v[i]; tab[(h0 + i) * P] = carry; }
        }
    };

    const unsigned cell_code = strip_cell_code(wv, lane);   // of the band cell this lane lists (waves 8-15: strip_list_cells)

    // S2, waves 0 .. 7: 64 entries of the list per wave: radius, contrast, result
    // A cell's entry in the stored plan: bits 0-8 row << 5 | column, bit 9 its own class, bits 10-14 the radius of its window
    // (0: it outgrows the tables), bits 15-27 the land-side cells in it; all ones: no cell.
    auto query = [&](int qpos, int strip, int jp, int buf, unsigned qi) __attribute__((always_inline)) {
        unsigned code;
        bool valid, found, own;
        int nn, nl;
        if (cached) {                                    // uniform: the list of the stored plan (loaded one step ahead)
            code = qc;
            valid = code != ~0u;
            if (__builtin_amdgcn_ballot_w64(valid) == 0ull) return;
            nn = (int)((code >> 10) & 31u);
            nl = (int)((code >> 15) & 8191u);
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
        const int x = strip * SW + lx, y = (jp - HB) * C + ly;
        const unsigned o = (unsigned)y * (unsigned)g.nx + (unsigned)x;     // (fewer than 2^31 cells: check_dims)
        const int rho = (int)slot_of(jp, ly);            // ring row of the cell
        const int cx = lx + 32;                          // its staged column (segment A)
        // the six entries of a window of radius rad: rows r1 = rho + rad and r0 = rho - rad - 1 (ring), columns
        // left = cx - rad - 1 (segment A: >= 0 for rad <= 31), min(cx + rad, 63) and -- where the window crosses into
        // segment B -- cx + rad itself
        auto corners = [&](int rad, unsigned &i11, unsigned &i10, unsigned &i01, unsigned &i00, unsigned &b1, unsigned &b0, bool &hasb) __attribute__((always_inline)) {
            int r1 = rho + rad, r0 = rho - rad - 1;
            r1 -= r1 >= RING ? RING : 0;
            r0 += r0 < 0 ? RING : 0;
            const int right = cx + rad, left = cx - rad - 1;
            hasb = right >= 64;
            const unsigned p1 = __umul24((unsigned)r1, P), p0 = __umul24((unsigned)r0, P);
            const unsigned rc = (unsigned)min(right, 63), rb = (unsigned)max(right, 64);
            i11 = p1 + rc; i10 = p1 + (unsigned)left; i01 = p0 + rc; i00 = p0 + (unsigned)left;
            b1 = p1 + rb; b0 = p0 + rb;
        };
        if (__builtin_expect(!cached, 0)) {
            int lim = S32_HMAX;
            if (limited) lim = min(lim, strip_frame_reach(g, x, y));   // uniform branch
            const int limc = max(lim, 1);
            // land-side count of the square of radius rad: the low 16 bits of the land-side table's six-entry combination
            const unsigned short *c16 = (const unsigned short *)sL;
            auto count = [&](int rad) __attribute__((always_inline)) {
                unsigned i11, i10, i01, i00, b1, b0;
                bool hasb;
                corners(rad, i11, i10, i01, i00, b1, b0, hasb);
                const unsigned a = (unsigned)c16[4 * i11] - (unsigned)c16[4 * i01] - (unsigned)c16[4 * i10] + (unsigned)c16[4 * i00];
                const unsigned b = (unsigned)c16[4 * b1] - (unsigned)c16[4 * b0];
                return (int)(unsigned short)(a + (hasb ? b : 0u));
            };
            // One round of independent probes -- radii 8, 16, 24, 31 -- brackets the answer ("holds both classes" is
            // monotone in the radius); three dependent probes bisect the bracket of at most eight radii.  (This is the
            // planning call's path: a stored plan knows every radius.  Seven independent probes instead of the bisection
            // cost the kernel 13 spilled vector registers.)
            int nl1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) nl1[k] = count(min(k == 3 ? S32_HMAX : 8 * (k + 1), limc));
            int lo = 1, hi = limc;
            nl = 0;
            bool got = false;
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                const int rad = min(k == 3 ? S32_HMAX : 8 * (k + 1), limc);
                const bool mixed = nl1[k] > 0 && nl1[k] < (2 * rad + 1) * (2 * rad + 1);
                if (mixed) { hi = rad; nl = nl1[k]; got = true; }
                else if (rad < hi) lo = max(lo, rad + 1);
            }
            found = valid && lim >= 1 && got;
            if (!got) lo = hi;                               // (no probe needed; the result is not used)
#pragma unroll 1
            for (int it = 0; it < 3; ++it) {                 // lo <= answer <= hi, hi holds both classes; hi - lo < 8
                const int mid = (lo + hi) >> 1;              // (mid < hi unless lo == hi)
                const int c = count(mid);
                const bool mixed = c > 0 && c < (2 * mid + 1) * (2 * mid + 1);
                if (lo < hi) {
                    if (mixed) { hi = mid; nl = c; }
                    else lo = mid + 1;
                }
            }
            nn = hi;
            // the cell's own class: the table's centre, except at the last longitude under the f2py boundary rule (see k_strip)
            const u64 ownw = s_land[rho];
            own = (code >> 10) & 1u ? ((code >> 9) & 1u) != 0u : ((ownw >> cx) & 1ull) != 0ull;
            if (store_lists)
                plan_lists[qi * (unsigned)(SW * C) + (unsigned)(wv * SB_WAVE + lane)] =
                    valid ? (code & 511u) | (own ? 1u << 9 : 0u) | (found ? (unsigned)nn << 10 : 0u) | (unsigned)nl << 15 : ~0u;
        }
        const int area = (2 * nn + 1) * (2 * nn + 1);
        unsigned i11, i10, i01, i00, b1, b0;
        bool hasb;
        corners(nn, i11, i10, i01, i00, b1, b0, hasb);
        const u64 l11 = sL[i11], l01 = sL[i01], l10 = sL[i10], l00 = sL[i00], lb1 = sL[b1], lb0 = sL[b0];
        const u64 q11 = sA[i11], q01 = sA[i01], q10 = sA[i10], q00 = sA[i00], qb1 = sA[b1], qb0 = sA[b0];
        // exact: the tables wrap, the window's sums do not.  Land side: (sum << 16) + count; all cells: sum + area x bias.
        const u64 PL = (l11 - l01) - (l10 - l00) + (hasb ? lb1 - lb0 : 0ull);
        const long long RL = (long long)(PL - (u64)nl) >> 16;
        const long long RS = (long long)((q11 - q01) - (q10 - q00) + (hasb ? qb1 - qb0 : 0ull) - (u64)area * S32_FIX_BIAS) - RL;      // sea side
        auto to_f64 = [](long long v) { return __builtin_fma((double)(int)(v >> 32), 0x1p32, (double)(unsigned)v); };
        const double dnl = (double)nl, dns = (double)(area - nl);
        const double num = to_f64(RL) * dns - to_f64(RS) * dnl;
        const T contrast = (T)(num * sb_inv(dnl * dns) * 0x1p-24);
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
    // ---- rounds: at most S32_ROUND active blocks each ----
    for (int ra = r_begin; ra < r_end; ra += S32_ROUND) {
        if (ra > r_begin) {                              // (a further round: wave 0 plans it; the cell lists lay over the prefix array)
            if (wv == 0) { strip_make_prefix<HB>(v, false); strip_make_schedule<HB>(v, ra, min(ra + S32_ROUND, r_end)); }
            __syncthreads();
        }
        const int nst = __builtin_amdgcn_readfirstlane(s_misc[0]);
        if (nst == 0) break;
        unsigned E0, J0, E1, J1, E2, J2;
        strip_entry(s_ent, nst, S32_DEPTH, E0, J0); strip_entry(s_ent, nst, S32_DEPTH + 1, E1, J1); strip_entry(s_ent, nst, S32_DEPTH + 2, E2, J2);
        S32Regs<FLY> A0, B0, A1, B1, A2, B2;
        issue(A0, B0, J0); issue(A1, B1, J1); issue(A2, B2, J2);
        if (fold_stats && ra == r_begin) strip_finish_stats<NWV>(v, shift_c);
        SB_T(4);                                         // march begins
        // A step: S1 -- both pieces of row wv of block i (and, without a stored plan, the list of the band cells to query) --
        // barrier, S2 -- sums along latitude (waves 8 .. 10) || queries of the block three up (waves 0 .. 7) -- barrier.
        // The three register sets take turns as three copies of the step, as in k_strip.
        auto step = [&](S32Regs<FLY> &RA, S32Regs<FLY> &RB, unsigned &E, unsigned &J, const unsigned &En, int i, int buf) __attribute__((always_inline)) {
            const unsigned ent = E, sj = J;
#if defined(SB_STAMPS) && !defined(SB_STAMPS_WIND)
            if (i < SB_NSTAMP - 10) SB_T(5 + i);         // step i begins (i >= 3)
#define SB_TS(k) do { if (i == 12) SB_T(27 + (k)); } while (0)      // the inside of one step (the tenth of the march)
#else
#define SB_TS(k) do { } while (0)
#endif
            strip_entry(s_ent, nst, i + S32_DEPTH, E, J);     // (consumed by `issue` below: the read travels under S1)
            const int pos = (int)(ent & 0xffffu);
            const int strip = (int)(sj >> 16), jp = (int)(sj & 0xffffu);
            const bool drain = (ent & SCH_DRAIN) != 0, idle = (ent & SCH_IDLE) != 0;
            const int qoff = drain ? HB : S32_QOFF;
            const bool qany = (ent & (drain ? SCH_Q1 : SCH_Q2)) != 0;
            if (!idle) {
                if (ent & SCH_RESTART) {
                    carry = 0;                                    // the tables start afresh (no window reaches above a run's first row)
                    if (FLY && (fold_stats || job.ngath > 0)) { sd = s_sdr[0]; rr = s_sdr[1]; }
                }
                BandWords bwd;
                const bool lister = qany && wv >= C / 2 && !cached;
                if (lister) bwd = strip_band_issue<HB>(job, g, wv, strip, jp - qoff);
                if (tid == S32_NT - 1) s_misc[1 + (buf == 2 ? 0 : buf + 1)] = 0;   // the next step's list starts empty
                if (!drain) {
                    const unsigned slot = slot_of(jp, wv);
                    stage(RA, slot, 0);
                    stage(RB, slot, 1);
                }
                if (lister) strip_list_cells<HB>(job, g, wv, lane, cell_code, strip, jp - qoff, bwd, s_cell[buf], &s_misc[1 + buf]);
            }
            // The stored list of the NEXT step's query, loaded AHEAD of this step's block loads: the vector-memory counter is
            // in order, and a list loaded behind them could only be waited for together with them -- every query step then
            // sat out what was left of the latency of loads meant for three steps later (round 4: 1.4 us per query step).
            unsigned qn = ~0u;
            if (cached) qn = plan_lists[((En >> SCH_QI_SHIFT) & (SB_PLAN_NQ - 1)) * (unsigned)(SW * C) + qc_off];
            SB_TS(0);                                             // staged
            issue(RA, RB, J);                                     // (the one place of this copy of the step that loads blocks)
            if (!idle) {
                SB_TS(1);                                         // loads issued, first barrier reached
                lds_barrier();
                SB_TS(2);                                         // ... passed
                if (qany && wv < C / 2) query(pos - qoff, strip, jp - qoff, buf, (ent >> SCH_QI_SHIFT) & (SB_PLAN_NQ - 1));
                if (!drain && wv >= 8 && wv <= 10) vertical(jp);
                SB_TS(3);                                         // queries / sums along latitude done
                lds_barrier();                                    // (the next step writes the ring block this step's queries read)
                SB_TS(4);                                         // second barrier passed
            }
            if (cached) qc = qn;
        };
        // (the statistics are in LDS before the first step reads them: the first real step begins with a restart)
        lds_barrier();
        for (int i = S32_DEPTH; i < nst; i += S32_DEPTH) {       // nst is a multiple of three
            step(A0, B0, E0, J0, E1, i, 0);
            step(A1, B1, E1, J1, E2, i + 1, 1);
            step(A2, B2, E2, J2, E0, i + 2, 2);
        }
        __syncthreads();                                 // the schedule and the ring are free for the next round
    }

    SB_T(5);                                             // march done
    strip_marked_cells<HB, S32_NT>(v, cached, limited, sd, rr, r_begin, r_end);
    SB_T(6);                                             // marked cells done
    if (job.update) strip_band_update<HB, S32_NT>(v, cached || store_lists, r_begin, r_end);
    if (job.fold && !(cached && job.lists_stand))        // k_wind's segment lists: with the plan
        sb_compact_segments<S32_NT>(g, job.bandbits, job.seg_list, job.seg_count, job.seg_cap, G, s_scan);
    SB_T(7);                                             // end
}

// single precision only: double precision keeps the tile kernel for radii beyond 16 (see the header of this file)
template <>
hipError_t sb_launch_strip32<float>(const DiagJob<float> &job, int ncu, hipStream_t st) {
    const dim3 gr(ncu), bl(S32_NT);                     // one persistent workgroup per CU
    const StripJob<float> sj = strip_job<float>(job);
    if (!job.wind_final) return hipErrorInvalidValue;   // (the update is k_wind's, or applied behind the march: sb_launch_diag sees to it)
    if (job.t0_fly) hipLaunchKernelGGL((k_strip32<true>), gr, bl, 0, st, sj.plan, sj.plan_gen, sj.fold_partials, ncu, sj);
    else hipLaunchKernelGGL((k_strip32<false>), gr, bl, 0, st, sj.plan, sj.plan_gen, sj.fold_partials, ncu, sj);
    return hipGetLastError();
}
template <>
hipError_t sb_launch_strip32<double>(const DiagJob<double> &, int, hipStream_t) { return hipErrorInvalidValue; }

// the block grid for a domain of nx x rows interior cells; false: the position plane cannot hold it
bool sb_strip32_shape(int nx, int rows, int *ntx, int *nty) {
    *ntx = (nx + S32_SW - 1) / S32_SW;
    *nty = (rows + S32_C - 1) / S32_C;
    return (long long)*ntx * (*nty + 2 * S32_HB) < (long long)S32_MAXW * 64 && *nty + 2 * S32_HB < 0xffff;
}
