// sb_strip_common.hpp -- what the two marching-strip contrast kernels share: k_strip (sb_strip_kernel.hip: search radii up
// to 16, 64-column rows, either precision) and k_strip32 (sb_strip32_kernel.hip: radii up to 31, 96-column rows, single
// precision).   ref: generic/sea_breeze_diag.f90:188-216
// First the pieces -- DPP scans, the flags of a schedule entry, the mark --, then the skeleton of the march: statistics,
// the plan and its planner, the addresses of a staged row, the cell lists, what follows the march.  Every algorithm is
// stated once, as a function of the halo of the tables in blocks (HB); the kernels keep their hot path (issue, stage,
// vertical, query, step), whose code generation is fragile -- see the comments there.
#pragma once
#include "sb_thc_common.hpp"

typedef unsigned long long u64;

// inclusive prefix sums over the 64 lanes of a wave of two 64-bit integers at once: per step and value one
// v_add_co_u32 + one v_addc_co_u32, the lane shift fused into the add (DPP).  The two chains alternate, so a value
// written by one step is read by the next four instructions later (a DPP read needs two wait states after a VALU
// write; hipcc pads nothing inside an asm statement -- hence also the leading s_nop).  Needs all 64 lanes active.
__device__ __forceinline__ void sb_scan2_u64(u64 &a, u64 &b) {
    unsigned al = (unsigned)a, ah = (unsigned)(a >> 32), bl = (unsigned)b, bh = (unsigned)(b >> 32);
#define SB_SCAN_STEP(ctl)                                          \
    "v_add_co_u32_dpp %0, vcc, %0, %0 " ctl "\n\t"               \
    "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc " ctl "\n\t"         \
    "v_add_co_u32_dpp %2, vcc, %2, %2 " ctl "\n\t"               \
    "v_addc_co_u32_dpp %3, vcc, %3, %3, vcc " ctl "\n\t"
    asm volatile("s_nop 1\n\t"
                 SB_SCAN_STEP("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 SB_SCAN_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 0"
                 : "+v"(al), "+v"(ah), "+v"(bl), "+v"(bh)::"vcc");
#undef SB_SCAN_STEP
    a = ((u64)ah << 32) | al;
    b = ((u64)bh << 32) | bl;
}

// ... of one 64-bit integer (rows that lie on one side of the coast: the land-side sums are all zero, or equal the
// sums over all cells); the steps follow each other directly, so each is padded to the two wait states of a DPP read
__device__ __forceinline__ void sb_scan1_u64(u64 &a) {
    unsigned al = (unsigned)a, ah = (unsigned)(a >> 32);
#define SB_SCAN_STEP1(ctl)                                         \
    "v_add_co_u32_dpp %0, vcc, %0, %0 " ctl "\n\t"               \
    "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc " ctl "\n\ts_nop 0\n\t"
    asm volatile("s_nop 1\n\t"
                 SB_SCAN_STEP1("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP1("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP1("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP1("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                 SB_SCAN_STEP1("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 SB_SCAN_STEP1("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 : "+v"(al), "+v"(ah)::"vcc");
#undef SB_SCAN_STEP1
    a = ((u64)ah << 32) | al;
}

__device__ __forceinline__ u64 sb_uniform64(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}

// schedule entry of a step: position | flags
#define SCH_Q2 (1u << 16)          // the block two positions up is active: its band cells are queried in this step's S2
#define SCH_RESTART (1u << 17)     // the block before is not staged: the tables start afresh here
#define SCH_DRAIN (1u << 18)       // no block: the step behind the last block of a run, in which ...
#define SCH_Q1 (1u << 19)          // ... the block one position up (the run's last active one) is queried
#define SCH_IDLE (1u << 20)        // nothing but the loads of the block three steps on (warm-up and padding steps)
#define SCH_QI_SHIFT 22            // bits 22 .. 27: number of the step's cell list in the stored plan

typedef const __attribute__((address_space(4))) u64 *cu64p;          // read-only planes: scalar loads

// A cell whose window outgrows the tables (none on a grid whose distance field was made with a window of at most 15
// cells) is marked during the march -- a NaN of this payload in thc -- and handled after it, by the one copy of the
// global-memory search that the kernel holds (three inlined copies inside the march's loop tripled the code there, and
// a call would have the compiler wait for the prefetched blocks around it).
template <typename T> __device__ __forceinline__ T strip_mark();
template <> __device__ __forceinline__ double strip_mark<double>() { return __longlong_as_double(0x7ff85ea5b4ee2e00ll); }
template <> __device__ __forceinline__ float strip_mark<float>() { return __uint_as_float(0x7fc5ea5bu); }
__device__ __forceinline__ bool strip_is_mark(double v) { return __double_as_longlong(v) == 0x7ff85ea5b4ee2e00ll; }
__device__ __forceinline__ bool strip_is_mark(float v) { return __float_as_uint(v) == 0x7fc5ea5bu; }

// Diagnostic build (-DSB_STAMPS: `make stamps`, tools/stamp_strip.py): every wave leaves the 100 MHz wall clock at a few
// marks -- one scalar clock read and one exec-masked store each, no registers held (an earlier version summed shader
// clocks per phase in 32 registers per lane: the spills that caused distorted what it measured).  Used inside the
// kernels, where job, lane, wv and NWV are in scope.
#if defined(SB_STAMPS) && !defined(SB_STAMPS_WIND)
#define SB_T(i) do { if (lane == 0) job.stamps[(size_t)(blockIdx.x * NWV + wv) * SB_NSTAMP + (i)] = wall_clock64(); } while (0)
#else
#define SB_T(i) do { } while (0)
#endif

// ---- The skeleton of the march, shared: statistics, the plan, the cell lists, what follows the march.  Both kernels cut
// the grid into strips of SBS_SW owned longitudes and blocks of SBS_C rows (one row per wave), keep SBS_DEPTH blocks of
// loads in flight and hold a round of SBS_SCHED steps; a cell's code (row << 5 | column) is built on these.  What
// differs is the halo of the tables in blocks, HB (k_strip: 1, k_strip32: 2): a block is staged if it lies within HB
// positions of an active one, a strip carries HB virtual blocks above and below, and an active block is queried in the
// step that stages the block HB + 1 positions down (a drain step, behind the last block of a run: HB down).
constexpr int SBS_SW = 32, SBS_C = 16, SBS_DEPTH = 3, SBS_SCHED = SB_PLAN_SCHED;
constexpr int SBS_CW_STAGED = 4, SBS_CW_ACTIVE = 2, SBS_CW_RUN = 2;      // cost weights of a share: see strip_plan

// A kernel's state as the shared code sees it: its job, its place in the grid of workgroups, pointers into its LDS.
template <typename T>
struct StripView {
    const StripJob<T> &job;
    const Geo &g;
    int tid, lane, wv;             // (wv is wave-uniform)
    int npad;                      // blocks of a strip incl. the virtual ones above and below
    unsigned npad_magic;           // floor(p / npad) = umulhi(p, magic) for p < 2^16
    int nwords;                    // 64-bit words of the position plane
    char *plan_wg;                 // this workgroup's stored plan: header ...
    unsigned *plan_lists;          // ... and cell lists
    u64 *bits;                     // the active blocks as a bit plane
    uint2 *ent;                    // steps of the round: x = position | flags, y = strip << 16 | block within the padded strip
    unsigned short *cell;          // three cell lists of SBS_SW * SBS_C entries; the planner's prefix array lies over them
    unsigned *cost;                // the planner's cost array (over the first rows of the first table)
    int *misc;                     // [0] steps of the round, [1..3] entries of the three cell lists, [4] a cell was marked,
                                   // [5], [6] the share (ranks of active blocks), [7] totals of the plane,
                                   // [8] the plan of this call is stored (incl. its cell lists),
                                   // [9] query steps of the plan (marked cells, a band step's update)
    Moments *wpart;                // one per wave
    int *scan;                     // one per wave
    T *sdr;                        // the sigmoid scalars, for all waves
    int tot_packed, tot_cost;      // totals of the prefix and cost arrays, in the wave that made them (strip_make_prefix)
};

// ---- statistics.  Returns whether this launch folds k_scan's partial sums (strip_finish_stats then has the scalars
// in v.sdr before the first run); a band step's gathered moments are merged here; otherwise the scalars stand.
template <bool FLY, typename T>
__device__ __forceinline__ bool strip_begin_stats(const StripView<T> &v, const Moments *fold_partials, T &sd, T &rr, Moments &pm, double &shift_c) {
    const StripJob<T> &job = v.job;
    const bool fold_stats = job.fold && job.fold_nparts > 0;
    if (fold_stats) {
        if (v.tid < job.fold_nparts) pm = fold_partials[v.tid];
        shift_c = (double)job.sigma[(size_t)v.g.h * v.g.nxh + v.g.h];
    } else if (FLY && job.ngath > 0) {
        // band step: the first wave merges the moments gathered from all ranks in rank order (one tree on every
        // workgroup of every rank: identical scalars everywhere); workgroup 0 publishes them
        if (v.wv == 0) {
            Moments m = moments_empty();
            for (int b = v.lane; b < job.ngath; b += SB_WAVE) m = moments_merge(m, job.gath[b]);
            m = wave_merge(m);
            if (v.lane == 0) {
                T st4[4];
                sigmoid_scalars<T>(m, st4);
                v.sdr[0] = st4[0]; v.sdr[1] = st4[1];
                if (blockIdx.x == 0) { for (int i = 0; i < 4; ++i) job.stats_out[i] = st4[i]; }
            }
        }
    } else if (FLY) { sd = job.stats[0]; rr = job.stats[1]; }
    return fold_stats;
}
// k_scan's shifted sums added up in k_prep's order and turned into the sigmoid scalars -- two divisions and a square
// root in fp64, some 200 dependent instructions -- by the FIRST wave alone (the oldest wave of its SIMD has priority
// at issue: it comes through the code in front of the march in half the time the last one takes, and everybody
// waits for these scalars); all pick them up behind the barrier that opens the first run.  Workgroup 0 publishes
// them (for the calls that reuse them: static sigma), with or without a share of the march.
template <int NWV, typename T>
__device__ __forceinline__ void strip_finish_stats(const StripView<T> &v, double shift_c) {
    if (v.wv == 0) {
        const Moments m = moments_of_shifted(shift_c, block_total_shifted_finish<NWV>(v.wpart));
        T st4[4];
        sigmoid_scalars<T>(m, st4);
        if (v.lane == 0) {
            v.sdr[0] = st4[0]; v.sdr[1] = st4[1];
            if (blockIdx.x == 0) { for (int i = 0; i < 4; ++i) v.job.stats_out[i] = st4[i]; }
        }
    }
}

// ---- the plan.  Which blocks this workgroup marches over, in which order, and where their band cells lie follows
// from the band plane alone, and a coast does not move: the plan is stored in device memory (steps and cell
// lists), and k_scan -- which rewrites the plane every call -- compares each word with the one it replaces and
// leaves the number of the last call that saw a difference.  A plan stored by that call or a later one is used as
// it is: no flags are read, nothing is planned, no list is built.
// Returns whether the stored plan stands (uniform).  If so its steps and share are in LDS; if not, the flags k_scan
// raised are, NT at a time, as a bit plane (word c NWV + wv = ballot of chunk c; nch chunks <= MAXW / 16: host).
template <int NT, typename T>
__device__ __forceinline__ bool strip_load_plan(const StripView<T> &v, const int *plan_gen, int npos, int nch) {
    typedef const __attribute__((address_space(4))) int *cintp;
    const StripJob<T> &job = v.job;
    const int tid = v.tid;
    // (the stored plan's steps travel WITH its header -- one round trip, not two; used only if the plan stands)
    const uint2 plan_ent = ((const uint2 *)(v.plan_wg + SB_PLAN_ENT_OFF))[tid < SBS_SCHED ? tid : 0];
    const int plan_stored = ((cintp)v.plan_wg)[0], plan_nst = min(((cintp)v.plan_wg)[1], SBS_SCHED);
    const int plan_rb = ((cintp)v.plan_wg)[2], plan_re = ((cintp)v.plan_wg)[3];
    const bool cached = job.plan_use != 0 && plan_stored != 0 && *(cintp)plan_gen <= plan_stored;      // uniform
    if (__builtin_expect(!cached, 0)) {
        u64 mine = 0;
        for (int base = 0; base < nch; base += 8) {              // 8 loads in flight (clamped, so none is conditional)
            int f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = (base + j) * NT + tid;
                f[j] = job.flags[i < npos ? i : npos - 1];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = (base + j) * NT + tid;
                mine |= (i < npos && f[j] != 0) ? 1ull << (base + j) : 0ull;
            }
        }
        for (int c = 0; c < nch; ++c) {
            const u64 b = __builtin_amdgcn_ballot_w64((mine >> c) & 1ull);
            if (v.lane == 0) v.bits[c * (NT / SB_WAVE) + v.wv] = b;
        }
    } else {
        if (tid < plan_nst) v.ent[tid] = plan_ent;      // (at most SBS_SCHED < NT steps)
        if (tid == 0) { v.misc[0] = plan_nst; v.misc[5] = plan_rb; v.misc[6] = plan_re; v.misc[8] = 0; }
    }
    return cached;
}

// ---- the planner: ONE WAVE.
__device__ __forceinline__ void strip_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }      // this wave's LDS writes have landed
template <int HB, typename T>
__device__ __forceinline__ u64 strip_stage_word(const StripView<T> &v, int k) {      // staged = within HB positions of an active block
    const u64 a = v.bits[k], pv = k > 0 ? v.bits[k - 1] : 0ull, nx = k + 1 < v.nwords ? v.bits[k + 1] : 0ull;
    u64 s = a;                                           // (virtual blocks separate the strips)
#pragma unroll
    for (int d = 1; d <= HB; ++d) s |= (a << d) | (pv >> (64 - d)) | (a >> d) | (nx << (64 - d));
    return s;
}
template <int HB, typename T>
__device__ __forceinline__ u64 strip_run_starts(const StripView<T> &v, int k, u64 sw) {      // staged blocks of word k whose predecessor is not staged
    const u64 swp = k > 0 ? strip_stage_word<HB>(v, k - 1) : 0ull;
    return sw & ~((sw << 1) | (swp >> 63));
}
// Per word of the plane: active and staged blocks before it, packed (low / high 16 bits) -- the array lies where
// the cell lists of the march will (they are not in use while a round is planned) -- and the cost before it, where
// the first rows of the first table will.
template <int HB, typename T>
__device__ __forceinline__ void strip_make_prefix(StripView<T> &v, bool with_cost) {
    unsigned *s_pre = (unsigned *)v.cell;
    const int lane = v.lane, nwords = v.nwords;
    int run = 0, crun = 0;
    for (int k0 = 0; k0 < nwords; k0 += SB_WAVE) {
        const int k = k0 + lane;
        const u64 a = k < nwords ? v.bits[k] : 0ull, sw = k < nwords ? strip_stage_word<HB>(v, k) : 0ull;
        const int pk = (int)((unsigned)__popcll(a) | (unsigned)__popcll(sw) << 16);
        const int incl = sb_wave_scan_add(pk);
        if (k < nwords) s_pre[k] = (unsigned)(run + incl - pk);
        run += __builtin_amdgcn_readlane(incl, SB_WAVE - 1);
        if (with_cost) {
            const int c = SBS_CW_STAGED * __popcll(sw) + SBS_CW_ACTIVE * __popcll(a) + SBS_CW_RUN * __popcll(k < nwords ? strip_run_starts<HB>(v, k, sw) : 0ull);
            const int cincl = sb_wave_scan_add(c);
            if (k < nwords) v.cost[k] = (unsigned)(crun + cincl - c);
            crun += __builtin_amdgcn_readlane(cincl, SB_WAVE - 1);
        }
    }
    v.tot_packed = run;
    v.tot_cost = crun;
    if (lane == 0) v.misc[7] = run;
    strip_wave_sync();
}
// the word that holds rank t of the packed prefix (hi: staged, else active) and the rank inside it; wave-uniform
template <typename T>
__device__ __forceinline__ int strip_find_word(const StripView<T> &v, int t, bool hi, int &n) {
    const unsigned *s_pre = (const unsigned *)v.cell;
    const int nwords = v.nwords;
    int kk = -1;
    n = 0;
    for (int k0 = 0; k0 < nwords; k0 += SB_WAVE) {
        const int k = k0 + v.lane;
        const unsigned pa = k < nwords ? s_pre[k] : 0u, pb = k + 1 < nwords ? s_pre[k + 1] : (unsigned)v.tot_packed;
        const int lo = (int)(hi ? pa >> 16 : pa & 0xffffu), up = (int)(hi ? pb >> 16 : pb & 0xffffu);
        const u64 hit = __builtin_amdgcn_ballot_w64(k < nwords && lo <= t && t < up);
        if (hit) {
            const int src = __ffsll((unsigned long long)hit) - 1;
            kk = k0 + src;
            n = t - __builtin_amdgcn_readlane(lo, src);
            break;
        }
    }
    return kk;
}
__device__ __forceinline__ int strip_nth_bit(u64 word, int n, int lane) {      // position of the n-th set bit (lane j looks at bit j)
    const bool me = ((word >> lane) & 1ull) && __popcll(word & ((1ull << lane) - 1ull)) == n;
    return __ffsll((unsigned long long)__builtin_amdgcn_ballot_w64(me)) - 1;
}
// position of the active block of rank r (-1: none); wave-uniform
template <typename T>
__device__ __forceinline__ int strip_block_of_rank(const StripView<T> &v, int r) {
    int n;
    const int kw = strip_find_word(v, r, false, n);
    return kw < 0 ? -1 : kw * 64 + strip_nth_bit(sb_uniform64(v.bits[kw < 0 ? 0 : kw]), n, v.lane);
}
// active blocks in front of the position at which the running cost reaches t (all of them beyond the total)
template <int HB, typename T>
__device__ __forceinline__ int strip_act_before_cost(const StripView<T> &v, int t) {
    const unsigned *s_pre = (const unsigned *)v.cell;
    const int lane = v.lane, nwords = v.nwords;
    const int nact = v.tot_packed & 0xffff;
    if (t >= v.tot_cost) return nact;
    for (int k0 = 0; k0 < nwords; k0 += SB_WAVE) {
        const int k = k0 + lane;
        const int lo = k < nwords ? (int)v.cost[k] : 0x7fffffff, up = k + 1 < nwords ? (int)v.cost[k + 1] : v.tot_cost;
        const u64 hit = __builtin_amdgcn_ballot_w64(k < nwords && lo <= t && t < up);
        if (hit) {                                   // wave-uniform: the word in which the cost crosses t
            const int src = __ffsll((unsigned long long)hit) - 1, kk = k0 + src;
            const u64 a = sb_uniform64(v.bits[kk]), sw = sb_uniform64(strip_stage_word<HB>(v, kk));
            const u64 rs = sb_uniform64(strip_run_starts<HB>(v, kk, strip_stage_word<HB>(v, kk)));
            const u64 upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;       // bits 0 .. lane
            const int cum = __builtin_amdgcn_readlane(lo, src) + SBS_CW_STAGED * __popcll(sw & upto) + SBS_CW_ACTIVE * __popcll(a & upto) + SBS_CW_RUN * __popcll(rs & upto);
            const u64 over = __builtin_amdgcn_ballot_w64(cum > t);
            const int bpos = over ? __ffsll((unsigned long long)over) - 1 : 63;       // the first position behind the crossing
            return (int)(__builtin_amdgcn_readfirstlane((int)s_pre[kk]) & 0xffff) + __popcll(a & ((1ull << bpos) - 1ull));
        }
    }
    return nact;
}
// The schedule of the round that holds the active blocks of ranks [ra, rb): the staged positions in ascending
// order with their flags, a drain step behind every run, three warm-up steps in front (they stage nothing and only
// issue the loads of the first three blocks, so that every load of the march is issued at the same three program
// points -- see the kernels' `step`), padded to a multiple of three.  One lane per position, 64 positions at a time.
// Leaves the number of steps in misc[0].
template <int HB, typename T>
__device__ __forceinline__ void strip_make_schedule(const StripView<T> &v, int ra, int rb) {
    const int lane = v.lane, npad = v.npad;
    const int p0 = strip_block_of_rank(v, ra), p1 = strip_block_of_rank(v, rb - 1);
    strip_wave_sync();                                   // (the prefix array may be overwritten from here on)
    if (p0 < HB || p1 < p0) { if (lane == 0) v.misc[0] = 0; return; }     // (cannot happen: the first HB positions are virtual)
    if (lane < SBS_DEPTH) v.ent[lane] = make_uint2(SCH_DRAIN | SCH_IDLE, 0u);
    if (lane < 3) v.misc[1 + lane] = 0;
    int n_out = SBS_DEPTH;
    constexpr unsigned near = (1u << (2 * HB + 1)) - 1u;  // 2 HB + 1 neighbouring positions, as bits of the window below
    for (int c = p0 - HB; c <= p1 + HB; c += SB_WAVE) {
        const int pp = c + lane;
        // active blocks (of this round) at positions pp - (HB + 1) .. pp + (HB + 1): bits 0 .. 2 HB + 2
        unsigned win = 0;
#pragma unroll
        for (int d = 0; d < 2 * HB + 3; ++d) {
            const int q = pp + d - (HB + 1);
            const bool in = q >= p0 && q <= p1;
            const u64 w = v.bits[in ? q >> 6 : 0];
            win |= (in && ((w >> (q & 63)) & 1ull)) ? 1u << d : 0u;
        }
        const bool st = pp <= p1 + HB && (win & (near << 1)) != 0u;           // pp - HB .. pp + HB
        // (a run never crosses from one strip into the next: the last virtual block of a strip ends it, the first one of
        // the next strip starts afresh -- the blocks of a run are queried by their position within ONE strip; found on
        // a grid whose band reaches the first and the last row)
        const int sp = (int)__umulhi((unsigned)(pp < 0 ? 0 : pp), v.npad_magic), jpp = pp - sp * npad;
        const bool st_prev = (win & near) != 0u && jpp != 0, st_next = (win & (near << 2)) != 0u && jpp != npad - 1;
        const bool en = st && !st_next;
        const u64 ms = __builtin_amdgcn_ballot_w64(st), me = __builtin_amdgcn_ballot_w64(en);
        const u64 below = (1ull << lane) - 1ull;
        const int at = n_out + __popcll(ms & below) + __popcll(me & below);
        n_out += __popcll(ms) + __popcll(me);
        if (st) {
            const unsigned sjv = ((unsigned)sp << 16) | (unsigned)jpp;
            const unsigned e = (unsigned)pp | ((win & 1u) ? SCH_Q2 : 0u) | (st_prev ? 0u : SCH_RESTART);
            if (at < SBS_SCHED) v.ent[at] = make_uint2(e, sjv);
            // (the run ends at pp: the block HB up is the run's last active one)
            if (en && at + 1 < SBS_SCHED) v.ent[at + 1] = make_uint2((unsigned)pp | SCH_DRAIN | ((win & 2u) ? SCH_Q1 : 0u), sjv);
        }
    }
    // (padded to a multiple of three with steps that do nothing: the march has no early exit -- with one, the
    // compiler's count of the loads in flight collapses and it drains the queue every third step)
    // (The padding steps' dummy loads go where the last real step's went -- same strip, same block: no column
    // arithmetic, lines that are in the cache.  A padding step cost 0.45 us, and the longest-lived workgroups of
    // the headline grid have two.)
    n_out = min(n_out, SBS_SCHED - 2);
    const int n_pad = (n_out + SBS_DEPTH - 1) / SBS_DEPTH * SBS_DEPTH;
    strip_wave_sync();
    const unsigned last_sj = v.ent[n_out - 1].y;         // (n_out >= SBS_DEPTH + 1 here)
    if (lane < n_pad - n_out) v.ent[n_out + lane] = make_uint2(SCH_DRAIN | SCH_IDLE, last_sj);
    if (lane == 0) v.misc[0] = n_pad;
}
// does the step of entry x query a block?  (a drain step: the block HB up; else: the block HB + 1 up)
__device__ __forceinline__ bool strip_step_queries(unsigned x) {
    return !(x & SCH_IDLE) && (x & ((x & SCH_DRAIN) ? SCH_Q1 : SCH_Q2)) != 0u;
}
// WAVE 0 ALONE (the others wait at one barrier): this workgroup's share and the schedule of its first round of at most
// ROUND active blocks.  Shares are equal in COST, in strip-major order.  The marks of tools/stamp_strip.py, fitted over
// the 256 workgroups of the headline grid, give a workgroup's life as 1.25 us per staged block (an active block or a
// neighbour of one) + 0.56 us per active block (its band cells are queried) + 0.68 us per run (drain step, restart):
// weights 4 : 2 : 2.  Workgroup b takes the active blocks at which the running cost lies in [b, b + 1) T / G.  (An
// equal share of active blocks left the workgroup with the most short runs with 15 staged blocks against a mean of
// 10; an equal share of staged blocks still had lives of 20 .. 30 us around a mean of 25.)
// The plan goes to device memory: the steps, each query step with the number of its cell list (the lists themselves
// are written by the waves that query them); a share of several rounds, or of more query steps than a stored plan
// holds, is planned every call.
template <int HB, int ROUND, typename T>
__device__ __forceinline__ void strip_plan(StripView<T> &v, int G) {
    const int lane = v.lane;
    strip_make_prefix<HB>(v, true);
    const int rb0 = strip_act_before_cost<HB>(v, (int)(((long long)blockIdx.x * v.tot_cost) / G));
    const int re0 = blockIdx.x + 1 == (unsigned)G ? (v.tot_packed & 0xffff) : strip_act_before_cost<HB>(v, (int)(((long long)(blockIdx.x + 1) * v.tot_cost) / G));
    if (lane == 0) { v.misc[5] = rb0; v.misc[6] = re0; v.misc[0] = 0; }
    if (rb0 < re0) strip_make_schedule<HB>(v, rb0, min(rb0 + ROUND, re0));
    strip_wave_sync();
    const int nstv = __builtin_amdgcn_readfirstlane(v.misc[0]);
    int nq = 0;
    uint2 *eg = (uint2 *)(v.plan_wg + SB_PLAN_ENT_OFF);
    for (int c0 = 0; c0 < nstv; c0 += SB_WAVE) {
        const int i = c0 + lane;
        uint2 e = v.ent[i < nstv ? i : 0];
        const bool q = i < nstv && strip_step_queries(e.x);
        const u64 m = __builtin_amdgcn_ballot_w64(q);
        const int qi = nq + __popcll(m & ((1ull << lane) - 1ull));
        nq += __popcll(m);
        if (q) e.x |= (unsigned)(qi & (SB_PLAN_NQ - 1)) << SCH_QI_SHIFT;
        if (i < nstv) { v.ent[i] = e; eg[i] = e; }
    }
    const bool ok = re0 - rb0 <= ROUND && nq <= SB_PLAN_NQ;
    if (lane == 0) {
        int *h = (int *)v.plan_wg;
        h[1] = nstv; h[2] = rb0; h[3] = re0;
        h[0] = ok ? v.job.call_id : 0;
        v.misc[8] = ok ? 1 : 0;
    }
}

// ---- addresses of the march's loads
// how far a window round (x, y) may reach inside a ghost-celled frame: the ghost width beyond the interior -- except
// in the directions in which a band's frame is not an edge at all (round the circle; beyond a pole)
__device__ __forceinline__ int strip_frame_reach(const Geo &g, int x, int y) {
    const int big_reach = 1 << 20;
    const int rx = (g.band & GEO_BAND_EW) ? big_reach : min(x + g.h, g.nx - 1 - x + g.h);
    const int rs = (g.band & GEO_BAND_SOUTH) ? big_reach : y + g.h, rn = (g.band & GEO_BAND_NORTH) ? big_reach : g.ny - 1 - y + g.h;
    return min(rx, min(rs, rn));
}
// column xs of the interior (may lie outside it) as a staged row loads it: byte offsets in a row of a field of `esize`-byte
// elements and in a row of the land-side plane, bit in the 32-bit word (0: no such cell, or a lane that is not `live`).
// fastx: nx exceeds the staged width by more than two, so one conditional add wraps every column of a staged row.
__device__ __forceinline__ void strip_column(const Geo &g, bool fastx, unsigned esize, int xs, bool live, unsigned &colb, unsigned &clsb, unsigned &lbit) {
    bool ok = live;
    int Xc = 0;
    if (g.bnd == BND_HALO) {
        int xw = xs;
        if (g.band & GEO_BAND_EW) xw = xs < 0 ? xs + g.nx : (xs >= g.nx ? xs - g.nx : xs);   // (a band holds whole circles, wider than a staged row)
        Xc = xw + g.h; ok = ok && Xc >= 0 && Xc < g.nxh;
    }
    else if (fastx) {
        if (g.bnd == BND_WRAPPER) {
            int m = xs + 1;
            m = m < 0 ? m + g.nx : (m >= g.nx ? m - g.nx : m);
            Xc = (m < 1 ? 1 : m) - 1;
        } else Xc = xs < 0 ? xs + g.nx : (xs >= g.nx ? xs - g.nx : xs);
    } else {
        int Yd;
        sb_map_cell(g, xs, 0, Xc, Yd);
    }
    const unsigned xc = ok ? (unsigned)Xc : 0u;      // every load is unconditional, from a clamped address
    colb = xc * esize;
    clsb = (xc >> 5) * 4u;
    lbit = ok ? 1u << (xc & 31u) : 0u;
}
// interior row ys (may lie outside the grid) -> the array row its loads go to (clamped); rowok: the row exists
__device__ __forceinline__ int strip_row(const Geo &g, int ys, bool &rowok) {
    int Yr;
    rowok = true;
    if (g.bnd == BND_HALO) {
        int yw = ys;
        if ((g.band & GEO_BAND_SOUTH) && yw < 0) yw = 0;          // beyond a pole: the edge row again (the latitude clamp)
        if ((g.band & GEO_BAND_NORTH) && yw >= g.ny) yw = g.ny - 1;
        Yr = yw + g.h; rowok = Yr >= 0 && Yr < g.nyh; Yr = rowok ? Yr : 0;
    }
    else Yr = ys < 0 ? 0 : (ys >= g.ny ? g.ny - 1 : ys);
    return Yr;
}
// a step's entry travels in scalar registers from the step that issues its block's loads (three steps ahead)
// to the step itself; behind the end of the schedule: idle steps
__device__ __forceinline__ void strip_entry(const uint2 *s_ent, int nst, int i, unsigned &e, unsigned &j) {
    const uint2 v = s_ent[i < nst ? i : nst - 1];
    e = i < nst ? (unsigned)__builtin_amdgcn_readfirstlane((int)v.x) : (SCH_DRAIN | SCH_IDLE);
    j = (unsigned)__builtin_amdgcn_readfirstlane((int)v.y);
}

// ---- the cell lists (the planning call only: a stored plan holds them)
// The band bits of the two rows this wave lists in block jp of `strip`, as SCALAR loads (constant address space: the
// plane is k_scan's, read-only here).  Scalar loads count in lgkmcnt, not in the in-order vmcnt queue of the
// prefetched blocks: a vector load here would sit between them, and the wait for it would drain every load
// issued before it.
struct BandWords { u64 a0, b0, a1, b1, c0, c1; int sh; };   // c: land-side word of the last longitude (f2py rule)
template <int HB, typename T>
__device__ __forceinline__ BandWords strip_band_issue(const StripJob<T> &job, const Geo &g, int wv, int strip, int jp) {
    constexpr int SW = SBS_SW, C = SBS_C;
    const int k = max(wv - C / 2, 0);                // the listing waves are 8 .. 15: two rows each
    const int y0 = (jp - HB) * C + 2 * k;
    const int ya = min(max(y0, 0), g.ny - 1), yb = min(max(y0 + 1, 0), g.ny - 1);
    const int xa = strip * SW + g.h;                 // array column of the strip's first owned cell
    const int wlo = xa >> 6, whi = min(wlo + 1, g.nw - 1);
    cu64p bits = (cu64p)job.bandbits;
    BandWords w;
    w.a0 = bits[(size_t)(ya + g.h) * g.nw + wlo]; w.b0 = bits[(size_t)(ya + g.h) * g.nw + whi];
    w.a1 = bits[(size_t)(yb + g.h) * g.nw + wlo]; w.b1 = bits[(size_t)(yb + g.h) * g.nw + whi];
    w.sh = xa & 63;
    w.c0 = w.c1 = 0;
    if (g.bnd == BND_WRAPPER && strip == job.ntx - 1) {      // uniform; the strip that owns longitude nx
        cu64p cls = (cu64p)job.clsbits;
        const int wl = (g.nx - 1 + g.h) >> 6;
        w.c0 = cls[(size_t)(ya + g.h) * g.nw + wl]; w.c1 = cls[(size_t)(yb + g.h) * g.nw + wl];
    }
    return w;
}
// Waves 8-15: the band cells of two rows of the queried block -> the step's compact list (n_cell: its length).  A cell's
// code is row << 5 | column (cell_code: the lane's, see strip_cell_code), plus (f2py rule, last longitude only) bit 10 and
// in bit 9 its own land-side bit -- see `query`.  The waves reserve their entries with one LDS atomic each: the order
// of the list is of no consequence.
__device__ __forceinline__ unsigned strip_cell_code(int wv, int lane) {
    return (unsigned)((2 * max(wv - SBS_C / 2, 0) + (lane >> 5)) << 5 | (lane & (SBS_SW - 1)));
}
template <int HB, typename T>
__device__ __forceinline__ void strip_list_cells(const StripJob<T> &job, const Geo &g, int wv, int lane, unsigned cell_code, int strip, int jp,
                                                 const BandWords &bwd, unsigned short *s_cell, int *n_cell) {
    constexpr int SW = SBS_SW, C = SBS_C;
    // the wave's 64 band bits (lanes 0-31: first row, 32-63: second) by scalar funnel shifts of the four words
    const int y0 = (jp - HB) * C + 2 * max(wv - C / 2, 0);
    const int ncol = min(g.nx - strip * SW, SW);      // owned columns that exist (the last strip may be cut)
    const unsigned colmask = ncol >= 32 ? 0xffffffffu : (1u << ncol) - 1u;
    auto row_bits = [&](u64 a, u64 b2, int y) -> unsigned {
        const u64 f = bwd.sh ? (a >> bwd.sh) | (b2 << (64 - bwd.sh)) : a;
        return (y >= 0 && y < g.rows) ? (unsigned)f & colmask : 0u;
    };
    const u64 m = (u64)row_bits(bwd.a0, bwd.b0, y0) | (u64)row_bits(bwd.a1, bwd.b1, y0 + 1) << 32;
    if (m == 0) return;                              // wave-uniform
    unsigned code = cell_code;
    if (g.bnd == BND_WRAPPER && strip == job.ntx - 1) {      // uniform: the strip that owns the last longitude
        if (strip * SW + (int)(lane & (SW - 1)) == g.nx - 1) {
            const unsigned sl = (unsigned)((g.nx - 1 + g.h) & 63);
            code |= 1u << 10 | (unsigned)(((lane >> 5) ? (bwd.c1 >> sl) : (bwd.c0 >> sl)) & 1ull) << 9;
        }
    }
    int base = 0;
    if (lane == 0) base = atomicAdd(n_cell, __popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    const unsigned at = (unsigned)base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if ((m >> lane) & 1ull) s_cell[at] = (unsigned short)code;
}

// ---- behind the march
// the global-memory search for one marked cell; everything it needs comes from the job's copy in device memory
template <typename T>
__device__ __forceinline__ void strip_slow_cell(const StripView<T> &v, const DiagJob<T> &cj, bool limited, T sd, T rr, int x, int y, int &nnmax) {
    const Geo &g = v.g;
    const unsigned o = (unsigned)y * (unsigned)g.nx + (unsigned)x;
    int cap = g.nx + g.ny;
    if (limited) cap = min(cap, strip_frame_reach(g, x, y));
    bool one_class;
    const T cg = contrast_global(cj, x, y, cap, sd, rr, nnmax, one_class);
    atomicAdd(&cj.counters[0], 1);
    if (one_class) atomicAdd(&cj.counters[1], 1);
    const T mulg = sb_bit(cj.clsbits, g.nw, x + g.h, y + g.h) ? T(1) : T(-1);
    v.job.thc[o] = mulg * cg;
}
// strip << 16 | block of every query step's list of the plan in LDS -> s_qblk (over the cell lists); returns the number
// of lists.  All threads.
template <int HB, int NT, typename T>
__device__ __forceinline__ int strip_list_blocks(const StripView<T> &v, int *s_qblk) {
    __syncthreads();
    if (v.tid == 0) v.misc[9] = 0;
    __syncthreads();
    const int nstp = v.misc[0];
    for (int i = v.tid; i < nstp; i += NT) {
        const uint2 e = v.ent[i];
        if (strip_step_queries(e.x)) {
            const int qi = (int)((e.x >> SCH_QI_SHIFT) & (SB_PLAN_NQ - 1));
            s_qblk[qi] = (int)((e.y & 0xffff0000u) | ((e.y & 0xffffu) - ((e.x & SCH_DRAIN) ? (unsigned)HB : (unsigned)(HB + 1))));
            atomicMax(&v.misc[9], qi + 1);
        }
    }
    __syncthreads();
    return v.misc[9];
}
// the band cell of thread tid in the block at position pos (every thread of the first SBS_SW * SBS_C has one); false: none
template <int HB, typename T>
__device__ __forceinline__ bool strip_band_cell_of(const StripView<T> &v, int pos, int &x, int &y) {
    const Geo &g = v.g;
    const int strip = pos / v.npad, jp = pos - strip * v.npad;
    x = strip * SBS_SW + (v.tid & (SBS_SW - 1)); y = (jp - HB) * SBS_C + (v.tid >> 5);
    return v.tid < SBS_SW * SBS_C && x < g.nx && y >= 0 && y < g.rows && sb_bit(v.job.bandbits, g.nw, x + g.h, y + g.h);
}
// The marked cells (rare: misc[4]): every band cell of this workgroup's blocks (ranks [r_begin, r_end)) that holds the
// mark takes the global-memory search.  All threads, behind the last round's barrier.
template <int HB, int NT, typename T>
__device__ __forceinline__ void strip_marked_cells(StripView<T> &v, bool cached, bool limited, T sd, T rr, int r_begin, int r_end) {
    constexpr int SW = SBS_SW, C = SBS_C;
    const StripJob<T> &job = v.job;
    if (v.misc[4] == 0) return;                          // (uniform)
    const DiagJob<T> &cj = *job.cold;
    if (cached) {
        // A stored plan knows its marked cells: the entries of its lists whose radius field is zero -- no flags read,
        // no plane ranked.
        int *s_qblk = (int *)v.cell;
        const int nq = strip_list_blocks<HB, NT>(v, s_qblk);
        for (int q = 0; q < nq; ++q) {
            const unsigned code = v.tid < SW * C ? v.plan_lists[(unsigned)q * (unsigned)(SW * C) + (unsigned)v.tid] : ~0u;
            if (code != ~0u && ((code >> 10) & 31u) == 0u) {
                const int blk = s_qblk[q];
                const int strip = blk >> 16, jp = blk & 0xffff;
                int nnmax = 0;
                strip_slow_cell(v, cj, limited, sd, rr, strip * SW + (int)(code & 31u), (jp - HB) * C + (int)((code >> 5) & 15u), nnmax);
                if (nnmax > 1) atomicMax(&job.flags[strip * v.npad + jp], nnmax);
            }
        }
        __syncthreads();                                 // (a band step's update lays its own table over the cell lists)
    } else {
        if (v.wv == 0) strip_make_prefix<HB>(v, false);  // the prefix array again (the cell lists lay over it)
        __syncthreads();
        v.tot_packed = v.misc[7];
        for (int r = r_begin; r < r_end; ++r) {
            const int pos = strip_block_of_rank(v, r);
            if (pos < 0) break;
            int nnmax = 0, x, y;
            if (strip_band_cell_of<HB>(v, pos, x, y)) {
                if (strip_is_mark(job.thc[(unsigned)y * (unsigned)v.g.nx + (unsigned)x])) strip_slow_cell(v, cj, limited, sd, rr, x, y, nnmax);
            }
            if (nnmax > 1) atomicMax(&job.flags[pos], nnmax);
        }
    }
}
// A band step (job.update): k_wind ran ahead of the ghost rows and left this call's winds in scratch planes; thresholds,
// scaling and state update (ref :235-266) of every band cell this workgroup queried, now that thc holds its
// contrast.  Behind the march, not inside it: a cell's winds and state loaded in a step would drain the blocks the
// march keeps in flight.  The cells come from the plan's lists (have_lists: stored, or written by this very launch); four
// list rows per wave in flight.  thc is read past the L1 (other waves of this workgroup wrote it).
template <int HB, int NT, typename T>
__device__ __forceinline__ void strip_band_update(StripView<T> &v, bool have_lists, int r_begin, int r_end) {
    constexpr int SW = SBS_SW, C = SBS_C, NWV = NT / SB_WAVE;
    const StripJob<T> &job = v.job;
    const Geo &g = v.g;
    __syncthreads();
    const DiagJob<T> &cj = *job.cold;
    auto apply = [&](unsigned o) __attribute__((always_inline)) {
        const T n_thc = __hip_atomic_load(&job.thc[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sb_trigger_update<T, false>(cj, (size_t)o, n_thc, sb_trigger_load<T>(cj, (size_t)o));
    };
    if (have_lists) {
        int *s_qblk = (int *)v.cell;
        const int nrows = strip_list_blocks<HB, NT>(v, s_qblk) * (C / 2);        // eight rows of 64 entries per list
        for (int r0 = v.wv; r0 < nrows; r0 += 4 * NWV) {
            unsigned code[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = r0 + k * NWV;
                code[k] = ~0u;
                if (r < nrows) code[k] = __hip_atomic_load(&v.plan_lists[(unsigned)(r >> 3) * (unsigned)(SW * C) + (unsigned)((r & 7) * SB_WAVE + v.lane)],
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (code[k] == ~0u) continue;
                const int blk = s_qblk[(r0 + k * NWV) >> 3];
                const int x = (blk >> 16) * SW + (int)(code[k] & 31u), y = ((blk & 0xffff) - HB) * C + (int)((code[k] >> 5) & 15u);
                apply((unsigned)y * (unsigned)g.nx + (unsigned)x);
            }
        }
    } else {
        // (no lists: a share of several rounds, or of more query steps than a plan holds -- block by block)
        if (v.wv == 0) strip_make_prefix<HB>(v, false);
        __syncthreads();
        v.tot_packed = v.misc[7];
        for (int r = r_begin; r < r_end; ++r) {
            const int pos = strip_block_of_rank(v, r);
            if (pos < 0) break;
            int x, y;
            if (strip_band_cell_of<HB>(v, pos, x, y)) apply((unsigned)y * (unsigned)g.nx + (unsigned)x);
        }
    }
}

// the hot part of the job, by value; everything else the kernel reads -- rarely -- from the copy of the whole job that
// k_scan leaves in device memory (job.self)
template <typename T>
static StripJob<T> strip_job(const DiagJob<T> &job) {
    StripJob<T> s;
    s.g = job.g;
    s.theta = job.t0_fly ? job.theta : job.t0; s.z = job.z; s.sigma = job.sigma;
    s.clsbits = job.clsbits; s.bandbits = job.bandbits;
    s.thc = job.thc;
    s.flags = job.tile_nnmax;
    s.ntx = job.thc_ntx; s.nty = job.thc_nty;
    s.fold = job.fold; s.fold_nparts = job.fold_nparts; s.ngath = job.ngath; s.seg_cap = job.seg_cap;
    s.lists_stand = job.lists_stand;
    s.stats = job.stats; s.stats_out = job.stats_out;
    s.fold_partials = job.fold_partials; s.gath = job.gath;
    s.seg_list = job.seg_list; s.seg_count = job.seg_count;
    s.cold = job.self;
    s.plan = job.plan; s.plan_gen = job.plan_gen; s.call_id = job.call_id; s.plan_use = job.plan_use;
    s.update = job.strip_update;
    s.stamps = job.stamps;
    return s;
}
