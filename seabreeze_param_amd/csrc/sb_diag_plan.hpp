// sb_diag_plan.hpp -- which kernels a diag call enqueues, in which order and in which mode, and which of the context's opt-in
// switches serve it: decided here, in pure functions, and nowhere else.  run_diag (sb_capi.hip) hands sb_apply_switches the
// switches and what it knows of the call, sizes its workspace from the plan, sb_launch_diag (sb_diag_kernels.hip) walks its
// steps, band_diag_dev asks sb_band_folds_frame which ghost cells of theta a band step fills.  Plain C++17: no HIP, no pointers,
// no heap -- a host compiler builds it alone (tests/plan_dump.cpp).
#pragma once

// kernels of a diag call that sb_profile_begin / sb_profile_end time, each with its own pair of events
enum { SB_PROF_NONE = -1, SB_PROF_SCAN = 0, SB_PROF_WIND = 1, SB_PROF_T0 = 2, SB_PROF_THC = 3, SB_PROF_PREP = 4, SB_PROF_KERNELS = 5 };
// (SB_K_TABLE_ROWS, SB_K_TABLE_COLS: the two passes that build the device-wide summed-area tables, sb_table_kernels.hip)
enum SbKernel { SB_K_SCAN, SB_K_PREP, SB_K_MERGE, SB_K_T0, SB_K_CONTRAST, SB_K_WIND, SB_K_TABLE_ROWS, SB_K_TABLE_COLS };
// sigma's statistics in a step.  k_scan: PARTIALS = it forms them; k_prep and the contrast kernel merge k_scan's `nparts`
// partial moments (0: the scalars stand) or, as k_merge_moments does, the moments GATHERED from every band
enum SbStatsSrc { SB_STATS_NONE, SB_STATS_PARTIALS, SB_STATS_GATHERED };
// the LDS halo for a search-radius hint (32: the largest a contrast kernel is instantiated for)
inline int sb_pick_halo(int r) { return r <= 8 ? 8 : r <= 16 ? 16 : r <= 24 ? 24 : 32; }
// A strip kernel that does k_prep's work merges k_scan's partial moments with one thread each.  k_scan runs at most one
// workgroup per compute unit, so the bound cannot fire on any device; it is part of the one predicate (`folds`) all the same.
enum { SB_FOLD_MAX_PARTS = 1024, SB_PLAN_MAX_STEPS = 7 };

// what sb_strip_shape, sb_strip32_shape and sb_thc_tile_shape answer for the domain (sb_contrast_shapes, sb_launch.hpp)
struct SbShapes {
    bool strip_fits, strip32_fits;  // the strip kernels' position planes hold the block grid
    int strip_ntx, strip_nty, strip32_ntx, strip32_nty;
    int tile_w, tile_rows24, tile_rows32;   // the tile kernel's tiles for LDS halos of 24 and 32 cells
};

struct SbPlanIn {
    int phases;                     // bit 0: k_scan, k_prep, k_wind (no ghost cells, no statistics of other bands needed);
                                    // bit 1: the statistics of all bands, k_t0, the contrast.  3: the whole call
    int esize, nx, rows, halo;      // sizeof(T); interior cells; the LDS halo (sb_pick_halo)
    bool t0_fly;                    // host-model flavour: the contrast kernel derives t0 (f2py flavour: k_t0 writes the plane)
    bool no_wide_strip, no_fold, no_plan_cache, band_late_wind;     // sb_set_wide_strip / _fold / _plan_cache / _band_order
    bool gathered;                  // sigma moments of every band are set (sb_use_gathered_moments, a band step)
    bool moments_out;               // phase 1 of a band step: this band's moments are published for the all-gather
    bool reuse_stats;               // static sigma: the sigmoid scalars of an earlier call stand
    bool plan_use, segs_built;      // the strip kernel's stored plan was made for this geometry; the last complete call's
                                    // strip kernel compacted k_wind's segment lists
    int scan_wgs;                   // k_scan's workgroups (sb_scan_workgroups, sb_launch.hpp)
    SbShapes shapes;
    bool table;                     // sb_set_table_contrast is on and the call is one it serves as far as the caller can tell: host-model
                                    // flavour, SB_BND_GLOBAL or SB_BND_HALO, Geo::band == 0 (whole call, no gathered moments: checked here)
    bool band_table;                // sb_set_table_contrast_bands is on beside it and the call is one that switch serves as far as the caller
                                    // can tell: host-model flavour, SB_BND_HALO, Geo::band == 0 (a band phase or gathered moments: checked here)
    bool f2py_table;                // sb_set_table_contrast_f2py is on beside sb_set_table_contrast and the call is of the f2py flavour
                                    // with SB_BND_WRAPPER; the caller sets `table` with it (whole call, no gathered moments: checked here)
    bool guard;                     // sb_set_nonfinite_guard is on and the frame is one the guard serves as far as the caller can tell
                                    // (Geo::band == 0); sb_plan_diag does not read it: the guard has a plan of its own, sb_plan_guard
    bool guard_bands;               // sb_set_nonfinite_guard_bands is on beside it: band phases and calls with gathered moments of the
                                    // host-model flavour too (checked in sb_plan_guard; sb_plan_diag does not read it either)
};

// the contrast kernel of the call and its block / tile grid
struct SbContrast {
    int strip;                      // 0: LDS tiles (k_thc3); 1: marching strips (k_strip); 2: the 96-column strips (k_strip32)
    int Hk;                         // LDS halo of the kernel that runs
    int txw, tyrows, tx, ty;        // owned columns and rows of a block / tile; blocks / tiles along x and y
    int vb;                         // virtual blocks above and below every strip in the flags (0: tiles, row-major flags)
    int ntile, nflag;               // flags of the blocks / tiles; the same plus the two slow-path counters
};

struct SbStep {
    signed char kernel, prof, stats;    // SbKernel; the SB_PROF_* pair that brackets it in a profiled call; SbStatsSrc
    int nparts;                     // k_prep, contrast with PARTIALS: partial moments to merge
    bool publish;                   // k_scan leaves this band's moments for the all-gather; the moments event is recorded behind it
    bool fold;                      // the strip kernel does k_prep's work: ranks the flags, publishes the scalars, compacts the lists
    bool wind_final;                // DiagJob::wind_final as this kernel sees it
    bool strip_update;              // the strip kernel applies thresholds and state update behind its march
    bool lists_stand;               // DiagJob::lists_stand: a march by the stored plan does not compact the segment lists again
    bool seg_trust;                 // k_wind reads the lists of the call before (no k_prep in this call)
    bool table;                     // the contrast is the query of the device-wide tables (k_table_query), not a strip / tile kernel
};

struct SbDiagPlan {
    SbContrast contrast;
    int scan_wgs, nsteps;
    SbStep steps[SB_PLAN_MAX_STEPS];
    bool wind_scratch;              // k_wind runs ahead of the contrast and leaves its winds in the nws / nwd planes
    bool segs_built;                // after a complete call: the contrast step carried `fold`
    bool table;                     // the call builds and queries the device-wide tables: run_diag sizes their workspace
};

// Marching strips (32 owned longitudes x 16-row blocks, flags strip-major with virtual blocks above and below every strip)
// for LDS halos up to 16 cells; beyond, in single precision, the 96-column strip kernel answers radii up to 31 from LDS
// -- what a distance field made with a window of up to 30 cells needs; double precision, sb_set_wide_strip(ctx, 0) and
// grids the strip kernels' position planes cannot hold take LDS tiles (halos of 24 and 32 cells, row-major flags).
inline SbContrast sb_plan_contrast(const SbPlanIn &in) {
    const SbShapes &s = in.shapes;
    SbContrast k{};
    if (in.halo > 16 && in.esize == 4 && !in.no_wide_strip && s.strip32_fits) k.strip = 2;
    else if (in.halo <= 16 && s.strip_fits) k.strip = 1;
    if (k.strip) {
        k.Hk = 16 * k.strip; k.vb = k.strip; k.txw = 32; k.tyrows = 16;
        k.tx = k.strip == 2 ? s.strip32_ntx : s.strip_ntx;
        k.ty = k.strip == 2 ? s.strip32_nty : s.strip_nty;
        k.ntile = k.tx * (k.ty + 2 * k.vb);
    } else {
        k.Hk = in.halo > 16 ? in.halo : 24;
        k.txw = s.tile_w; k.tyrows = k.Hk <= 24 ? s.tile_rows24 : s.tile_rows32;
        k.tx = (in.nx + k.txw - 1) / k.txw; k.ty = (in.rows + k.tyrows - 1) / k.tyrows;
        k.ntile = k.tx * k.ty;
    }
    k.nflag = k.ntile + 2;
    return k;
}

inline SbDiagPlan sb_plan_diag(const SbPlanIn &in) {
    SbDiagPlan p{};
    p.contrast = sb_plan_contrast(in);
    p.scan_wgs = in.scan_wgs;
    const bool strip = p.contrast.strip != 0, reuse = in.reuse_stats, ph1 = (in.phases & 1) != 0, ph2 = (in.phases & 2) != 0;
    // the strip kernel does k_prep's work itself (host-model flavour: one dependent launch less on the critical path)
    const bool folds = strip && in.t0_fly && !in.no_fold && in.scan_wgs <= SB_FOLD_MAX_PARTS;
    // the segment lists the strip kernel of the call before compacted belong to the planes its stored plan belongs to
    const bool stand = folds && in.plan_use && in.segs_built && !in.no_plan_cache;
    // Whole single-domain calls run the contrast first and let k_wind apply the update.  A band step runs k_scan and
    // k_wind ahead of the join with the communication stream and applies the update in the contrast kernel; its
    // single-domain order (sb_set_band_order) was measured and is slower.
    const bool whole = in.phases == 3 && !in.gathered;
    // Opt-in (sb_set_table_contrast): the contrast of every band cell from device-wide summed-area tables, whatever its
    // radius -- whole single-domain host-model calls; with sb_set_table_contrast_bands beside it, band steps and calls with
    // gathered moments of that flavour too (`table` alone never changes those)
    const bool band_table = in.band_table && in.table && !whole && in.t0_fly;
    // ... and with sb_set_table_contrast_f2py beside it, whole calls of the f2py flavour: the row pass forms t0 and writes
    // the plane that flavour returns, so the six launches of the host-model table call stand where five ran, without k_t0
    const bool f2py_table = in.f2py_table && in.table && whole && !in.t0_fly;
    p.table = (in.table && whole && in.t0_fly) || band_table || f2py_table;
    const bool late_wind = in.band_late_wind && in.gathered && folds && !band_table;    // (sb_set_band_order: not for the tables)
    p.wind_scratch = !(whole || late_wind);
    SbStep *contrast = nullptr;
    auto add = [&p](SbKernel k, int prof, bool stats = false, int nparts = 0) -> SbStep & {
        SbStep &s = p.steps[p.nsteps++];
        s.kernel = (signed char)k; s.prof = (signed char)prof; s.wind_final = !p.wind_scratch;
        s.stats = stats ? SB_STATS_PARTIALS : SB_STATS_NONE; s.nparts = nparts;
        return s;
    };
    // A whole table call: k_prep merges the moments, publishes the scalars the row pass forms t0 with and compacts the
    // segment lists the query takes its band cells from.  A profiled call times the row pass in k_t0's pair (the host-model
    // flavour has no k_t0), the column pass and the query together in the contrast's.
    if (band_table) {
        // A band step / a call with gathered moments on the tables.  Ahead of the join, as without them: k_scan (publishes
        // the band's moments), k_prep (every call: no stored plan is trusted), k_wind to the scratch planes.  Behind it:
        // k_merge_moments leaves the scalars the row pass reads (dropped when they stand), the two passes over the whole
        // ghost-celled frame, and the query, which applies thresholds and state update itself.
        if (ph1) {
            const bool own = (!in.gathered || in.moments_out) && !reuse, publishes = own && in.gathered;
            add(SB_K_SCAN, SB_PROF_SCAN, own).publish = publishes;
            add(SB_K_PREP, SB_PROF_PREP, own && !publishes, own && !publishes ? in.scan_wgs : 0);
            add(SB_K_WIND, SB_PROF_WIND);
        }
        if (ph2) {
            if (in.gathered && !reuse) add(SB_K_MERGE, SB_PROF_NONE).stats = SB_STATS_GATHERED;
            add(SB_K_TABLE_ROWS, SB_PROF_T0);
            add(SB_K_TABLE_COLS, SB_PROF_THC);
            contrast = &add(SB_K_CONTRAST, SB_PROF_THC);
            contrast->table = true;
        }
    } else if (p.table) {
        add(SB_K_SCAN, SB_PROF_SCAN, !reuse);
        add(SB_K_PREP, SB_PROF_PREP, !reuse, reuse ? 0 : in.scan_wgs);
        add(SB_K_TABLE_ROWS, SB_PROF_T0);
        add(SB_K_TABLE_COLS, SB_PROF_THC);
        contrast = &add(SB_K_CONTRAST, SB_PROF_THC);
        contrast->table = true;
        add(SB_K_WIND, SB_PROF_WIND);
    } else if (whole) {
        const int nparts = reuse ? 0 : in.scan_wgs;
        add(SB_K_SCAN, SB_PROF_SCAN, !reuse);
        if (!folds) add(SB_K_PREP, SB_PROF_PREP, !reuse, nparts);
        if (!in.t0_fly) add(SB_K_T0, SB_PROF_T0);
        contrast = &add(SB_K_CONTRAST, SB_PROF_THC, folds, folds ? nparts : 0);
        contrast->fold = folds;
        add(SB_K_WIND, SB_PROF_WIND);
        for (int i = 0; i < p.nsteps; ++i) p.steps[i].lists_stand = stand;
    } else if (late_wind) {
        // a band step in the single-domain order: k_scan ahead of the join; behind it the strip kernel -- it merges the
        // gathered moments and compacts k_wind's segment lists itself -- and k_wind with the update.  (Never profiled.)
        const bool publishes = in.moments_out && !reuse;
        if (ph1) add(SB_K_SCAN, SB_PROF_NONE, publishes).publish = publishes;
        if (ph2) {
            contrast = &add(SB_K_CONTRAST, SB_PROF_NONE);
            contrast->fold = true;
            if (!reuse) contrast->stats = SB_STATS_GATHERED;
            add(SB_K_WIND, SB_PROF_NONE);
        }
    } else {
        if (ph1) {
            // a band step: k_scan's last workgroup merges and publishes this band's moments (the all-gather starts behind it)
            const bool own = (!in.gathered || in.moments_out) && !reuse, publishes = own && in.gathered;
            const bool trust = stand && in.gathered;
            add(SB_K_SCAN, SB_PROF_SCAN, own).publish = publishes;
            if (!trust) add(SB_K_PREP, SB_PROF_PREP, own && !publishes, own && !publishes ? in.scan_wgs : 0);
            add(SB_K_WIND, SB_PROF_WIND).seg_trust = trust;
        }
        if (ph2) {
            const bool merge = in.gathered && !reuse;
            // k_t0 needs the scalars first; the contrast kernel that derives t0 merges the gathered moments in its prologue
            if (merge && !in.t0_fly) add(SB_K_MERGE, SB_PROF_NONE).stats = SB_STATS_GATHERED;
            if (!in.t0_fly) add(SB_K_T0, SB_PROF_T0);
            contrast = &add(SB_K_CONTRAST, SB_PROF_THC);
            if (merge && in.t0_fly) contrast->stats = SB_STATS_GATHERED;
            // the strip kernel applies thresholds and state update behind its march whatever the order (it leaves the
            // contrast in thc) and compacts the segment lists: this call's update reads them, and the next call's k_wind
            // if the planes stand (no k_prep then)
            if (strip) { contrast->wind_final = contrast->strip_update = true; contrast->fold = folds; }
        }
    }
    p.segs_built = contrast && contrast->fold;
    return p;
}

// ---- the opt-in guard for missing and non-finite temperatures (sb_set_nonfinite_guard; sb_guard_kernels.hip).  Purely
// additive: the main plan above is the same with the switch on and off, and the guard's launches go between its steps.
//   k_guard_bits    ahead of step `bits_before` (the first): the bad-bit plane of the frame and the number of bad cells
//   k_guard_taint   behind step `after` (the CONTRAST step), two launches: the bad plane dilated along longitude, then along
//                   latitude, by the reach of the contrast kernel that ran -- or, for the tile kernel, whose floating-point
//                   prefix sums let one bad cell poison a whole tile, by the staged rectangle of every tile ("by tile")
//   k_guard_repair  behind it and ahead of the final WIND: the tainted band cells again, the way the reference sums them
// Whole calls in which CONTRAST runs ahead of a final WIND.  Where the contrast kernel applies the update itself (phase 2 of
// a band step, a one-sequence call with gathered moments) thc is consumed, and ws / wd -- the state of the step before,
// which the trigger rule needs -- are overwritten, before a repair could run: the guard is ignored there unless
// sb_set_nonfinite_guard_bands is on beside it (`guard_bands`; host-model flavour only).  The taint follows from theta, z,
// the band plane and the reach alone, so then
//   k_guard_bits and both taint passes go directly AHEAD of the CONTRAST step (`taint_before`), the latitude pass puts ws / wd
//                   of every tainted band cell aside in two stash planes;
//   k_guard_repair  directly behind it computes those cells again and applies the update again from the stash (`update`).
// A call with gathered moments in the single-domain order (sb_set_band_order: CONTRAST, then a final WIND) runs as a whole
// call does.  A phase-1 plan gets nothing.
enum { SB_GUARD_BY_TILE = -1, SB_GUARD_REACH_STRIP = 16, SB_GUARD_REACH_STRIP32 = 31, SB_GUARD_REACH_TABLE = 127, SB_GUARD_LAUNCHES = 4 };
struct SbGuardPlan {
    bool on;                        // the guard runs in this call
    int reach;                      // cells a bad cell taints round itself, or SB_GUARD_BY_TILE
    int tile_w, tile_rows, halo;    // by tile: the tiles' owned columns and rows and their LDS halo (SbContrast)
    int bits_before, after;         // steps of the main plan: k_guard_bits goes ahead of the one, taint and repair behind the other
    int nlaunch;                    // launches the guard adds (sb_last_step_report[0] counts them)
    int taint_before;               // the two taint passes go ahead of this step and stash ws / wd; -1: behind `after`, no stash
    bool update;                    // the repair applies thresholds and state update from the stash (the CONTRAST step applied them)
};
inline SbGuardPlan sb_plan_guard(const SbPlanIn &in, const SbDiagPlan &p) {
    SbGuardPlan gp{};
    gp.bits_before = gp.after = gp.taint_before = -1;
    if (!in.guard || !(in.phases & 2) || p.nsteps < 1) return gp;
    const bool whole = in.phases == 3 && !in.gathered;
    if (!whole && !(in.guard_bands && in.t0_fly)) return gp;
    int ci = p.nsteps - 1;
    if (p.steps[ci].kernel == SB_K_WIND) --ci;
    if (ci < 0 || p.steps[ci].kernel != SB_K_CONTRAST) return gp;
    const SbStep &c = p.steps[ci];
    const bool wind_behind = ci + 1 < p.nsteps;
    if (wind_behind) {
        // CONTRAST ahead of a final WIND: a whole call, or gathered moments in the single-domain order (phase 2 of a band
        // step in that order: CONTRAST is its step 0)
        if (c.strip_update || !p.steps[ci + 1].wind_final || p.wind_scratch) return gp;
        gp.bits_before = 0;
    } else {
        // the CONTRAST step applies the update
        if (whole || !(c.strip_update || p.wind_scratch)) return gp;
        gp.bits_before = gp.taint_before = ci; gp.update = true;
    }
    gp.on = true;
    gp.after = ci; gp.nlaunch = SB_GUARD_LAUNCHES;
    if (c.table) gp.reach = SB_GUARD_REACH_TABLE;
    else if (p.contrast.strip == 1) gp.reach = SB_GUARD_REACH_STRIP;
    else if (p.contrast.strip == 2) gp.reach = SB_GUARD_REACH_STRIP32;
    else { gp.reach = SB_GUARD_BY_TILE; gp.tile_w = p.contrast.txw; gp.tile_rows = p.contrast.tyrows; gp.halo = p.contrast.Hk; }
    return gp;
}

// ---- the opt-in switches of a context (sb_set_table_contrast, _bands, _f2py, sb_set_table_window_cache, sb_set_nonfinite_guard,
// _bands) and the calls each of them serves.  Every predicate over a switch and a call stands here once; sb_plan_diag and
// sb_plan_guard above check the halves that they can see (`whole`, `t0_fly`) for themselves, so they are valid for any input.
struct SbSwitches { bool table, table_bands, table_f2py, table_cache, guard, guard_bands; };
// what run_diag knows of a call before it plans
enum SbCallBnd { SB_CALL_BND_WRAPPER = 0, SB_CALL_BND_GLOBAL = 1, SB_CALL_BND_HALO = 2 };    // BND_* (sb_device.hpp)
struct SbCall {
    bool host_model;                // the host-model flavour (seabreeze_diag*, band steps); false: the f2py flavour (sb_diag_*, stream steps)
    int bnd;                        // the boundary rule, SbCallBnd
    bool ghost;                     // the ghost width is not 0
    bool band_geo;                  // Geo::band is not 0: a band step whose strip kernel takes ghost cells of theta from its interior
};
// the two pairs of switches that a band step's frame depends on  (static, here and below: the library's exported symbols stay as they are)
static inline bool sb_band_tables_on(const SbSwitches &s) { return s.table && s.table_bands; }
static inline bool sb_band_guard_on(const SbSwitches &s) { return s.guard && s.guard_bands; }

// Fills the switches' fields of `in` (table, band_table, f2py_table, guard, guard_bands; phases and gathered are set already)
// and answers whether the call is a table call that keeps its windows (sb_set_table_window_cache): as sb_plan_diag decides
// `table` for a whole call, and the switch.  Its k_scan watches the planes whatever the contrast kernel of the domain would
// be: where that is the tile kernel, run_diag allocates the header of the strip kernel's plan alone.
static inline bool sb_apply_switches(const SbSwitches &s, const SbCall &c, SbPlanIn &in) {
    const bool whole = in.phases == 3 && !in.gathered;
    // the tables and the guard's kernels see plain geometry: every ghost cell of the frame as filled
    const bool host_frame = c.host_model && (c.bnd == SB_CALL_BND_GLOBAL || c.bnd == SB_CALL_BND_HALO) && !c.band_geo;
    // the f2py flavour on the tables: a switch of its own beside sb_set_table_contrast, the wrapper's boundary rule alone
    in.f2py_table = s.table && s.table_f2py && !c.host_model && c.bnd == SB_CALL_BND_WRAPPER && !c.ghost;
    in.table = (s.table && host_frame) || in.f2py_table;
    // ... and the tables for a band phase or a call with gathered moments: a switch of its own beside that one, ghost cells only
    in.band_table = sb_band_tables_on(s) && host_frame && c.bnd == SB_CALL_BND_HALO && !whole;
    // the guard for missing and non-finite temperatures: a plan of its own (sb_plan_guard), whatever the flavour
    in.guard = s.guard && !c.band_geo;
    in.guard_bands = sb_band_guard_on(s) && !c.band_geo;
    return s.table_cache && in.table && whole;
}

// A band step (band_diag_dev) on a strip kernel sends only the ghost rows of theta that come from a neighbour; the east-west
// ghost columns and the rows beyond a pole follow from theta's interior, and the strip kernels take them from there by index
// (Geo::band != 0) -- which needs a circle of latitude wider than any row they stage (sb_strip_common.hpp: one wrap of the index
// then suffices).  Never where the band tables or the band guard may be served: they read the whole frame as filled, so theta
// gets the whole swap_bounds and Geo::band stays 0, which is what sb_apply_switches asks of the two phases that follow.
// `k`: sb_plan_contrast of the band.
enum { SB_BAND_FOLD_NX_ABOVE = 96 + 2 };
static inline bool sb_band_folds_frame(const SbSwitches &s, const SbContrast &k, int nx) {
    return !sb_band_tables_on(s) && !sb_band_guard_on(s) && k.strip != 0 && nx > SB_BAND_FOLD_NX_ABOVE;
}
