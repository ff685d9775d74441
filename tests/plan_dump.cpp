// plan_dump.cpp -- prints what seabreeze_param_amd/csrc/sb_diag_plan.hpp decides, and drives the host's half of the window
// cache (sb_table_cache.hpp), one command per line of standard input, for tests/plan_dump.py and the tests that import it.
// Host only: the headers need neither HIP nor a device.
//
//   plan label [name=value ...]      the launch plan (sb_plan_diag) and the guard's (sb_plan_guard) of one SbPlanIn:
//                                    label | the contrast kernel | the steps | what the host keeps | the guard | its band fields
//   switches label [name=value ...]  what sb_apply_switches makes of the switches sw_* and the call host_model, bnd, ghost,
//                                    band_geo (with phases, gathered and the rest of the plan's inputs): the five fields it
//                                    fills, its answer about the window cache, sb_band_folds_frame of the same switches and
//                                    domain, and whether the plans of the filled input take the tables and run the guard
//   call nx ny h bnd rows band cls W C seq   a call with the cache in effect is about to be enqueued: prints why the host
//                                    forces a fill (or "steady"), then notes the call as enqueued whole
//   other | failed | toggled         another diag call or band step ran k_scan; a launch failed; the switch was set
//   word found radius nl             prints the word of plane W for a cell and what the query reads back from it:
//                                    "word radius nl"
// An input that is not named takes the default that get() states below; a name nobody asks for is an error.  The domain
// is nx x 96 interior cells, nx = 200 unless given: both strip kernels' block grids are 7 x 6 (32 owned columns x 16 rows)
// and fit their position planes unless `fits` is 0; the tile kernel's tiles are 32 x 32 (halo 24) and 32 x 16 (halo 32).
// The addresses of a `call` are small integers: the key compares them, nothing reads through them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../seabreeze_param_amd/csrc/sb_diag_plan.hpp"
#include "../seabreeze_param_amd/csrc/sb_table_cache.hpp"

namespace {

// the name=value pairs of one command
struct Args {
    enum { MAX = 48 };
    const char *name[MAX];
    int value[MAX], n = 0;
    bool used[MAX];
    bool parse(char *rest) {
        for (char *t = std::strtok(rest, " \t\n"); t; t = std::strtok(nullptr, " \t\n")) {
            char *eq = std::strchr(t, '=');
            if (!eq || n == MAX) return false;
            *eq = 0;
            name[n] = t; value[n] = std::atoi(eq + 1); used[n++] = false;
        }
        return true;
    }
    int get(const char *key, int dflt) {
        for (int i = 0; i < n; ++i)
            if (!std::strcmp(name[i], key)) { used[i] = true; dflt = value[i]; }
        return dflt;
    }
    bool all_used() const {
        for (int i = 0; i < n; ++i)
            if (!used[i]) return false;
        return true;
    }
};

// a new planner input costs one line here
SbPlanIn plan_in(Args &a) {
    SbPlanIn in{};
    in.phases = a.get("phases", 3); in.esize = a.get("esize", 8); in.t0_fly = a.get("t0_fly", 1) != 0;
    in.halo = sb_pick_halo(a.get("hint", 6));
    in.no_wide_strip = a.get("no_wide", 0) != 0; in.no_fold = a.get("no_fold", 0) != 0; in.no_plan_cache = a.get("no_cache", 0) != 0;
    in.band_late_wind = a.get("late", 0) != 0;
    in.gathered = a.get("gathered", 0) != 0; in.moments_out = a.get("mout", 0) != 0; in.reuse_stats = a.get("reuse", 0) != 0;
    in.plan_use = a.get("plan_use", 0) != 0; in.segs_built = a.get("segs_built", 0) != 0; in.scan_wgs = a.get("wgs", 12);
    in.nx = a.get("nx", 200); in.rows = 96;
    const bool fits = a.get("fits", 1) != 0;
    in.shapes = SbShapes{fits, fits, 7, 6, 7, 6, 32, 32, 16};
    in.table = a.get("table", 0) != 0;
    in.band_table = a.get("band_table", 0) != 0;
    in.f2py_table = a.get("f2py_table", 0) != 0;
    in.guard = a.get("guard", 0) != 0;
    in.guard_bands = a.get("guard_bands", 0) != 0;
    return in;
}

void print_plan(const char *label, const SbPlanIn &in) {
    static const char *const kname[] = {"SCAN", "PREP", "MERGE", "T0", "CONTRAST", "WIND", "TABLE_ROWS", "TABLE_COLS"};
    static const char *const pname[] = {"scan", "wind", "t0", "thc", "prep"};
    static const char *const sname[] = {"none", "partials", "gathered"};
    const SbDiagPlan p = sb_plan_diag(in);
    const SbGuardPlan g = sb_plan_guard(in, p);
    const SbContrast &k = p.contrast;
    std::printf("%s | strip=%d Hk=%d tile=%dx%d grid=%dx%d vb=%d nflag=%d |", label, k.strip, k.Hk, k.txw, k.tyrows, k.tx, k.ty,
                k.vb, k.nflag);
    for (int i = 0; i < p.nsteps; ++i) {
        const SbStep &s = p.steps[i];
        std::printf(" %s:prof=%s,stats=%s*%d", kname[(int)s.kernel], s.prof == SB_PROF_NONE ? "none" : pname[(int)s.prof],
                    sname[(int)s.stats], s.nparts);
        if (s.publish) std::printf(",publish");
        if (s.fold) std::printf(",fold");
        if (s.wind_final) std::printf(",final");
        if (s.strip_update) std::printf(",update");
        if (s.lists_stand) std::printf(",stand");
        if (s.seg_trust) std::printf(",trust");
        if (s.table) std::printf(",table");
    }
    std::printf(" | segs_built=%d wind_scratch=%d scan_wgs=%d table=%d nsteps=%d max=%d", (int)p.segs_built, (int)p.wind_scratch,
                p.scan_wgs, (int)p.table, p.nsteps, (int)SB_PLAN_MAX_STEPS);
    if (!g.on) std::printf(" | guard=0 nlaunch=%d", g.nlaunch);
    else {
        std::printf(" | guard=1 reach=");
        if (g.reach == SB_GUARD_BY_TILE) std::printf("tile:%dx%d+%d", g.tile_w, g.tile_rows, g.halo);
        else std::printf("%d", g.reach);
        std::printf(" bits_before=%d after=%d nlaunch=%d", g.bits_before, g.after, g.nlaunch);
    }
    std::printf(" | taint_before=%d update=%d\n", g.taint_before, (int)g.update);
}

void print_switches(const char *label, const SbSwitches &s, const SbCall &c, SbPlanIn in) {
    const bool cache = sb_apply_switches(s, c, in);
    const SbDiagPlan p = sb_plan_diag(in);
    std::printf("%s | table=%d band_table=%d f2py_table=%d guard=%d guard_bands=%d | cache=%d | folds=%d | plan_table=%d guard_on=%d\n",
                label, (int)in.table, (int)in.band_table, (int)in.f2py_table, (int)in.guard, (int)in.guard_bands, (int)cache,
                (int)sb_band_folds_frame(s, sb_plan_contrast(in), in.nx), (int)p.table, (int)sb_plan_guard(in, p).on);
}

}  // namespace

int main() {
    static const char *const why[] = {"steady", "no_key", "key_differs", "seq_restart", "toggled", "failed", "other_call"};
    static char line[4096];
    SbTabCache cache;
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[32], label[128];
        int at = 0;
        if (std::sscanf(line, "%31s%n", cmd, &at) != 1) continue;       // (an empty line)
        char *rest = line + at;
        if (!std::strcmp(cmd, "plan") || !std::strcmp(cmd, "switches")) {
            Args a;
            if (std::sscanf(rest, "%127s%n", label, &at) != 1 || !a.parse(rest + at)) return 1;
            const SbPlanIn in = plan_in(a);
            if (cmd[0] == 'p') {
                if (!a.all_used()) return 1;                            // (a name nobody asked for: the switches' and the call's too)
                print_plan(label, in);
                continue;
            }
            const SbSwitches s{a.get("sw_table", 0) != 0, a.get("sw_table_bands", 0) != 0, a.get("sw_table_f2py", 0) != 0,
                               a.get("sw_table_cache", 0) != 0, a.get("sw_guard", 0) != 0, a.get("sw_guard_bands", 0) != 0};
            const SbCall c{a.get("host_model", 1) != 0, a.get("bnd", SB_CALL_BND_GLOBAL), a.get("ghost", 0) != 0, a.get("band_geo", 0) != 0};
            if (!a.all_used()) return 1;
            print_switches(label, s, c, in);
        } else if (!std::strcmp(cmd, "call")) {
            long long v[10];
            if (std::sscanf(rest, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7,
                            v + 8, v + 9) != 10) return 1;
            const SbTabKey key{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (const void *)(uintptr_t)v[5],
                               (const void *)(uintptr_t)v[6], (const void *)(uintptr_t)v[7], (const void *)(uintptr_t)v[8]};
            std::printf("%s\n", why[(int)sb_tab_cache_decide(cache, key, (int)v[9])]);
            sb_tab_cache_filled(cache, key, (int)v[9]);
        } else if (!std::strcmp(cmd, "other")) sb_tab_cache_other_call(cache);
        else if (!std::strcmp(cmd, "failed")) sb_tab_cache_launch_failed(cache);
        else if (!std::strcmp(cmd, "toggled")) sb_tab_cache_toggled(cache);
        else if (!std::strcmp(cmd, "word")) {
            int found, r, nl;
            if (std::sscanf(rest, "%d %d %d", &found, &r, &nl) != 3) return 1;
            const unsigned w = found ? sb_tab_pack(r, nl) : 0u;
            std::printf("%u %d %d\n", w, sb_tab_radius(w), sb_tab_nl(w));
        } else return 1;
    }
    return 0;
}
