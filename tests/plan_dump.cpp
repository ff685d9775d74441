// plan_dump.cpp -- prints what seabreeze_param_amd/csrc/sb_diag_plan.hpp and sb_ice_plan.hpp decide, and drives the host's
// half of the window cache (sb_table_cache.hpp), one command per line of standard input, for tests/plan_dump.py and the
// tests that import it.
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
//   ice | band_ice | um_ice  P | M label ...   what sb_ice_plan.hpp decides for a coast that moves with the sea ice: of a
//                                    stream, of a latitude band, of the UM layout.  P: the path and the planes' sizes; M: the
//                                    mark plane after the words that hold the changed cells (x, row of the bit plane) marked
//                                    their reach, each word once, as k_edge_bits_delta does
//     ice P label nx k incremental                        -> label WHOLE | DELTA
//     ice M label nx ny k n x1 y1 .. xn yn                -> label ntiles, then ny * ntiles marks (0 / 1), row by row
//     band_ice P label nx ny halo south north k incremental -> label NONE | (WHOLE | DELTA) f0 nys r0 r1 nw ntiles
//     band_ice M label nx ny halo south north k n x1 s1 .. xn sn   (s: a SOURCE row)
//                                                         -> label ntiles, then ny * ntiles marks, own row by own row
//     um_ice P label nx ny hi hj wi wj incremental        -> label NONE | (WHOLE | DELTA) nw ngroups ntiles
//     um_ice M label nx ny wi wj n x1 y1 .. xn yn         -> label ngroups ntiles, then ngroups * ntiles marks, group by group
//                                    Exit status 2: a reach outside the mark plane (the kernel would write out of bounds);
//                                    3: a plan whose path is not the path function's.
// An input that is not named takes the default that get() states below; a name nobody asks for is an error.  The domain
// is nx x 96 interior cells, nx = 200 unless given: both strip kernels' block grids are 7 x 6 (32 owned columns x 16 rows)
// and fit their position planes unless `fits` is 0; the tile kernel's tiles are 32 x 32 (halo 24) and 32 x 16 (halo 32).
// The addresses of a `call` are small integers: the key compares them, nothing reads through them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>
#include "../seabreeze_param_amd/csrc/sb_diag_plan.hpp"
#include "../seabreeze_param_amd/csrc/sb_ice_plan.hpp"
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

// ---- sb_ice_plan.hpp ----
static_assert(SB_UM_ICE_ROWS == 4 && SB_UM_ICE_COLS == 64, "the tests' model states the UM tile as 4 x 64");

// the next n integers of a line
bool ints(char *&p, int *v, int n) {
    for (int i = 0; i < n; ++i) {
        char *end;
        v[i] = (int)std::strtol(p, &end, 10);
        if (end == p) return false;
        p = end;
    }
    return true;
}

// The M line of any layout: reads "n x1 y1 .. xn yn" (x < nx, y < rows of the bit plane), marks what reach(x0, y) says
// for each word once and prints the plane `m`.  -> the exit status, 0 to go on
template <typename R>
int print_marks(const char *label, char *p, int nx, int rows, SbIceMarks m, bool with_rows, R reach) {
    int n, xy[2];
    if (!ints(p, &n, 1) || n < 0) return 1;
    std::set<std::pair<int, int>> words;
    for (int i = 0; i < n; ++i) {
        if (!ints(p, xy, 2) || xy[0] < 0 || xy[0] >= nx || xy[1] < 0 || xy[1] >= rows) return 1;
        words.insert({xy[0] & ~63, xy[1]});
    }
    std::vector<unsigned char> marks((size_t)m.rows * m.tiles, 0);
    for (const auto &w : words) {
        const SbIceReach r = reach(w.first, w.second);
        // a mark outside the plane: the kernel would write out of bounds.  The first piece is never empty.
        if (r.r0 < 0 || r.r1 >= m.rows || r.r0 > r.r1 || r.a0 < 0 || r.a1 >= m.tiles || r.a0 > r.a1) return 2;
        if (r.b0 <= r.b1 && (r.b0 < 0 || r.b1 >= m.tiles)) return 2;
        for (int y = r.r0; y <= r.r1; ++y) {
            for (int t = r.a0; t <= r.a1; ++t) marks[(size_t)y * m.tiles + t] = 1;
            for (int t = r.b0; t <= r.b1; ++t) marks[(size_t)y * m.tiles + t] = 1;
        }
    }
    std::printf("%s", label);
    if (with_rows) std::printf(" %d", m.rows);
    std::printf(" %d", m.tiles);
    for (unsigned char b : marks) std::printf(" %d", (int)b);
    std::printf("\n");
    return 0;
}

const char *path_name(SbIcePath p) { return p == SbIcePath::WHOLE ? "WHOLE" : "DELTA"; }

// one `ice`, `band_ice` or `um_ice` line -> the exit status, 0 to go on
int ice_line(const char *cmd, char *rest) {
    char what[8], label[128];
    int at = 0, v[7];
    if (std::sscanf(rest, "%7s %127s%n", what, label, &at) != 2 || (what[0] != 'P' && what[0] != 'M')) return 1;
    char *p = rest + at;
    const bool P = what[0] == 'P';
    if (cmd[0] == 'i') {
        if (P) {
            if (!ints(p, v, 3)) return 1;
            std::printf("%s %s\n", label, path_name(sb_ice_path(v[0], v[1], v[2])));
            return 0;
        }
        if (!ints(p, v, 3) || v[0] < 1 || v[1] < 1) return 1;
        const int nx = v[0], ny = v[1], k = v[2];
        return print_marks(label, p, nx, ny, sb_ice_marks(nx, ny), false, [=](int x0, int y) { return sb_ice_reach(nx, ny, k, x0, y); });
    }
    if (cmd[0] == 'b') {
        if (!ints(p, v, 6) || v[0] < 1 || v[1] < 1) return 1;
        const int nx = v[0], k = v[5];
        int inc = 1;
        if (P && !ints(p, &inc, 1)) return 1;
        const SbBandIcePlan pl = sb_band_ice_plan(nx, v[1], v[2], v[3] != 0, v[4] != 0, k, inc);
        if (P) {
            if (!pl.ok) std::printf("%s NONE\n", label);
            else
                std::printf("%s %s %d %d %d %d %d %d\n", label, path_name(pl.path), pl.rows.f0, pl.rows.nys, pl.rows.r0, pl.rows.r1,
                            pl.nw, pl.marks.tiles);
            return 0;
        }
        if (!pl.ok) return 1;
        const int r0 = pl.rows.r0, r1 = pl.rows.r1;
        return print_marks(label, p, nx, pl.rows.nys, pl.marks, false,
                           [=](int x0, int s) { return sb_band_ice_reach(nx, r0, r1, k, x0, s); });
    }
    if (!ints(p, v, 2)) return 1;
    const int nx = v[0], ny = v[1];
    if (P) {
        if (!ints(p, v, 5)) return 1;
        const SbUmIcePlan pl = sb_um_ice_plan(nx, ny, v[0], v[1], v[2], v[3], v[4]);
        if (!pl.ok) std::printf("%s NONE\n", label);
        else std::printf("%s %s %d %d %d\n", label, path_name(pl.path), pl.nw, pl.marks.rows, pl.marks.tiles);
        return pl.ok && pl.path != sb_um_ice_path(v[4]) ? 3 : 0;
    }
    if (!ints(p, v, 2) || nx < 1 || ny < 1) return 1;
    const int wi = v[0], wj = v[1];
    return print_marks(label, p, nx, ny, sb_um_ice_marks(nx, ny), true, [=](int x0, int y) { return sb_um_ice_reach(nx, ny, wi, wj, x0, y); });
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
        } else if (!std::strcmp(cmd, "ice") || !std::strcmp(cmd, "band_ice") || !std::strcmp(cmd, "um_ice")) {
            if (const int rc = ice_line(cmd, rest)) return rc;
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
