// band_guard_plan_dump.cpp -- tests/guard_plan_dump.cpp with a 20th input, `guard_bands` (sb_set_nonfinite_guard_bands is on
// beside sb_set_nonfinite_guard), and the guard plan's two further fields: reads one command per line from standard input,
// for tests/test_band_guard_plan.py.  Host only.
//
//   plan label <20 integers>     the 19 of guard_plan_dump.cpp, in its order, then `guard_bands`.  Prints the main plan in the
//                                format of f2py_table_plan_dump.cpp, then " | guard=0 nlaunch=0" or
//                                " | guard=1 reach=R|tile:WxH+halo bits_before=I after=J nlaunch=N" as guard_plan_dump.cpp does,
//                                then " | taint_before=K update=U".
// The domain of a plan is that of table_plan_dump.cpp.
#include <cstdio>
#include <cstring>
#include "../seabreeze_param_amd/csrc/sb_diag_plan.hpp"

int main() {
    static const char *const kname[] = {"SCAN", "PREP", "MERGE", "T0", "CONTRAST", "WIND", "TABLE_ROWS", "TABLE_COLS"};
    static const char *const pname[] = {"scan", "wind", "t0", "thc", "prep"};
    static const char *const sname[] = {"none", "partials", "gathered"};
    char cmd[32], label[128];
    while (std::scanf("%31s", cmd) == 1) {
        if (std::strcmp(cmd, "plan") || std::scanf("%127s", label) != 1) return 1;
        int v[20];
        for (int &x : v)
            if (std::scanf("%d", &x) != 1) return 1;
        SbPlanIn in{};
        in.phases = v[0]; in.esize = v[1]; in.t0_fly = v[2] != 0; in.halo = sb_pick_halo(v[3]);
        in.no_wide_strip = v[4] != 0; in.no_fold = v[5] != 0; in.no_plan_cache = v[6] != 0; in.band_late_wind = v[7] != 0;
        in.gathered = v[8] != 0; in.moments_out = v[9] != 0; in.reuse_stats = v[10] != 0;
        in.plan_use = v[11] != 0; in.segs_built = v[12] != 0; in.scan_wgs = v[13];
        in.nx = 200; in.rows = 96;
        in.shapes = SbShapes{v[14] != 0, v[14] != 0, 7, 6, 7, 6, 32, 32, 16};
        in.table = v[15] != 0;
        in.band_table = v[16] != 0;
        in.f2py_table = v[17] != 0;
        in.guard = v[18] != 0;
        in.guard_bands = v[19] != 0;
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
    return 0;
}
