// f2py_table_plan_dump.cpp -- tests/band_table_plan_dump.cpp with one more input, and the host's half of the window cache
// beside it: reads one command per line from standard input, for tests/test_f2py_table_plan.py.  Host only.
//
//   plan label <18 integers>                 the 17 of band_table_plan_dump.cpp, in its order, then `f2py_table`
//                                            (sb_set_table_contrast and sb_set_table_contrast_f2py are both on and the call
//                                            is of the f2py flavour with SB_BND_WRAPPER).  Prints the plan in the format of
//                                            table_plan_dump.cpp, with " nsteps=N max=SB_PLAN_MAX_STEPS" appended.
//   call nx ny h bnd rows band cls W C seq   a call with the cache in effect is about to be enqueued: prints why the host
//                                            forces a fill (or "steady"), then notes the call as enqueued whole
//   other                                    another diag call or band step ran k_scan (tests/table_cache_dump.cpp)
// The domain of a plan is that of table_plan_dump.cpp; the addresses of a call are small integers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../seabreeze_param_amd/csrc/sb_diag_plan.hpp"
#include "../seabreeze_param_amd/csrc/sb_table_cache.hpp"

int main() {
    static const char *const kname[] = {"SCAN", "PREP", "MERGE", "T0", "CONTRAST", "WIND", "TABLE_ROWS", "TABLE_COLS"};
    static const char *const pname[] = {"scan", "wind", "t0", "thc", "prep"};
    static const char *const sname[] = {"none", "partials", "gathered"};
    static const char *const why[] = {"steady", "no_key", "key_differs", "seq_restart", "toggled", "failed", "other_call"};
    SbTabCache cache;
    char cmd[32], label[128];
    while (std::scanf("%31s", cmd) == 1) {
        if (!std::strcmp(cmd, "other")) { sb_tab_cache_other_call(cache); continue; }
        if (!std::strcmp(cmd, "call")) {
            long long v[10];
            for (long long &x : v)
                if (std::scanf("%lld", &x) != 1) return 1;
            const SbTabKey key{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (const void *)(uintptr_t)v[5],
                               (const void *)(uintptr_t)v[6], (const void *)(uintptr_t)v[7], (const void *)(uintptr_t)v[8]};
            std::printf("%s\n", why[(int)sb_tab_cache_decide(cache, key, (int)v[9])]);
            sb_tab_cache_filled(cache, key, (int)v[9]);
            continue;
        }
        if (std::strcmp(cmd, "plan") || std::scanf("%127s", label) != 1) return 1;
        int v[18];
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
        const SbDiagPlan p = sb_plan_diag(in);
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
        std::printf(" | segs_built=%d wind_scratch=%d scan_wgs=%d table=%d nsteps=%d max=%d\n", (int)p.segs_built, (int)p.wind_scratch,
                    p.scan_wgs, (int)p.table, p.nsteps, (int)SB_PLAN_MAX_STEPS);
    }
    return 0;
}
