// band_table_plan_dump.cpp -- tests/table_plan_dump.cpp with one more input: prints the launch plan (seabreeze_param_amd/csrc/
// sb_diag_plan.hpp) of the cases it reads from standard input, one per line, for tests/test_band_table_plan.py.  Host only.
//
// A case is a label and 17 integers: the 16 of table_plan_dump.cpp, in its order, then `band_table` (sb_set_table_contrast
// and sb_set_table_contrast_bands are both on and the call is of the host-model flavour with SB_BND_HALO and
// Geo::band == 0: a band phase or a call with gathered moments, as far as the caller can tell).  The domain and the output
// format are those of table_plan_dump.cpp.
#include <cstdio>
#include "../seabreeze_param_amd/csrc/sb_diag_plan.hpp"

int main() {
    static const char *const kname[] = {"SCAN", "PREP", "MERGE", "T0", "CONTRAST", "WIND", "TABLE_ROWS", "TABLE_COLS"};
    static const char *const pname[] = {"scan", "wind", "t0", "thc", "prep"};
    static const char *const sname[] = {"none", "partials", "gathered"};
    char label[128];
    int v[17];
    for (;;) {
        if (std::scanf("%127s", label) != 1) return 0;
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
        std::printf(" | segs_built=%d wind_scratch=%d scan_wgs=%d table=%d\n", (int)p.segs_built, (int)p.wind_scratch, p.scan_wgs, (int)p.table);
    }
}
