// dist_plan_dump.cpp -- prints what seabreeze_param_amd/csrc/sb_dist_plan.hpp decides for the cases it reads from standard
// input, one per line, for tests/test_dist_plan.py.  Host only: the header needs neither HIP nor a device.
//   B label                              -> label NEAREST CIRCLE INNER ROWS           (the values of the four cut bits)
//   K label nx k                         -> label kernel
//   C label k nx ny lon[nx] lat[ny]      -> label cuts(double) cuts(float) circle inner latmono maxstep maxstep_inner
#include <cstdio>
#include <vector>
#include "../seabreeze_param_amd/csrc/sb_dist_plan.hpp"

int main() {
    static const char *const kname[] = {"BYTES", "BITS_SMALL", "BITS32", "BITS64", "WIDE"};
    char what[8], label[128];
    while (std::scanf("%7s %127s", what, label) == 2) {
        if (what[0] == 'B') {
            std::printf("%s %d %d %d %d\n", label, (int)SB_CUT_NEAREST, (int)SB_CUT_CIRCLE, (int)SB_CUT_INNER, (int)SB_CUT_ROWS);
        } else if (what[0] == 'K') {
            int nx, k;
            if (std::scanf("%d %d", &nx, &k) != 2) return 1;
            std::printf("%s %s\n", label, kname[(int)sb_dist_kernel(nx, k)]);
        } else if (what[0] == 'C') {
            int k, nx, ny;
            if (std::scanf("%d %d %d", &k, &nx, &ny) != 3 || nx < 1 || ny < 1) return 1;
            std::vector<double> lon(nx), lat(ny);
            for (double &v : lon)
                if (std::scanf("%lf", &v) != 1) return 1;
            for (double &v : lat)
                if (std::scanf("%lf", &v) != 1) return 1;
            const std::vector<float> lonf(lon.begin(), lon.end()), latf(lat.begin(), lat.end());
            const SbDistTraits t = sb_dist_traits<double>(lon.data(), lat.data(), nx, ny);
            const SbDistTraits tf = sb_dist_traits<float>(lonf.data(), latf.data(), nx, ny);
            std::printf("%s %d %d %d %d %d %.17g %.17g\n", label, sb_dist_cuts(t, k), sb_dist_cuts(tf, k), (int)t.circle, (int)t.inner,
                        (int)t.latmono, t.maxstep, t.maxstep_inner);
        } else
            return 1;
    }
    return 0;
}
