// band_plan_dump.cpp -- prints what seabreeze_param_amd/csrc/sb_dist_plan.hpp decides for a latitude band's frame, for the
// cases it reads from standard input, one per line, for tests/test_band_plan.py.  Host only, like dist_plan_dump.cpp.
//   R label ny halo south north k                          -> label f0 nys r0 r1
//   T label ny halo south north k nx lon[nx] lat[ny+2halo] -> label cuts circle inner latmono   (traits over the source rows'
//                                                             latitudes only; "nan" is a valid entry)
#include <cstdio>
#include <vector>
#include "../seabreeze_param_amd/csrc/sb_dist_plan.hpp"

int main() {
    char what[8], label[128];
    while (std::scanf("%7s %127s", what, label) == 2) {
        int ny, halo, south, north, k;
        if (std::scanf("%d %d %d %d %d", &ny, &halo, &south, &north, &k) != 5) return 1;
        const SbBandRows b = sb_band_rows(ny, halo, south != 0, north != 0, k);
        if (what[0] == 'R') {
            std::printf("%s %d %d %d %d\n", label, b.f0, b.nys, b.r0, b.r1);
        } else if (what[0] == 'T') {
            int nx;
            if (std::scanf("%d", &nx) != 1 || nx < 1 || ny < 1 || halo < 0) return 1;
            std::vector<double> lon(nx), lat(ny + 2 * halo);
            for (double &v : lon)
                if (std::scanf("%lf", &v) != 1) return 1;
            for (double &v : lat)
                if (std::scanf("%lf", &v) != 1) return 1;
            if (b.f0 < 0 || b.f0 + b.nys > ny + 2 * halo) return 1;
            const SbDistTraits t = sb_dist_traits<double>(lon.data(), lat.data() + b.f0, nx, b.nys);
            std::printf("%s %d %d %d %d\n", label, sb_dist_cuts(t, k), (int)t.circle, (int)t.inner, (int)t.latmono);
        } else
            return 1;
    }
    return 0;
}
