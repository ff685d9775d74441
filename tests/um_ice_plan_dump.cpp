// um_ice_plan_dump.cpp -- prints what seabreeze_param_amd/csrc/sb_ice_plan.hpp decides for a UM-layout coast that moves
// (sb_um_coast_open / sb_um_ice_*), for the cases it reads from standard input, one per line, for
// tests/test_um_ice_plan.py.  Host only: the header needs neither HIP nor a device.
//   P label nx ny hi hj wi wj incremental -> label NONE | (WHOLE | DELTA) nw ngroups ntiles
//   M label nx ny wi wj n x1 y1 .. xn yn  -> label ngroups ntiles then ngroups * ntiles marks (0 / 1), row group by row
//                                            group: what the words that hold the changed cells (interior column x, row y)
//                                            mark, each word once, as k_edge_bits_delta_um does
#include <cstdio>
#include <set>
#include <utility>
#include <vector>
#include "../seabreeze_param_amd/csrc/sb_ice_plan.hpp"

static_assert(SB_UM_ICE_ROWS == 4 && SB_UM_ICE_COLS == 64, "the tests' model states the tile as 4 x 64");

int main() {
    char what[8], label[128];
    while (std::scanf("%7s %127s", what, label) == 2) {
        int nx, ny;
        if (std::scanf("%d %d", &nx, &ny) != 2) return 1;
        if (what[0] == 'P') {
            int hi, hj, wi, wj, inc;
            if (std::scanf("%d %d %d %d %d", &hi, &hj, &wi, &wj, &inc) != 5) return 1;
            const SbUmIcePlan p = sb_um_ice_plan(nx, ny, hi, hj, wi, wj, inc);
            if (!p.ok) std::printf("%s NONE\n", label);
            else
                std::printf("%s %s %d %d %d\n", label, p.path == SbIcePath::WHOLE ? "WHOLE" : "DELTA", p.nw, p.ngroups, p.ntiles);
            if (p.ok && p.path != sb_um_ice_path(inc)) return 3;
        } else if (what[0] == 'M') {
            int wi, wj, n;
            if (std::scanf("%d %d %d", &wi, &wj, &n) != 3 || n < 0 || nx < 1 || ny < 1) return 1;
            const int ng = sb_um_ice_groups(ny), nt = sb_um_ice_tiles(nx);
            std::vector<unsigned char> marks((size_t)ng * nt, 0);
            std::set<std::pair<int, int>> words;
            for (int i = 0; i < n; ++i) {
                int x, y;
                if (std::scanf("%d %d", &x, &y) != 2 || x < 0 || x >= nx || y < 0 || y >= ny) return 1;
                words.insert({x & ~63, y});
            }
            for (const auto &w : words) {
                const SbUmIceReach r = sb_um_ice_reach(nx, ny, wi, wj, w.first, w.second);
                // a mark outside the plane: the kernel would write out of bounds
                if (r.g0 < 0 || r.g1 >= ng || r.t0 < 0 || r.t1 >= nt || r.g0 > r.g1 || r.t0 > r.t1) return 2;
                for (int g = r.g0; g <= r.g1; ++g)
                    for (int t = r.t0; t <= r.t1; ++t) marks[(size_t)g * nt + t] = 1;
            }
            std::printf("%s %d %d", label, ng, nt);
            for (unsigned char m : marks) std::printf(" %d", (int)m);
            std::printf("\n");
        } else
            return 1;
    }
    return 0;
}
