// ice_plan_dump.cpp -- prints what seabreeze_param_amd/csrc/sb_ice_plan.hpp decides for the cases it reads from standard
// input, one per line, for tests/test_ice_plan.py.  Host only: the header needs neither HIP nor a device.
//   P label nx k incremental             -> label WHOLE | DELTA
//   M label nx ny k n x1 y1 .. xn yn     -> label ntiles then ny * ntiles marks (0 / 1), row by row: what the words that
//                                           hold the changed cells (x, y) mark, each word once, as k_edge_bits_delta does
#include <cstdio>
#include <set>
#include <utility>
#include <vector>
#include "../seabreeze_param_amd/csrc/sb_ice_plan.hpp"

int main() {
    char what[8], label[128];
    while (std::scanf("%7s %127s", what, label) == 2) {
        if (what[0] == 'P') {
            int nx, k, inc;
            if (std::scanf("%d %d %d", &nx, &k, &inc) != 3) return 1;
            std::printf("%s %s\n", label, sb_ice_path(nx, k, inc) == SbIcePath::WHOLE ? "WHOLE" : "DELTA");
        } else if (what[0] == 'M') {
            int nx, ny, k, n;
            if (std::scanf("%d %d %d %d", &nx, &ny, &k, &n) != 4 || nx < 1 || ny < 1 || n < 0) return 1;
            const int nt = sb_ice_tiles(nx);
            std::vector<unsigned char> marks((size_t)ny * nt, 0);
            std::set<std::pair<int, int>> words;
            for (int i = 0; i < n; ++i) {
                int x, y;
                if (std::scanf("%d %d", &x, &y) != 2 || x < 0 || x >= nx || y < 0 || y >= ny) return 1;
                words.insert({x & ~63, y});
            }
            for (const auto &w : words) {
                const SbIceReach r = sb_ice_reach(nx, ny, k, w.first, w.second);
                for (int yt = r.r0; yt <= r.r1; ++yt) {
                    for (int t = r.a0; t <= r.a1; ++t) marks[(size_t)yt * nt + t] = 1;
                    for (int t = r.b0; t <= r.b1; ++t) marks[(size_t)yt * nt + t] = 1;
                }
            }
            std::printf("%s %d", label, nt);
            for (unsigned char m : marks) std::printf(" %d", (int)m);
            std::printf("\n");
        } else
            return 1;
    }
    return 0;
}
