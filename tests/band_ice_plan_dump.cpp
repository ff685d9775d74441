// band_ice_plan_dump.cpp -- prints what seabreeze_param_amd/csrc/sb_ice_plan.hpp decides for a latitude band whose coast
// moves (sb_band_coast_open / sb_band_ice_*), for the cases it reads from standard input, one per line, for
// tests/test_band_ice_plan.py.  Host only: the header needs neither HIP nor a device.
//   P label nx ny halo south north k incremental -> label NONE | (WHOLE | DELTA) f0 nys r0 r1 nw ntiles
//   M label nx ny halo south north k n x1 s1 .. xn sn
//                                                -> label ntiles then ny * ntiles marks (0 / 1), own row by own row: what
//                                                   the words that hold the changed cells (column x, SOURCE row s) mark,
//                                                   each word once, as k_edge_bits_delta_band does
#include <cstdio>
#include <set>
#include <utility>
#include <vector>
#include "../seabreeze_param_amd/csrc/sb_ice_plan.hpp"

int main() {
    char what[8], label[128];
    while (std::scanf("%7s %127s", what, label) == 2) {
        int nx, ny, halo, south, north, k;
        if (std::scanf("%d %d %d %d %d %d", &nx, &ny, &halo, &south, &north, &k) != 6 || nx < 1 || ny < 1) return 1;
        if (what[0] == 'P') {
            int inc;
            if (std::scanf("%d", &inc) != 1) return 1;
            const SbBandIcePlan p = sb_band_ice_plan(nx, ny, halo, south != 0, north != 0, k, inc);
            if (!p.ok) std::printf("%s NONE\n", label);
            else
                std::printf("%s %s %d %d %d %d %d %d\n", label, p.path == SbIcePath::WHOLE ? "WHOLE" : "DELTA", p.rows.f0, p.rows.nys,
                            p.rows.r0, p.rows.r1, p.nw, p.ntiles);
        } else if (what[0] == 'M') {
            int n;
            if (std::scanf("%d", &n) != 1 || n < 0) return 1;
            const SbBandIcePlan p = sb_band_ice_plan(nx, ny, halo, south != 0, north != 0, k, 1);
            if (!p.ok) return 1;
            const int nt = p.ntiles, r0 = p.rows.r0, r1 = p.rows.r1;
            std::vector<unsigned char> marks((size_t)ny * nt, 0);
            std::set<std::pair<int, int>> words;
            for (int i = 0; i < n; ++i) {
                int x, s;
                if (std::scanf("%d %d", &x, &s) != 2 || x < 0 || x >= nx || s < 0 || s >= p.rows.nys) return 1;
                words.insert({x & ~63, s});
            }
            for (const auto &w : words) {
                const SbIceReach r = sb_band_ice_reach(nx, r0, r1, k, w.first, w.second);
                for (int yt = r.r0; yt <= r.r1; ++yt) {
                    if (yt < r0 || yt >= r1) return 2;           // a mark outside the plane: the kernel would write out of bounds
                    for (int t = r.a0; t <= r.a1; ++t) marks[(size_t)(yt - r0) * nt + t] = 1;
                    for (int t = r.b0; t <= r.b1; ++t) marks[(size_t)(yt - r0) * nt + t] = 1;
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
