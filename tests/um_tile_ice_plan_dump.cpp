// um_tile_ice_plan_dump.cpp -- what an ice call of one UM tile decides on the host (sb_um_tile_ice_plan, sb_um_tile_ice_reach:
// seabreeze_param_amd/csrc/sb_ice_plan.hpp), printed for tests/test_um_tile_ice_plan.py.  Host-only: no HIP, no device.
// Lines on stdin, one answer line each:
//   P label nx ny hi hj wi wj bW bE bS bN inc   ->  label NONE  |  label WHOLE|DELTA eW eE eS eN nw rows tiles
//   M label nx ny wi wj bW bE bS bN n  x0 s ... ->  label rows tiles  marks (rows x tiles, row by row) of the union of the reach
//                                                   of the n words (x0, s) of the SOURCE rectangle's bit plane (x0 is rounded
//                                                   down to a multiple of 64)
// Exit status 1: a line it cannot read or a word outside the rectangle; 2: a reach outside the mark plane or empty (the
// kernel would write out of bounds, or leave a word without a mark).
#include "../seabreeze_param_amd/csrc/sb_ice_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

namespace {

bool ints(char *&p, int *v, int n) {
    for (int i = 0; i < n; ++i) {
        char *end;
        const long x = std::strtol(p, &end, 10);
        if (end == p) return false;
        v[i] = (int)x;
        p = end;
    }
    return true;
}

}  // namespace

int main() {
    static char line[1 << 16];
    while (std::fgets(line, sizeof line, stdin)) {
        char what[8], label[128];
        int at = 0;
        if (std::sscanf(line, "%7s %127s%n", what, label, &at) != 2) continue;
        char *p = line + at;
        if (what[0] == 'P') {
            int v[11];
            if (!ints(p, v, 11)) return 1;
            const SbUmTileIcePlan pl = sb_um_tile_ice_plan(v[0], v[1], v[2], v[3], v[4], v[5], v + 6, v[10]);
            if (!pl.ok) std::printf("%s NONE\n", label);
            else
                std::printf("%s %s %d %d %d %d %d %d %d\n", label, pl.path == SbIcePath::WHOLE ? "WHOLE" : "DELTA", pl.reach.eW,
                            pl.reach.eE, pl.reach.eS, pl.reach.eN, pl.nw, pl.marks.rows, pl.marks.tiles);
            continue;
        }
        if (what[0] != 'M') return 1;
        int v[8], n, xy[2];
        if (!ints(p, v, 8) || !ints(p, &n, 1) || n < 0 || v[0] < 1 || v[1] < 1) return 1;
        const int nx = v[0], ny = v[1], wi = v[2], wj = v[3];
        const SbTileReach e = sb_um_tile_ice_sources(wi, wj, v + 4);
        const SbIceMarks m = sb_um_ice_marks(nx, ny);
        std::set<std::pair<int, int>> words;
        for (int i = 0; i < n; ++i) {
            if (!ints(p, xy, 2) || xy[0] < 0 || xy[0] >= nx + e.eW + e.eE || xy[1] < 0 || xy[1] >= ny + e.eS + e.eN) return 1;
            words.insert({xy[0] & ~63, xy[1]});
        }
        std::vector<unsigned char> marks((size_t)m.rows * m.tiles, 0);
        for (const auto &w : words) {
            const SbIceReach r = sb_um_tile_ice_reach(nx, ny, wi, wj, e.eW, e.eS, w.first, w.second);
            if (r.r0 < 0 || r.r1 >= m.rows || r.r0 > r.r1 || r.a0 < 0 || r.a1 >= m.tiles || r.a0 > r.a1) return 2;
            if (r.b0 <= r.b1) return 2;                                  // (nothing wraps: no second piece)
            for (int y = r.r0; y <= r.r1; ++y)
                for (int t = r.a0; t <= r.a1; ++t) marks[(size_t)y * m.tiles + t] = 1;
        }
        std::printf("%s %d %d", label, m.rows, m.tiles);
        for (unsigned char b : marks) std::printf(" %d", (int)b);
        std::printf("\n");
    }
    return 0;
}
