// moments_dump.cpp -- what the host functions of seabreeze_param_amd/csrc/sb_device.hpp (moments_empty, moments_merge,
// moments_of_shifted) make of a partitioned sample, for tests/test_stats_ref.py.  It calls host functions only and never
// initialises a device.
//
// Standard input, any number of times:
//   K                       the number of parts, then for every part
//   cnt x x x ...           its size (0: an empty part) and its values (hex or decimal floats)
// Every part is reduced as a thread of k_scan reduces its cells -- shifted sums about the sample's first value c -- and
// the parts are combined in the three ways the kernels combine them.  One line each, "tag n mean m2 mn mx" in %a:
//   seq      moments_of_shifted per part, then moments_merge in index order from moments_empty
//   wave     moments_of_shifted per part, then k_merge_moments' order restated: lane l of 64 merges parts l, l + 64, ...
//            in turn, then the wave tree (lane l takes lane l + 32, 16, 8, 4, 2, 1)
//   shifted  the parts' shifted sums added up in index order, one moments_of_shifted at the end (k_prep, the strip
//            kernel's prologue, k_scan's last workgroup)
//   idl idr  moments_merge(moments_empty(), seq) and moments_merge(seq, moments_empty()): seq again, bit for bit
//   empty    moments_of_shifted(c, moments_empty())
#include <cstdio>
#include <vector>
#include "../seabreeze_param_amd/csrc/sb_device.hpp"

static void show(const char *tag, const Moments &m) {
    std::printf("%s %a %a %a %a %a\n", tag, m.n, m.mean, m.m2, m.mn, m.mx);
}

int main() {
    int k;
    while (std::scanf("%d", &k) == 1) {
        if (k < 1) return 1;
        std::vector<std::vector<double>> parts((size_t)k);
        bool have_c = false;
        double c = 0.0;
        for (auto &p : parts) {
            int cnt;
            if (std::scanf("%d", &cnt) != 1 || cnt < 0) return 1;
            p.resize((size_t)cnt);
            for (double &x : p) {
                if (std::scanf("%la", &x) != 1) return 1;
                if (!have_c) { c = x; have_c = true; }
            }
        }
        // a thread's shifted sums (sb_scan_body.hpp)
        std::vector<Moments> sh((size_t)k), mo((size_t)k);
        for (int i = 0; i < k; ++i) {
            Moments t = moments_empty();
            for (double x : parts[(size_t)i]) {
                const double d = x - c;
                t.n += 1.0; t.mean += d; t.m2 += d * d;
                t.mn = x < t.mn ? x : t.mn;
                t.mx = x > t.mx ? x : t.mx;
            }
            sh[(size_t)i] = t;
            mo[(size_t)i] = moments_of_shifted(c, t);                // (of no cells: the empty set, see "empty")
        }
        Moments seq = moments_empty();
        for (const Moments &m : mo) seq = moments_merge(seq, m);
        show("seq", seq);
        Moments lane[64];
        for (int l = 0; l < 64; ++l) {
            lane[l] = moments_empty();
            for (int b = l; b < k; b += 64) lane[l] = moments_merge(lane[l], mo[(size_t)b]);
        }
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) lane[l] = moments_merge(lane[l], lane[l + off]);
        show("wave", lane[0]);
        Moments tot = moments_empty();
        for (const Moments &t : sh) {
            tot.n += t.n; tot.mean += t.mean; tot.m2 += t.m2;
            tot.mn = t.mn < tot.mn ? t.mn : tot.mn;
            tot.mx = t.mx > tot.mx ? t.mx : tot.mx;
        }
        show("shifted", moments_of_shifted(c, tot));
        show("idl", moments_merge(moments_empty(), seq));
        show("idr", moments_merge(seq, moments_empty()));
        show("empty", moments_of_shifted(c, moments_empty()));
    }
    return 0;
}
