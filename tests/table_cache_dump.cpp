// table_cache_dump.cpp -- drives the host's half of the window cache of the table contrast (seabreeze_param_amd/csrc/
// sb_table_cache.hpp: sb_set_table_window_cache) from standard input, one command per line, for
// tests/test_table_cache_host.py.  Host only.
//
//   call nx ny h bnd rows band cls W C seq   a call with the cache in effect is about to be enqueued: prints why the host
//                                            forces a fill (or "steady"), then notes the call as enqueued whole
//   other | failed | toggled                 another diag call or band step ran k_scan; a launch failed; the switch was set
//   word found radius nl                     prints the word of plane W for a cell and what the query reads back from it:
//                                            "word radius nl"
// The addresses are small integers: the key compares them, nothing reads through them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../seabreeze_param_amd/csrc/sb_table_cache.hpp"

int main() {
    static const char *const why[] = {"steady", "no_key", "key_differs", "seq_restart", "toggled", "failed", "other_call"};
    SbTabCache s;
    char cmd[32];
    while (std::scanf("%31s", cmd) == 1) {
        if (!std::strcmp(cmd, "call")) {
            long long v[10];
            for (long long &x : v)
                if (std::scanf("%lld", &x) != 1) return 1;
            const SbTabKey key{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (const void *)(uintptr_t)v[5],
                               (const void *)(uintptr_t)v[6], (const void *)(uintptr_t)v[7], (const void *)(uintptr_t)v[8]};
            std::printf("%s\n", why[(int)sb_tab_cache_decide(s, key, (int)v[9])]);
            sb_tab_cache_filled(s, key, (int)v[9]);
        } else if (!std::strcmp(cmd, "other")) sb_tab_cache_other_call(s);
        else if (!std::strcmp(cmd, "failed")) sb_tab_cache_launch_failed(s);
        else if (!std::strcmp(cmd, "toggled")) sb_tab_cache_toggled(s);
        else if (!std::strcmp(cmd, "word")) {
            int found, r, nl;
            if (std::scanf("%d %d %d", &found, &r, &nl) != 3) return 1;
            const unsigned w = found ? sb_tab_pack(r, nl) : 0u;
            std::printf("%u %d %d\n", w, sb_tab_radius(w), sb_tab_nl(w));
        } else return 1;
    }
    return 0;
}
