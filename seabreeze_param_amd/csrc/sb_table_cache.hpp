// sb_table_cache.hpp -- the stored windows of the table contrast (sb_set_table_window_cache): the word of plane W, and the
// host's half of the decision whether a table call searches every band cell's window afresh ("fills") or takes it from W.
// The other half is the device's: k_scan compares both bit planes with what the call before left and reports a difference
// under this call's number, so the table kernels evaluate  fill = host_force || *plan_gen == call_id.  The device sees a
// coast that moved; only the host knows WHICH call left the planes k_scan compared with -- and W belongs to the planes of
// the last table call that ran with the cache in effect.  Plain C++17: no HIP, no heap -- a host compiler builds it alone
// (tests/plan_dump.cpp).
#pragma once

#ifndef SB_TAB_REACH
#define SB_TAB_REACH 127            // (sb_launch.hpp states it, with the format it follows from)
#endif

// W: 32 bits per interior cell.  0: the tables do not answer this cell (beyond the reach, wider than the circle, one class
// as far as the search may go: the global-memory search, every call -- t0 changes).  Else radius | nl << 8: the smallest
// radius whose square holds both classes, 1 .. SB_TAB_REACH, and the land-side cells in that square, 0 < nl < (2 radius + 1)^2.
static_assert(SB_TAB_REACH >= 1 && SB_TAB_REACH < (1 << 8), "the radius of a stored window has eight bits");
static_assert((2 * SB_TAB_REACH + 1) * (2 * SB_TAB_REACH + 1) <= (1 << 24), "the land-side count of a stored window has 24 bits");
constexpr unsigned sb_tab_pack(int radius, int nl) { return (unsigned)radius | ((unsigned)nl << 8); }
constexpr int sb_tab_radius(unsigned w) { return (int)(w & 255u); }
constexpr int sb_tab_nl(unsigned w) { return (int)(w >> 8); }

// what W was filled for: the geometry, and where the planes it follows from and the workspace live (a reallocated plane or
// table is another plane or table)
struct SbTabKey {
    int nx, ny, h, bnd, rows;
    const void *band, *cls, *W, *C;
};
inline bool sb_tab_key_equal(const SbTabKey &a, const SbTabKey &b) {
    return a.nx == b.nx && a.ny == b.ny && a.h == b.h && a.bnd == b.bnd && a.rows == b.rows && a.band == b.band && a.cls == b.cls &&
           a.W == b.W && a.C == b.C;
}

// why the host forces a fill (SB_TAB_STEADY: it does not, the device decides by the planes alone)
enum SbTabForce { SB_TAB_STEADY = 0, SB_TAB_NO_KEY, SB_TAB_KEY_DIFFERS, SB_TAB_SEQ_RESTART, SB_TAB_TOGGLED, SB_TAB_FAILED, SB_TAB_OTHER_CALL };

struct SbTabCache {
    bool have_key = false;          // a call with the cache in effect was enqueued whole and nothing has dropped its key since
    SbTabKey key{};
    int seq = 0;                    // that call's number (sb_ctx::call_seq)
    bool toggled = false;           // sb_set_table_window_cache since
    bool failed = false;            // a launch of a diag call or band step failed since
    bool other = false;             // k_scan ran on the context's planes in a call that was not such a table call
};

// the call `seq` with key `key` is about to be enqueued with the cache in effect
inline SbTabForce sb_tab_cache_decide(const SbTabCache &s, const SbTabKey &key, int seq) {
    if (s.toggled) return SB_TAB_TOGGLED;
    if (s.failed) return SB_TAB_FAILED;
    if (s.other) return SB_TAB_OTHER_CALL;
    if (!s.have_key) return SB_TAB_NO_KEY;
    if (!sb_tab_key_equal(s.key, key)) return SB_TAB_KEY_DIFFERS;
    if (seq <= s.seq) return SB_TAB_SEQ_RESTART;        // (the numbers started over: *plan_gen of an earlier era means nothing)
    return SB_TAB_STEADY;
}
// ... and it was, every launch of it
inline void sb_tab_cache_filled(SbTabCache &s, const SbTabKey &key, int seq) {
    s = SbTabCache{};
    s.have_key = true; s.key = key; s.seq = seq;
}
// every other diag call or band step that runs k_scan: the f2py flavour and a stream step unless they run as table calls
// themselves (sb_set_table_contrast_f2py), a band step, a call with either switch off or with gathered moments in use
inline void sb_tab_cache_other_call(SbTabCache &s) { s.have_key = false; s.other = true; }
inline void sb_tab_cache_launch_failed(SbTabCache &s) { s.have_key = false; s.failed = true; }
inline void sb_tab_cache_toggled(SbTabCache &s) { s.have_key = false; s.toggled = true; }
