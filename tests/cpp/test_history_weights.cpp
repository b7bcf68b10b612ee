// The life cycle of the log-weight rows of backward simulation (ssme_amd/csrc/series_history.h; backward.h), without a device: the
// sequences ssme_pf_run_series / ensure_history / backward_weights go through in pf_api.hip.  Plain C++; prints "ok" or the failed line.
#include <cstdio>

#include "../../ssme_amd/csrc/series_history.h"

using S = ssme::SeriesHistoryState;
static int failed = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failed = 1; } } while (0)

struct Handle { S s; bool rows = false, lw = false; int fills = 0, allocs = 0; };

// ssme_pf_run_series around a series of T steps (tests/cpp/test_history_state.cpp); the log-weight buffer is freed with the rows
static void run_series(Handle& h, int T, bool alloc_ok = true) {
    h.s.moved_on();
    if (!h.s.on) { h.s.rows_dropped(); h.rows = false; h.lw = false; }
    else if (T > h.s.cap) {
        h.s.rows_dropped(); h.rows = false; h.lw = false;
        if (!alloc_ok) return;
        h.s.rows_ready(T); h.rows = true;
    }
    h.s.recorded(T);
}
// backward_weights of pf_api.hip: false where the call is refused before it (no history in force) or its allocation fails
static bool backward_call(Handle& h, int T, bool alloc_ok = true) {
    if (h.s.query(h.rows, T) != S::in_force) return false;
    if (h.s.weights_query(h.lw) == S::allocate) {
        h.s.weights_dropped(); h.lw = false;
        if (!alloc_ok) return false;
        h.s.weights_ready(T); h.lw = true; ++h.allocs;
    }
    if (h.s.weights_query(true) == S::fill) { ++h.fills; h.s.weights_filled(); }
    return true;
}

int main() {
    Handle h;
    h.s.on = 1;
    EXPECT(!backward_call(h, 7));                                     // nothing recorded
    run_series(h, 7);
    EXPECT(backward_call(h, 7) && h.allocs == 1 && h.fills == 1);     // the first call allocates and fills
    EXPECT(backward_call(h, 7) && h.allocs == 1 && h.fills == 1);     // ... the second reuses the rows
    EXPECT(h.s.weights_query(h.lw) == S::filled);
    h.s.moved_on();                                                   // ssme_pf_step, reset, set_params, set_seed
    EXPECT(!backward_call(h, 7) && h.s.lw_T == 0);
    run_series(h, 7);                                                 // a second recording run: the same buffer, filled again
    EXPECT(h.s.weights_query(h.lw) == S::fill);
    EXPECT(backward_call(h, 7) && h.allocs == 1 && h.fills == 2);
    run_series(h, 5);                                                 // a shorter series in the same rows
    EXPECT(backward_call(h, 5) && h.allocs == 1 && h.fills == 3 && h.s.lw_T == 5);
    EXPECT(!backward_call(h, 7));                                     // another length than the recorded one
    run_series(h, 7);                                                 // back to 7 steps: the history rows cover them, so does the buffer
    EXPECT(backward_call(h, 7) && h.allocs == 1 && h.fills == 4);
    run_series(h, 9);                                                 // longer: the history rows are replaced and the buffer goes with them
    EXPECT(!h.lw && h.s.lw_cap == 0 && h.s.weights_query(h.lw) == S::allocate);
    EXPECT(backward_call(h, 9) && h.allocs == 2 && h.fills == 5);
    run_series(h, 12, false);                                         // refused rows: no history, no buffer
    EXPECT(!h.rows && !h.lw && !backward_call(h, 12) && !backward_call(h, 9));
    run_series(h, 12);
    EXPECT(!backward_call(h, 12, false) && !h.lw && h.s.lw_cap == 0 && h.s.lw_T == 0);   // a refused buffer leaves none ...
    EXPECT(backward_call(h, 12) && h.allocs == 3 && h.fills == 6);                        // ... and the handle usable
    // a history recorded in rows longer than the buffer: series of 5 in rows of 12 first, then 12
    run_series(h, 5);
    EXPECT(backward_call(h, 5) && h.allocs == 3);
    h.s.on = 0;
    run_series(h, 5);                                                 // recording off: rows and buffer are freed
    EXPECT(!h.rows && !h.lw && h.s.lw_cap == 0 && !backward_call(h, 5));
    S t;
    t.on = 1; t.cap = 8; t.recorded(8); t.weights_ready(4);           // a buffer the history does not fit is never "filled"
    t.weights_filled();
    EXPECT(t.lw_T == 0 && t.weights_query(true) == S::allocate);
    if (!failed) std::printf("ok\n");
    return failed;
}
