// The life cycle of the rows of marginal smoothing (ssme_amd/csrc/marginal_state.h; marginal.h), without a device: the sequences
// ssme_pf_run_series / ensure_history / backward_weights / marginal_rows go through in pf_api.hip.  Plain C++; prints "ok" or the
// failed line.
#include <cstdio>

#include "../../ssme_amd/csrc/series_history.h"
#include "../../ssme_amd/csrc/marginal_state.h"

using B = ssme::SeriesHistoryState;
using M = ssme::MarginalRowsState;
static int failed = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failed = 1; } } while (0)

struct Handle { B s; M m; bool rows = false, lw = false, ms = false; int fills = 0, allocs = 0, lw_fills = 0; };

// ssme_pf_run_series around a series of T steps; the log-weight buffer and the marginal rows are freed with the history rows
static void run_series(Handle& h, int T, bool alloc_ok = true) {
    h.s.moved_on(); h.m.moved_on();
    if (!h.s.on) { h.s.rows_dropped(); h.m.dropped(); h.rows = h.lw = h.ms = false; }
    else if (T > h.s.cap) {
        h.s.rows_dropped(); h.m.dropped(); h.rows = h.lw = h.ms = false;
        if (!alloc_ok) return;
        h.s.rows_ready(T); h.rows = true;
    }
    h.s.recorded(T); h.m.moved_on();
}
// backward_weights of pf_api.hip (allocations succeed here)
static void backward_weights(Handle& h, int T) {
    if (h.s.weights_query(h.lw) == B::allocate) { h.s.weights_dropped(); h.s.weights_ready(T); h.lw = true; }
    if (h.s.weights_query(true) == B::fill) { ++h.lw_fills; h.s.weights_filled(); }
}
// a marginal call: false where it is refused before marginal_rows (no history in force) or the allocation of the rows fails
static bool marginal_call(Handle& h, int T, bool alloc_ok = true) {
    if (h.s.query(h.rows, T) != B::in_force) return false;
    backward_weights(h, T);
    if (h.m.query(h.ms, h.s.T) == M::rows_allocate) {
        h.m.dropped(); h.ms = false;
        if (!alloc_ok) return false;
        h.m.ready(T); h.ms = true; ++h.allocs;
    }
    if (h.m.query(true, h.s.T) == M::rows_fill) { ++h.fills; h.m.filled(h.s.T); }
    return true;
}

int main() {
    Handle h;
    h.s.on = 1;
    EXPECT(!marginal_call(h, 7));                                     // nothing recorded
    run_series(h, 7);
    EXPECT(marginal_call(h, 7) && h.allocs == 1 && h.fills == 1 && h.lw_fills == 1);     // the first call allocates and fills both
    EXPECT(marginal_call(h, 7) && h.allocs == 1 && h.fills == 1 && h.lw_fills == 1);     // ... the second reuses the rows
    EXPECT(h.m.query(h.ms, h.s.T) == M::rows_filled);
    h.s.moved_on(); h.m.moved_on();                                   // ssme_pf_step, reset, set_params, set_seed
    EXPECT(!marginal_call(h, 7) && h.m.T == 0 && h.s.lw_T == 0 && h.s.T == 0);
    run_series(h, 7);                                                 // a second recording run: the same buffers, filled again
    EXPECT(h.m.query(h.ms, h.s.T) == M::rows_fill);
    backward_weights(h, 7);                                           // backward simulation first: the marginal rows are still stale
    EXPECT(h.s.weights_query(h.lw) == B::filled && h.m.query(h.ms, h.s.T) == M::rows_fill);
    EXPECT(marginal_call(h, 7) && h.allocs == 1 && h.fills == 2 && h.lw_fills == 2);
    run_series(h, 7);                                                 // the SAME length again: nothing of the run before is handed out
    EXPECT(h.m.query(h.ms, h.s.T) == M::rows_fill && marginal_call(h, 7) && h.fills == 3);
    run_series(h, 5);                                                 // a shorter series in the same rows
    EXPECT(marginal_call(h, 5) && h.allocs == 1 && h.fills == 4 && h.m.T == 5);
    EXPECT(!marginal_call(h, 7));                                     // another length than the recorded one
    run_series(h, 7);                                                 // back to 7 steps: the buffers cover them
    EXPECT(marginal_call(h, 7) && h.allocs == 1 && h.fills == 5);
    run_series(h, 9);                                                 // longer: the history rows are replaced and the marginal rows go with them
    EXPECT(!h.ms && h.m.cap == 0 && h.m.query(h.ms, h.s.T) == M::rows_allocate);
    EXPECT(marginal_call(h, 9) && h.allocs == 2 && h.fills == 6);
    run_series(h, 12, false);                                         // refused history rows: no history, no buffers
    EXPECT(!h.rows && !h.ms && !marginal_call(h, 12) && !marginal_call(h, 9));
    run_series(h, 12);
    EXPECT(!marginal_call(h, 12, false) && !h.ms && h.m.cap == 0 && h.m.T == 0);   // refused marginal rows leave none ...
    EXPECT(h.s.query(h.rows, 12) == B::in_force && h.s.weights_query(h.lw) == B::filled);  // ... the history in force, its log-weights filled
    EXPECT(marginal_call(h, 12) && h.allocs == 3 && h.fills == 7);                         // ... and the handle usable
    h.s.on = 0;
    run_series(h, 5);                                                 // recording off: everything is freed
    EXPECT(!h.rows && !h.ms && h.m.cap == 0 && !marginal_call(h, 5));
    M t;
    t.ready(4); t.filled(8);                                          // a buffer the history does not fit is never "filled"
    EXPECT(t.T == 0 && t.query(true, 8) == M::rows_allocate);
    if (!failed) std::printf("ok\n");
    return failed;
}
