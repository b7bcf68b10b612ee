// The rules of ssme_amd/csrc/series_history.h (when a recorded series history is in force), without a device: the sequences
// ssme_pf_run_series / ensure_history / the smoothing calls go through in pf_api.hip, among them a REFUSED allocation of larger rows
// after a recorded series, after which no call may be answered from the freed rows.  Plain C++; prints "ok" or the failed line.
#include <cstdio>

#include "../../ssme_amd/csrc/series_history.h"

using S = ssme::SeriesHistoryState;
static int failed = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failed = 1; } } while (0)

// what ssme_pf_run_series does to the state around a series of T steps; alloc_ok: does an allocation of new rows succeed?
// Returns whether the device rows exist afterwards (have_rows of query()).
static bool run_series(S& s, bool have_rows, int T, bool alloc_ok, bool series_ok = true) {
    s.moved_on();
    if (!s.on) { s.rows_dropped(); have_rows = false; }
    else if (T > s.cap) {
        s.rows_dropped(); have_rows = false;
        if (!alloc_ok) return have_rows;                  // SSME_ERR_HIP: run_series returns here
        s.rows_ready(T); have_rows = true;
    }
    if (!series_ok) return have_rows;                     // a later HIP call failed: nothing was recorded
    s.recorded(T);
    return have_rows;
}

int main() {
    S s;
    bool rows = false;
    EXPECT(s.query(rows, 7) == S::none);                  // a new handle
    rows = run_series(s, rows, 7, true);
    EXPECT(s.query(rows, 7) == S::none);                  // recording was off
    s.on = 1;
    EXPECT(s.query(rows, 7) == S::none);                  // switched on, no run_series yet
    rows = run_series(s, rows, 7, true);
    EXPECT(rows && s.query(rows, 7) == S::in_force && s.query(rows, 6) == S::other_length && s.query(rows, 8) == S::other_length);
    // a longer series whose rows are refused: the old rows are freed, so the old history must not stay in force
    rows = run_series(s, rows, 9, false);
    EXPECT(!rows && s.cap == 0);
    EXPECT(s.query(rows, 7) == S::none && s.query(rows, 9) == S::none);
    EXPECT(s.query(true, 7) == S::none);                  // ... whatever the pointers say
    // the handle stays usable: the same request granted later records again
    rows = run_series(s, rows, 9, true);
    EXPECT(rows && s.query(rows, 9) == S::in_force && s.query(rows, 7) == S::other_length);
    // rows replaced successfully, then the series itself fails: the new rows are unwritten and nothing is in force
    rows = run_series(s, rows, 12, true, false);
    EXPECT(rows && s.cap == 12 && s.query(rows, 12) == S::none && s.query(rows, 9) == S::none);
    // a shorter series in the larger rows; a failure of a run that needs no new rows also ends the earlier history
    rows = run_series(s, rows, 5, true);
    EXPECT(s.query(rows, 5) == S::in_force);
    rows = run_series(s, rows, 5, true, false);
    EXPECT(s.query(rows, 5) == S::none);
    rows = run_series(s, rows, 5, true);
    s.moved_on();                                         // ssme_pf_step, reset, set_params, set_seed
    EXPECT(s.query(rows, 5) == S::none);
    rows = run_series(s, rows, 5, true);
    EXPECT(s.query(false, 5) == S::none);                 // never in force without rows
    s.on = 0;
    rows = run_series(s, rows, 5, true);
    EXPECT(!rows && s.cap == 0 && s.query(rows, 5) == S::none);
    s.on = 1; s.cap = 3; s.recorded(4);                   // a length the rows do not cover is never recorded
    EXPECT(s.T == 0);
    if (!failed) std::printf("ok\n");
    return failed;
}
