// series_history.h -- when is a recorded series history in force?  The host-side state of ssme_pf_set_series_history, kept apart from
// pf_api.hip as plain C++ (no HIP), so that its rules are tested without a device (tests/cpp/test_history_state.cpp):
//   * a history is in force from the end of a recording ssme_pf_run_series until the handle moves on (moved_on: the start of any
//     run_series, ssme_pf_step, do_reset) or its rows are freed or replaced (rows_dropped: also a REFUSED allocation, after which the
//     handle holds no rows at all);
//   * the smoothing calls ask query(): never SSME_OK unless rows exist, cover the recorded length and the caller's T is that length;
//   * the log-weight rows of backward simulation (backward.h) belong to ONE history: they are filled on the first backward call after
//     the recording run (weights_query: fill), reused while that history is in force (filled), stale the moment it is not
//     (moved_on, recorded), and their buffer goes with the history rows (rows_dropped) or when it is too short (allocate).
#pragma once

namespace ssme {

struct SeriesHistoryState {
    int on = 0;      // the setting (ssme_pf_set_series_history)
    int cap = 0;     // time rows the device buffers hold (0: none)
    int T = 0;       // rows of the history in force (0: none)
    int lw_cap = 0;  // time rows the log-weight buffer of backward simulation holds (0: none)
    int lw_T = 0;    // rows of it that hold the log-weights of the history in force (0: not filled)

    void moved_on() { T = 0; lw_T = 0; }                    // the state the smoothing weights live in is changed or discarded
    void rows_dropped() { cap = 0; T = 0; lw_cap = 0; lw_T = 0; }   // the rows are freed or about to be replaced: whatever they held is gone, the log-weight buffer with them
    void rows_ready(int rows) { cap = rows; }               // both allocations succeeded
    void recorded(int steps) { T = (on && steps <= cap) ? steps : 0; lw_T = 0; }     // a run_series has queued and finished `steps` steps

    // the log-weight rows of the history in force
    void weights_dropped() { lw_cap = 0; lw_T = 0; }        // the buffer is freed or about to be replaced
    void weights_ready(int rows) { lw_cap = rows; }         // its allocation succeeded
    void weights_filled() { lw_T = (T >= 1 && T <= lw_cap) ? T : 0; }      // the fill kernel is queued behind the recording run
    enum Weights { filled = 0, fill = 1, allocate = 2 };
    // have_buffer: the device pointer is non-null.  Asked only while a history is in force (query() == in_force).
    Weights weights_query(bool have_buffer) const {
        if (!have_buffer || T > lw_cap) return allocate;
        return (T >= 1 && lw_T == T) ? filled : fill;
    }

    enum Answer { in_force = 0, none = 1, other_length = 2 };
    // have_rows: both device pointers are non-null
    Answer query(bool have_rows, int T_asked) const {
        if (T < 1 || !have_rows || T > cap) return none;
        return T_asked == T ? in_force : other_length;
    }
};

}  // namespace ssme
