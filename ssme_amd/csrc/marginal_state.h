// marginal_state.h -- when do the rows of marginal smoothing (marginal.h: the weight rows om_t and the column tables m, D) hold the
// history in force?  Plain C++ (no HIP) next to SeriesHistoryState (series_history.h), which stays as it is
// (tests/cpp/test_marginal_state.cpp):
//   * the rows belong to ONE history, like the log-weight rows of backward simulation: filled by the first marginal call after the
//     recording run (query: rows_fill), reused while that history is in force (rows_filled), stale the moment the handle moves on
//     (moved_on), and their buffer goes with the history rows (dropped) or when it is too short (rows_allocate);
//   * a handle holds one of these beside its SeriesHistoryState, and every event of that state is passed on here on the same line
//     (moved_on and recorded -> moved_on, rows_dropped -> dropped).
#pragma once

namespace ssme {

struct MarginalRowsState {
    int cap = 0;     // time rows the buffer holds (0: none)
    int T = 0;       // rows of it that hold the weights of the history in force (0: not filled)

    void moved_on() { T = 0; }                              // the history the rows were formed from is no longer in force
    void dropped() { cap = 0; T = 0; }                      // the buffer is freed or about to be replaced
    void ready(int rows) { cap = rows; }                    // its allocation succeeded
    void filled(int hist_T) { T = (hist_T >= 1 && hist_T <= cap) ? hist_T : 0; }     // the kernels are queued behind the recording run
    enum Rows { rows_filled = 0, rows_fill = 1, rows_allocate = 2 };
    // have_buffer: the device pointer is non-null; hist_T: rows of the history in force (asked only while one is)
    Rows query(bool have_buffer, int hist_T) const {
        if (!have_buffer || hist_T > cap) return rows_allocate;
        return (hist_T >= 1 && T == hist_T) ? rows_filled : rows_fill;
    }
};

}  // namespace ssme
