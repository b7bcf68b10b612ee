"""The cases at which a recorded Liu-West series (ssme_lw_set_series_expectations) is pinned to the step API's read-out
(tests/test_lw_series_expect_gpu.py), importable without a GPU.

A case is a dict in the format of lw_edge_cases; every base case runs for both forms.  Every listed case compares all T x 8 x R values.
The schedules and the degenerate inputs are lw_series_cases' own, by name."""
import lw_edge_cases as lc
import lw_series_cases as sc

VIRTUAL_THREADS = 256                          # k_lw_param_partials: virtual thread v adds particles v, v + 256, ...
# the wave edge of the virtual threads (63 .. 65), 256 where a virtual thread goes from one term to two, 512, and the half-tile and
# tile edges of the series kernel's own 512 x 2 x 2 map
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 500, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
TILED_ONLY = (2049, 5000)                      # two and three tiles: the tiled route alone serves them
DEGENERATE = sc.DEGENERATE
N_VALUES = 8                                   # ids 0-3: x, x^2, exp(x/2), 42; 4-7: phi, mu, sigma, rho
NAN_Y_STEP = 2                                 # nan-y-R3: y[2] = NaN


def _both(base):
    return [dict(c, name=f"{c['name']}-form{form}", form=form, base=c["name"]) for c in base for form in (0, 1)]


def size_cases():
    return _both([lc._c(f"rec-n{n}", n=n, T=6) for n in SIZES])


def schedule_cases():
    """resamp_sched 2 and 3 at T = 7, and T = 1 and 2: lw_series_cases' list."""
    return sc.schedule_cases()


def degenerate_cases():
    return sc.degenerate_cases()


def tiled_only_cases():
    return _both([lc._c(f"rec-tiled-n{n}", n=n, T=4) for n in TILED_ONLY])


def all_cases():
    return size_cases() + schedule_cases() + degenerate_cases() + tiled_only_cases()


def invisible_cases():
    """Recording against not recording: both routes at resamp_sched 1 and 2, both forms; 5 steps of series, then 3 filter() calls."""
    return _both([lc._c(f"rec-invisible-rs{rs}", n=700, T=8, rs=rs) for rs in (1, 2)])


LONG_N, LONG_T = sc.LONG_N, sc.LONG_T          # the first 300 rows of spy_returns.csv, z its lag
BANK_N, BANK_R, BANK_T = sc.BANK_N, sc.BANK_R, sc.BANK_T
BANK_STEPPED = sc.BANK_ORACLE_REPS             # filters 0, 1, 99 against stepped twins with first_filter_id 0, 1, 99
