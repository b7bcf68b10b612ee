"""The cases at which the whole-series Liu-West kernel (ssme_amd/csrc/lw_small.h) is pinned to the tiled route and to the oracle
(tests/test_lw_series_gpu.py), importable without a GPU.  test_lw_series_cpu.py walks the list through the oracle alone and proves
that every case reaches what it is listed for.

A case is a dict in the format of lw_edge_cases (its `series`, `prior` and `oracle_filters` read it); every base case runs for both
forms.  The degenerate inputs are lw_edge_cases' own, by name (N = 700, T = 5)."""
import lw_edge_cases as lc

ONE_TILE = 2048                                # the series route serves N <= 2048
SIZES = (1, 2, 3, 63, 64, 65, 500, 1023, 1024, 1025, 2047, 2048)      # wave, half-tile (k = 0 / 1) and tile edges of the 512 x 2 x 2 map
TILED_ONLY = 2049                              # the first size of two tiles
DEGENERATE = ("nan-y", "inf-weights", "nan-z", "huge-y", "delta1", "point-prior", "one-dim-point", "nan-y-R3", "huge-y-3030")


def _both(base):
    return [dict(c, name=f"{c['name']}-form{form}", form=form, base=c["name"]) for c in base for form in (0, 1)]


def size_cases():
    return _both([lc._c(f"series-n{n}", n=n, T=6, expect=dict(clamped_last=(n == 1), nan_steps=())) for n in SIZES])


def schedule_cases():
    c = [lc._c(f"series-rs{rs}", n=700, T=7, rs=rs, expect=dict(no_draw_steps=tuple(t for t in range(1, 7) if t % rs), nan_steps=()))
         for rs in (2, 3)]
    c += [lc._c(f"series-T{T}", n=700, T=T, expect=dict(nan_steps=())) for T in (1, 2)]
    return _both(c)


def degenerate_cases():
    by = {c["name"]: c for c in lc.base_cases()}
    out = _both([by[name] for name in DEGENERATE])
    for c in out:
        assert c["n"] == 700 and c["T"] == 5
    return out


def handover_cases():
    """8 steps: a series of 5, then 3 calls of the step API.  rs = 2 carries the second-stage log-weights across the hand-over
    (step 5 does not resample)."""
    return _both([lc._c(f"series-handover-rs{rs}", n=700, T=8, rs=rs, expect=dict(nan_steps=())) for rs in (1, 2)])


def all_cases():
    return size_cases() + schedule_cases() + degenerate_cases() + handover_cases()


LONG_N, LONG_T = 500, 300                      # the first 300 rows of spy_returns.csv, z its lag
BANK_N, BANK_R, BANK_T = 500, 100, 16
BANK_ORACLE_REPS = (0, 1, 99)
