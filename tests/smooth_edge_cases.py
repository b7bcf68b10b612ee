"""The routes and inputs at which tests/test_smoothing_edges_gpu.py pins the smoothing calls beyond tests/test_smoothing_gpu.py: the
level-2 routes of the tiled step that had never recorded a history (the route table and route_of of bs_edge_cases.py), and
degenerate series.  Everything a case expects is stated here, before any device run; test_smoothing_edges_cpu.py derives the same
facts from the CPU oracle (which filters end without weight, where the populations turn NaN, where the lineages coalesce).

A recording series sends k_filter_step to its general instantiation (ancestors are written, RS = -1), so the routes are asserted in
route_of's form "general"."""
import numpy as np

import bs_edge_cases as bc
import series_expect_cases as sc

T = 7
NAN = float("nan")
BS_ROUTES = {r["name"]: r for r in bc.routes()}
# (N, tile_particles, set_small_series, split_level2) by name: the six shapes of test_smoothing_gpu.py and the level-2 routes of bs_edge_cases.py
ROUTES = {
    "lane-500": (500, 0, True, None), "pair-1030": (1030, 0, True, None), "tiled-1027-t512": (1027, 512, True, None),
    "tiled-4100-t2048": (4100, 2048, True, None),
}
for _n in ("wl2-1024", "wl2-2048", "inkernel-129", "split-forced-5", "tables-5", "split-1025"):
    _r = BS_ROUTES[_n]
    ROUTES[_n] = (_r["n"], _r["tile"], _r["small"], _r["split"])

# route_of(case, route, "general", resampler 0) written out by hand: (kernel, threads, BIG = split level-2, tile, RS, WL2, level-2)
ROUTE_TABLE = {
    "wl2-1024": ("k_filter_step", 512, False, 1024, -1, True, "wave-by-wave in k_filter_step + fused accounting (ticket)"),
    "wl2-2048": ("k_filter_step", 512, False, 2048, -1, True, "wave-by-wave in k_filter_step + fused accounting (ticket)"),
    "inkernel-129": ("k_filter_step", 256, False, 512, -1, False, "level2_scan in k_filter_step + fused accounting (ticket)"),
    "split-forced-5": ("k_filter_step", 256, True, 512, -1, False, "k_l2_scan_blocks x1 (l2_inkernel), ranges in k_filter_step"),
    "tables-5": ("k_filter_step", 256, True, 512, -1, False, "k_level2_plan"),
    "split-1025": ("k_filter_step", 256, True, 512, -1, False, "k_l2_scan_blocks x2 (l2_inkernel), ranges in k_filter_step"),
}
ROUTE_TILES = {"wl2-1024": 4, "wl2-2048": 4, "inkernel-129": 129, "split-forced-5": 5, "tables-5": 5, "split-1025": 1025}

SMOOTHED_ROUTES = ("pair-1030", "wl2-1024", "tiled-4100-t2048", "inkernel-129")
LINEAGE_ROUTES = ("wl2-1024", "wl2-2048", "inkernel-129", "split-forced-5", "tables-5", "split-1025")
TH2 = sc.TH_SVOL3[:2]


def route_case(sched, R=2):
    """The (case) argument of bs_edge_cases.route_of / shape for a recording run."""
    return dict(R=R, T=T, sched=sched)


def steps_of(route):
    return 3 if route == "split-1025" else T


# ---- degenerate series -------------------------------------------------------------------------------------------------------------
# dead: the filters whose FINAL weights are all zero / NaN (S' = 0): NaN states from sample_trajectories, NaN in every smoothed row.
# x_nan_from: the populations are NaN from that step on.  coalesced_before: every lineage is ONE particle at all rows < that step
# (the draw of that step read a cdf of zeros, which resolves every target to index 0, or one particle held all the weight).
# zero_scale: in the final weights some tile's scale e^(m_b - m) is exactly zero while the tile has q > 0 (tiled route only).
# A live filter has no NaN row: its smoothed rows are finite everywhere.
def _d(name, model, theta, sched=1, y=None, y_set=None, z_set=None, dead=(), x_nan_from=None, coalesced_before=None, zero_scale=False):
    return dict(name=name, model=model, theta=theta, R=2, T=T, sched=sched, y=y, y_set=y_set or {}, z_set=z_set or {}, dead=tuple(dead),
                x_nan_from=x_nan_from, coalesced_before=coalesced_before, zero_scale=zero_scale)


TH_LG2 = (bc.TH_LG, (0.6, 0.1, 0.01))
DEGENERATE = (
    # a NaN observation at t = 2: the weights of step 2 are NaN, the draw of step 3 takes every ancestor from a cdf of zeros
    _d("nan-y", sc.MODEL_SVOL, TH2, y_set={2: NAN}, coalesced_before=3),
    # schedule 3 (draws at t = 3, 6), NaN at t = 4: carried through t = 5, the draw of t = 6 reads zeros
    _d("nan-sched3-carried", sc.MODEL_SVOL, TH2, sched=3, y_set={4: NAN}, coalesced_before=6),
    # an observation of 1000 at t = 2: one particle holds all the weight of step 2, every lineage passes through it
    _d("huge-y", sc.MODEL_SVOL, TH2, y_set={2: 1e3}, coalesced_before=3),
    # a NaN covariate at t = 2 (leverage model): NaN states from row 2 on, no filter has weight at the end; every draw from t = 3 on
    # reads a cdf of zeros, the last of them at t = 6
    _d("nan-z", sc.MODEL_SVOL_LEVERAGE, sc.TH_LEV3[:2], z_set={2: NAN}, dead=(0, 1), x_nan_from=2, coalesced_before=6),
    # linear Gaussian model with tau = 0.01 and a final observation far out: tile maxima more than 746 apart in the FINAL weights
    _d("zero-tile", sc.MODEL_LIN_GAUSS, TH_LG2, y=(0.3, 0.31, -0.2, 0.25, 0.1, 0.05, 3.0), zero_scale=True),
    # the series ends on a NaN: every filter dead
    _d("ends-on-nan", sc.MODEL_SVOL, TH2, y_set={T - 1: NAN}, dead=(0, 1)),
)
DEGENERATE_ROUTES = ("lane-500", "tiled-1027-t512")


def series(case):
    """(y [T], z [T] or None): spy_returns.csv[:T] or the case's own y, with y_set / z_set applied (bs_edge_cases.series)."""
    return bc.series(case)


def checked_triples(case):
    """(filter, row, functional) triples of the rational check: every live filter, every row, four functionals."""
    return (case["R"] - len(case["dead"])) * case["T"] * 4
