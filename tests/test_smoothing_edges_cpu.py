"""What tests/smooth_edge_cases.py states about its routes and degenerate series, derived without a device: the route table against
bs_edge_cases.route_of, and for every degenerate series the CPU oracle's own run -- which filters end without weight, from which step
the populations are NaN, before which step every lineage is one particle, and that the final weights have a tile scale of zero."""
import numpy as np
import pytest

import bs_edge_cases as bc
import expect_ref as er
import smooth_edge_cases as ec
import smooth_ref as sr


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build()
    return O


def test_route_table_is_route_of():
    assert set(ec.ROUTE_TABLE) == set(ec.LINEAGE_ROUTES)
    for name, want in ec.ROUTE_TABLE.items():
        for sched in (1, 2):
            case = ec.route_case(sched)
            assert bc.route_of(case, ec.BS_ROUTES[name], "general", 0) == want, name
            assert bc.shape(case, ec.BS_ROUTES[name])[:3] == (ec.ROUTES[name][0], want[3], ec.ROUTE_TILES[name]), name
    # what the list is for: tiles of 1024 and 2048, the block-wide level-2, the forced split and the tables at 5 tiles, the split by size
    t = ec.ROUTE_TABLE
    assert t["wl2-1024"][3] == 1024 and t["wl2-1024"][5] and not t["inkernel-129"][5] and not t["inkernel-129"][2]
    assert t["split-forced-5"][2] and t["tables-5"][2] and t["tables-5"][6] == "k_level2_plan" and ec.ROUTES["split-1025"][3] is None
    assert ec.ROUTE_TILES["split-1025"] > bc.SPLIT_ABOVE_TILES and ec.ROUTE_TILES["inkernel-129"] > bc.WL2_MAX_TILES
    assert set(ec.SMOOTHED_ROUTES) <= set(ec.ROUTES) and ec.steps_of("split-1025") == 3


@pytest.mark.parametrize("route", ec.DEGENERATE_ROUTES)
@pytest.mark.parametrize("case", ec.DEGENERATE, ids=[c["name"] for c in ec.DEGENERATE])
def test_degenerate_series_are_what_the_list_says(oracle, case, route):
    n, tile, _, _ = ec.ROUTES[route]
    tile = tile or 2048
    y, z = ec.series(case)
    assert len(y) == case["T"]
    for r in range(case["R"]):
        of = oracle.Filter(case["model"], n, np.asarray(case["theta"][r], dtype=np.float64), ec.sc.SEED, rep=r, resampler=0,
                           resamp_sched=case["sched"], tile=tile)
        xs, ancs = [], []
        for t in range(case["T"]):
            of.step(y[t], 0.0 if z is None else z[t])
            st = of.state()
            xs.append(np.asarray(st["x"]).copy())
            ancs.append(np.asarray(st["anc"]).copy())
        dead = not (st["S"] > 0) or bc.no_weight_left(st)
        assert dead == (r in case["dead"]), (case["name"], r)
        first_nan = next((t for t in range(case["T"]) if np.isnan(xs[t]).any()), None)
        assert first_nan == case["x_nan_from"], (case["name"], r, first_nan)
        if first_nan is not None:
            assert all(np.isnan(xs[t]).all() for t in range(first_nan, case["T"]))
        B = sr.genealogy(ancs, case["sched"])
        if case["coalesced_before"] is not None:
            s = case["coalesced_before"]
            assert sr.resampled(s, case["sched"])
            assert all(len(np.unique(B[t])) == 1 for t in range(s)), (case["name"], r)
            assert len(np.unique(B[s])) > 1
        if case["zero_scale"] and tile < n:
            e = er.make_state(oracle, st, tile, n)
            zero = (e["s"] == 0.0) & (np.asarray(e["A"]) > 0)
            assert zero.any() and not zero.all(), (case["name"], r, e["s"])
    assert ec.checked_triples(case) == (case["R"] - len(case["dead"])) * 7 * 4
