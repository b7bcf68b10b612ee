"""The lists of tests/vector_series_cases.py through the oracle alone (no GPU): every degenerate case reaches what its `expect` says at
the two shapes of the whole-series kernels, and the listed sizes sit on both sides of every switch of the route.  The proof of a case
is test_user_edges_cpu._prove and the closures are user_edge_cases' / oracle_models' (imported, not copied).
test_vector_series_gpu.py then asks the device for the oracle's bits on the same lists."""
import numpy as np
import pytest

import user_edge_cases as uc
import vector_series_cases as vc
from test_user_edges_cpu import _prove


@pytest.mark.parametrize("item", vc.edge_items(), ids=lambda it: f"{it[0]}-{it[1]['name']}-n{it[2]}")
def test_degenerate_case_reaches_what_its_expect_says(oracle, item):
    lib, case, n = item
    header = vc.LIBS[lib]["edge"]
    for rs in vc.EDGE_RESAMPLERS if n == vc.EDGE_SHAPES[0] else (0,):
        _prove(oracle, header, case, vc.edge_route(n), rs)
    uc.forget_runs()


def test_edge_cases_are_the_listed_ones():
    for lib, names in vc.EDGE_CASES.items():
        have = {c["name"] for c in uc.cases(vc.LIBS[lib]["edge"])}
        assert set(names) <= have, (lib, set(names) - have)
        assert any(uc.case_of(vc.LIBS[lib]["edge"], n)["clean_tail"] for n in names) == (lib == "svol_two_factor_cov")
    # plane 1 NaN from step 0 while plane 0 stays finite
    assert uc.case_of("svol_two_factor_cov", "nan-z3-first")["expect"]["x1_nan_from"] == 0
    assert {vc.expected_route(n)[0] for n in vc.EDGE_SHAPES} == {vc.ROUTE_SERIES_LANE, vc.ROUTE_SERIES_PAIR}


def test_sizes_sit_on_both_sides_of_every_switch():
    for s in vc.SWITCHES:
        assert s in vc.SIZES and s + 1 in vc.SIZES, s
    shape = lambda n: vc.expected_route(n) + (0 if n <= 512 else (1 if n <= 1024 else 2),)       # (route, threads, pairs per lane)
    for s in vc.SWITCHES:
        assert shape(s) != shape(s + 1), s
    assert len({shape(n) for n in vc.SIZES}) == 6 == len(vc.SWITCHES) + 1
    assert 2047 in vc.SIZES and 2048 in vc.SIZES and vc.expected_route(2049)[0] == vc.ROUTE_TILED
    assert vc.expected_route(500, tile=512)[0] == vc.ROUTE_TILED
    assert 1 in vc.SIZES and 2 in vc.SIZES                                # half a pair, one pair
    # the oracle-compared subset: the lane kernel at its smallest, a middle and its largest block, and the pair kernel (two pairs per
    # lane, just above the switch and at the last one-tile size); one pair per lane reaches the oracle through the tiled kernel's bits
    assert {shape(n) for n in vc.ORACLE_SIZES} == {shape(1), shape(128), shape(512), shape(2048)}
    assert set(vc.ORACLE_SIZES) <= set(vc.SIZES) and set(vc.ORACLE_RESAMPLERS) <= set(vc.RESAMPLERS)
    for lib, s in vc.LIBS.items():
        assert len(s["theta"]) == vc.R == len({tuple(t) for t in s["theta"]}), "different rows in every filter"
        assert s["dx"] > 1 or s["dy"] > 1
    assert {s["dx"] for s in vc.LIBS.values()} == {2, 3, 4}
    c = vc.LONG
    assert -(-c["T"] // 64) == 5 and c["then"] == (40, c["T"])


def test_healthy_series_are_finite_and_filters_differ(oracle):
    """The healthy series of every library at N = 65 (schedule 3: carried weights): finite terms, and three different filters."""
    for lib in vc.LIBS:
        per, sts = vc.oracle_series(oracle, lib, 65, 0, 3)
        assert per.shape == (vc.R, vc.T) and np.isfinite(per).all(), lib
        assert len({per[r].tobytes() for r in range(vc.R)}) == vc.R, lib
        for r in range(vc.R):
            assert sts[r]["x"].shape == (vc.LIBS[lib]["dx"], 65) and np.isfinite(sts[r]["x"]).all(), lib
            assert len({sts[r]["x"][d].tobytes() for d in range(vc.LIBS[lib]["dx"])}) == vc.LIBS[lib]["dx"], "planes differ"
