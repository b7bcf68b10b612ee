"""The case and layout lists of tests/shard_edge_cases.py through the oracle alone (no GPU): every (case, layout) pair reaches what it is
listed for -- the collapse to particle 0 that needs tile 0 on every rank, the reach of exactly `margin` and `margin + 1` tiles, the rank
of one particle, the rank whose whole share has a rescaled tile sum of zero -- and `expect` (shard_edge_cases.MUST_LEAVE: the steps and
ranks whose needed reach exceeds the halo margin) is what the oracle's ancestors give, no pair more and no pair less."""
import numpy as np
import pytest

import bs_edge_cases as bc
import shard_edge_cases as sc

PAIRS = sc.pairs()


def _pid(p):
    return f"{p[0]['name']}@{p[1]['name']}"


def test_pairs_cover_every_layout_and_every_case():
    assert {l["name"] for _, l in PAIRS} == set(sc.LAYOUTS) and len(sc.LAYOUTS) == 8
    assert {c["name"] for c, _ in PAIRS} == set(sc.CASES)
    want = {"nan-y", "inf-y", "huge-y", "zero-tile", "neg-huge-y", "zeros-y", "nan-z", "nan-sched3-carried", "nan-sched3-resampling",
            "bad-theta-phi-1", "bad-theta-sigma0-1", "bad-theta-beta-1"}
    assert set(sc.CASES) == want
    assert [c["name"] for c, l in PAIRS if l["name"] == "split-l2"] == ["nan-y", "huge-y"]
    for g in sc.GUARD_CASES:
        assert {l["name"] for c, l in PAIRS if c["name"] == g} >= set(sc.LAYOUTS) - {"split-l2"}
    runs = sc.runs()
    assert len({sc.run_id(r) for r in runs}) == len(runs)
    assert {r[2] for r in runs} == set(sc.RESAMPLERS) and {r[3] for r in runs} == {0, 1, 2}
    assert all(not (rs == sc.IID and mode == 1) for _, _, rs, mode in runs)      # rejected: asserted on its own in the GPU module
    for l in sc.layouts():                                                        # every layout sees every mode and a collapse in each
        assert {r[3] for r in runs if r[1]["name"] == l["name"] and r[0]["name"] == "nan-y"} == {0, 1, 2}
    assert bc.cases()[0]["name"] == "nan-y" and len(bc.cases()) == 14             # bs_edge_cases' own lists are as they were
    assert len(bc.routes()) == 22 and len(bc.pairs()) == 103


def test_layouts_are_the_shapes_they_are_listed_for():
    sh = {k: sc.shares(l["n"], l["world"]) for k, l in sc.LAYOUTS.items()}
    mg = {k: sc.halo_margin(sh[k][1], l["world"]) for k, l in sc.LAYOUTS.items()}
    assert sh["4x2"][:3] == (8, 2, [2, 2, 2, 2]) and mg["4x2"] == 2
    assert sh["4r-ragged"][:3] == (7, 2, [2, 2, 2, 1]) and sh["4r-ragged"][3] == [4096, 4096, 4096, 2048 - 700] and mg["4r-ragged"] == 2
    assert sh["3x1"][:3] == (3, 1, [1, 1, 1]) and mg["3x1"] == 1
    assert sh["2r-one-particle"] == (2, 1, [1, 1], [2048, 1]) and mg["2r-one-particle"] == 1
    assert sh["1r"] == (4, 4, [4], [3 * 2048 + 77]) and mg["1r"] == 0
    assert sh["2xBl4"][:2] == (8, 4) and mg["2xBl4"] == 4
    assert sh["2xBl5"][:2] == (10, 5) and mg["2xBl5"] == 4
    assert sh["split-l2"][:3] == (1026, 513, [513, 513]) and sh["split-l2"][3] == [513 * 2048, 512 * 2048 + 1] and mg["split-l2"] == 8
    assert sh["split-l2"][0] > bc.SPLIT_ABOVE_TILES                          # set_layout: split_l2 = B > kSplitLevel2Above
    assert all(sh[k][0] <= bc.SPLIT_ABOVE_TILES for k in sh if k != "split-l2")
    assert sc.shares(5 * 2048, 4) is None and sc.shares(4 * 2048, 3) is None  # Bl = 2: the last rank would own nothing
    assert sc.halo_margin(64 * 9, 2) == 9 and sc.halo_margin(3, 2) == 3 and sc.halo_margin(300, 1) == 0
    assert sc.shape(sc.CASES["nan-y"], sc.LAYOUTS["split-l2"]) == (1025 * 2048 + 1, 4)


@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_pair_reaches_what_it_is_listed_for(oracle, pair):
    case, layout = pair
    n, T = sc.shape(case, layout)
    world = layout["world"]
    B, Bl, own, parts = sc.shares(n, world)
    margin = sc.halo_margin(Bl, world)
    e = case["expect"]
    for rs in sc.SORTED:
        run = sc.oracle_run(oracle, case, layout, rs)
        got, widest = sc.must_leave_from_oracle(oracle, case, layout, rs)
        assert tuple(got) == sc.must_leave(case, layout, rs), (rs, got, widest)
        nan_steps = [t for t in range(T) if np.isnan(run[t][0][0])]
        assert nan_steps == [t for t in e.get("nan_steps", ()) if t < T], (rs, nan_steps)
        for t in e.get("collapsed_at", ()):
            if t >= T:
                continue
            anc = run[t][1][0]["anc"]
            assert not anc.any(), (rs, t)                                      # every ancestor is particle 0 ...
            need = sc.needed(anc, layout)
            assert all(nd[:2] == (0, 0) for nd in need)                        # ... so every rank needs tile 0 and nothing else
            assert [nd[2] for nd in need] == [r * Bl for r in range(world)]
            assert [(t, r) for r in range(world) if r * Bl > margin] == [p for p in got if p[0] == t]
            if layout["name"] == "2xBl4":
                assert need[1][2] == 4 == margin                               # reach = margin: the halo holds the collapse
            if layout["name"] == "2xBl5":
                assert need[1][2] == 5 == margin + 1                           # reach = margin + 1: it cannot
        if case["name"] == "zero-tile" and world > 1:
            # after step 1 some rank's WHOLE share has rescaled tile sums of zero: its gathered entries are zeros among others' weights
            Ap = np.asarray(bc.rescaled_sums(oracle, run[1][1][0]))
            dead = [r for r in range(world) if not Ap[r * Bl:r * Bl + own[r]].any()]
            assert dead and len(dead) < world, (rs, Ap)
        if case["name"] == "bad-theta-sigma0-1":
            assert not run[T - 1][1][0]["x"].any()
    if layout["name"] == "2r-one-particle":
        assert parts == [2048, 1]
    if case["name"] == "nan-y":
        assert 3 in e["collapsed_at"] and T > 3                                # the collapse is inside every layout's series


@pytest.mark.parametrize("cname", list(sc.LW_CASES))
@pytest.mark.parametrize("lname", sc.LW_LAYOUTS)
def test_liu_west_cases_reach_their_step(oracle, cname, lname):
    """The Liu-West side: the NaN steps, and where the oracle proves that a window leaves the halo (SSME_ERR_STATE is then required)."""
    case, layout = sc.LW_CASES[cname], sc.LAYOUTS[lname]
    for form in (0, 1):
        run = sc.lw_oracle_run(oracle, case, layout, form)
        nan = [t for t in range(sc.LW_T) if np.isnan(run[t][0])]
        assert nan == {"nan-y": [2], "inf-y": [2], "huge-y": [], "nan-z": [2, 3, 4]}[cname]
        must = sc.lw_must_leave(oracle, case, layout, form)
        if cname != "huge-y":
            assert not np.asarray(run[3][1]["anc"]).any()                      # step 3 resamples from zeros: particle 0
            assert must == (lname != "2r-one-particle")                        # tile 0 is within the margin of both ranks there
        else:
            assert not must                                                    # the path of huge-y is an observation


def test_python_driver_pairs_reach_both_routes(oracle):
    """The pairs of test_shard_edges_gpu.py's Python-driver tests (nan-y and huge-y on shard_edge_cases.py_layout, Bl = 2) reach both
    routes of _ShardedFilter._windows.  World 2: B - Bl = 2 is within the margin, so every window fits and every draw is in place.
    World 4 (the layout 4x2 itself): must_leave is non-empty for both bootstrap cases -- test_pair_reaches_what_it_is_listed_for holds
    it to the oracle's ancestors exactly -- and the Liu-West resampling draw of nan-y's step 3 needs tile 0 on ranks 2 and 3; the
    Liu-West huge-y proves nothing (its route is an observation)."""
    for world in (2, 4):
        B, Bl, own, parts = sc.shares(sc.py_layout(world)["n"], world)
        assert (B, Bl) == (2 * world, 2) and sc.py_margin(B, Bl, world) == 2 == sc.halo_margin(Bl, world)
    assert sc.py_margin(8 * 64, 64, 8) == 32 and sc.py_margin(3, 1, 3) == 2 and sc.py_margin(2, 1, 2) == 1 and sc.py_margin(4, 4, 1) == 0
    B, Bl, own, parts = sc.shares(sc.py_layout(2)["n"], 2)
    assert B - Bl <= sc.py_margin(B, Bl, 2)
    layout = sc.py_layout(4)
    assert layout == sc.LAYOUTS["4x2"]
    for cname, want in (("nan-y", ((3, 2), (3, 3))), ("huge-y", ((3, 0), (3, 1)))):
        case = sc.CASES[cname]
        assert sc.must_leave(case, layout, 0) == want == tuple(sc.must_leave_from_oracle(oracle, case, layout, 0)[0])
        assert sc.shape(case, layout)[1] > 3                                   # step 3 is inside the series
    assert 3 in sc.lw_must_leave_steps(oracle, sc.LW_CASES["nan-y"], layout, 0) and sc.LW_T > 3
    assert sc.lw_must_leave_steps(oracle, sc.LW_CASES["huge-y"], layout, 0) == []
