"""The lists of tests/lifecycle_cases.py, without a GPU: every hazard scenario contains what it claims (from the events the host model
predicts), the walks cover every ordered pair of state-changing op classes with a reader between the two and never leave the contract,
every expected value is computable from the oracle and finite, the model's bookkeeping equals a table written out by hand for three
short sequences, and profiles/lifecycle_paths.txt is what the lists say today.  The module prints the time the memoised oracle
evaluation of all runs took (`-s`, or the captured output of test_oracle_time_is_printed)."""
import os
import time

import numpy as np
import pytest

import bs_edge_cases as bc
import lifecycle_cases as L

RUNS = L.all_runs()
_TIME = {"oracle_s": 0.0, "runs": 0}


@pytest.fixture(scope="module")
def memo(oracle):
    return L.OracleMemo(oracle)


def _events(hazard):
    """{shape name: [(op index, op, events)]} of a hazard's scenarios."""
    return {n: [(i, op, ev) for i, (op, ev) in enumerate(L.trace(n, ops))] for h, n, ops in L.scenarios() if h == hazard}


def test_shapes_are_the_routes_they_are_named_for():
    s, routes = L.SHAPES, {r["name"]: r for r in bc.routes()}
    case = dict(R=1, sched=1, T=6)
    assert bc.route_of(dict(case, R=3), routes["small-100"], "hot", 0)[0] == "k_filter_series_lane<128>" and s["small-100"]["n"] == 100
    assert bc.route_of(dict(case, R=2), bc._r("pair", "small", 1500), "hot", 1)[0] == "k_filter_series_small<512,2>" and s["pair-1500"]["B"] == 1
    for name in ("wl2-512", "split-1025"):
        assert (s[name]["n"], s[name]["tile"]) == (routes[name]["n"], routes[name]["tile"])
    assert s["split-1025"]["B"] == 1025 and s["split-1025"]["tmax"] <= 6
    for name in ("tiles5-2048", "split-forced-5", "tables-5"):
        assert (s[name]["B"], s[name]["tile"], s[name]["n"]) == (5, 2048, s["tiles5-2048"]["n"])
    assert (s["split-forced-5"]["split"], s["tables-5"]["split"]) == (True, "tables")
    bs = [x for x in s.values() if x["kind"] == "bs"]
    assert {(x["sched"], x["rs"]) for x in bs} >= {(3, 0), (3, 1), (1, 0), (1, 1)} and sum(x["f32"] for x in bs) == 1
    assert {x["model"] for x in bs} == {L.SVOL, L.LEV} and {x["R"] for x in bs} == {1, 2, 3}
    lw = [x for x in s.values() if x["kind"] == "lw"]
    assert {x["n"] for x in lw} == {300, 3 * 2048 + 5}
    for n in (300, 3 * 2048 + 5):
        assert {k: {x[k] for x in lw if x["n"] == n} for k in ("form", "rs", "split")} == dict(form={0, 1}, rs={1, 3}, split={None, True})


def test_h1_has_a_recapture_and_a_replay_for_every_key_field_and_every_drop():
    ev = _events("H1")
    assert ev
    pure = set()
    for name, tr in ev.items():
        series = [e for _, op, e in tr if op[0] == "series"]
        assert any("replay" in e for e in series) and any(x.startswith("recapture") for e in series for x in e), name
        for a, b in zip(series, series[1:]):
            for x in a:
                if x.startswith("recapture:") and x[10:] in L.KEY_FIELDS and "replay" in b:
                    pure.add(x[10:])        # one field alone differed, and the next series replayed the new graph
    assert pure == set(L.KEY_FIELDS), pure
    drops = {x for tr in ev.values() for _, _, e in tr for x in e if x.startswith("drop:")}
    assert drops == {"drop:set_debug policy", "drop:set_stream", "drop:series buffers moved", "drop:gamma moved"}
    forms = {x for tr in ev.values() for _, _, e in tr for x in e if x.startswith("series:")}
    assert {f.split(":")[1] for f in forms} == {"graph", "eager"}
    # the larger T comes before the first replay of a shorter one: a stale longer graph stays inside ycap / tcap
    for name, tr in ev.items():
        Ts = [op[1] for _, op, _ in tr if op[0] == "series"]
        assert Ts[:4] == [6, 130, 6, 6] and max(Ts) == 130


def test_h2_raises_each_capacity_by_a_different_call():
    for name, tr in _events("H2").items():
        m = L.HandleModel(L.SHAPES[name])
        grow = {k: [i for i, _, e in tr if "regrow:" + k in e] for k in ("ybuf", "per_step", "gamma")}
        assert grow["per_step"] and grow["ybuf"], name
        if m.mult:
            first = grow["gamma"][0]
            assert tr[first][1][0] in ("step", "lw_filter") and first not in grow["per_step"], name     # gcap -> 64 while tcap = 1
            assert any(i not in grow["gamma"] for i in grow["per_step"]), name                          # T = 5: tcap alone
            assert any(i in grow["gamma"] for i in grow["per_step"]), name                              # T = 65: both
        alloc = [i for i, _, e in tr if "alloc:anc" in e]
        assert len(alloc) == 1 and tr[alloc[0] + 1][1][:2] == ("read", "state_idx" if m.lw else "state_anc"), name
        if not m.lw:
            assert tr[alloc[0] - 1][1][0] == "step_queued", name                                        # behind steps nobody waited for
        reads = [(i, op) for i, op, _ in tr if op[:2] == ("read", "per_step")]
        assert any(op[2] == 5 and i > max(grow["per_step"]) for i, op in reads), name                   # per_step(5) after tcap = 130


def test_h3_runs_without_covariates_after_a_longer_series_with_them():
    ev = _events("H3")
    assert {L.SHAPES[n]["kind"] for n in ev} == {"bs", "lw"}
    for name, tr in ev.items():
        ser = [op for _, op, _ in tr if op[0] in ("series", "lw_series")]
        assert ser[0][1] == 130 and ser[0][3] and ser[1][1] == 6 and not ser[1][3], name


def test_h4_redraws_the_chunk_for_each_trigger():
    ev = _events("H4")
    assert {L.SHAPES[n]["kind"] for n in ev} == {"bs", "lw"}
    for name, tr in ev.items():
        causes = [x[7:] for _, _, e in tr for x in e if x.startswith("redraw:")]
        lw = L.SHAPES[name]["kind"] == "lw"
        assert set(causes) == ({"first", "chunk-end", "reset", "series"} if lw else {"set_params", "chunk-end", "set_seed", "reset", "series"}), (name, causes)
        assert causes.count("series") >= 3 and causes.count("chunk-end") >= 2, name     # after T < 64, after T > 64, steps - series - steps
        m, at = L.HandleModel(L.SHAPES[name]), []
        for _, op, e in tr:
            t0 = m.t
            m.apply(op)
            if any(x == "redraw:series" for x in e):
                at.append(t0)
        assert 5 in at and 65 in at, name                                                # steps continue at t = T


def test_h5_has_both_parities_on_every_launch_form():
    for name, tr in _events("H5").items():
        s = L.SHAPES[name]
        got = {x for _, _, e in tr for x in e if x.startswith("series:")}
        forms = ("eager",) if s["kind"] == "lw" else (("small", "graph", "eager") if s["B"] == 1 else ("graph", "eager"))
        assert got == {f"series:{f}:{p}" for f in forms for p in ("odd", "even")}, (name, got)
    lw = [tr for n, tr in _events("H5").items() if L.SHAPES[n]["kind"] == "lw"]
    assert lw and all(tr[0][1][:2] == ("lw_filter", 3) for tr in lw)                    # an odd number of filter calls first


def test_h6_h7_h8_contain_what_they_claim():
    for name, tr in _events("H6").items():
        ops = [op for _, op, _ in tr]
        behind = {b[1] for a, b in zip(ops, ops[1:]) if a[0] == "step_queued" and b[0] == "read"}
        assert behind == {"loglik", "per_step", "state", "expectations_multi", "weights", "sim_future_obs", "swarm_aggregate", "log_mean_exp"}, name
        assert any(a[0] == "step_queued" and b[0] == "set_seed" for a, b in zip(ops, ops[1:])), name
    for name, tr in _events("H7").items():
        assert [op[1] for _, op, _ in tr if op[0] == "set_params"] == ["one", "rows", "one", "second"], name
    for name, tr in _events("H8").items():
        ops = [op for _, op, _ in tr]
        steps = [i for i, op in enumerate(ops) if op[0] in ("step", "lw_filter")]
        assert all(any(o[0] == "refused" for o in ops[a + 1:b]) for a, b in zip(steps[:5], steps[1:6])), name
        want = L.LW_REFUSED if L.SHAPES[name]["kind"] == "lw" else L.REFUSED
        assert {op[1] for op in ops if op[0] == "refused"} == set(want), name


def test_h9_plan():
    plan = L.churn_plan()
    assert len(plan) == 40 and {p[0] for p in plan} == set(L.CHURN_SHAPES) and len(L.CHURN_SHAPES) == 4
    assert all(sum(p[0] == c for p in plan) >= 5 for c in L.CHURN_SHAPES) and max(p[2] for p in plan) == 2


def test_walks_cover_every_ordered_pair_with_a_reader_between():
    """Counted again from the op lists, independently of the generator's own bookkeeping: 100 %, a condition and not a measurement."""
    runs, cov = L.walks()
    assert not L.missing_pairs(cov)
    seen = {"bs": set(), "lw": set()}
    for name, _, ops in runs:
        m, prev, reader = L.HandleModel(L.SHAPES[name]), None, False
        for op in ops:
            if op[0] == "read":
                reader = True
            elif op[0] != "refused":
                if prev is not None and reader:
                    seen[L.SHAPES[name]["kind"]].add((prev, m.op_class(op)))
                prev, reader = m.op_class(op), False
    assert seen["bs"] == {(a, b) for a in L.BS_CLASSES for b in L.BS_CLASSES}
    assert seen["lw"] == {(a, b) for a in L.LW_CLASSES for b in L.LW_CLASSES}
    assert len(runs) >= 2 * len(L.SHAPES) and all(len(ops) >= L.SHAPES[n]["walk_ops"] for n, _, ops in runs)
    assert {T for n, _, ops in runs for op in ops if op[0] in ("series", "lw_series") for T in (op[1],)} == set(L.SERIES_T)
    assert L.walks()[0] == runs and L.walk(L.SHAPES["wl2-512"], 0, {}) == L.walk(L.SHAPES["wl2-512"], 0, {})      # fixed seeds


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_run_stays_in_the_contract_and_every_expected_value_is_finite(memo, run):
    rid, name, ops = run
    s = L.SHAPES[name]
    m = L.HandleModel(s)
    t0 = time.perf_counter()
    for i, op in enumerate(ops):
        assert m.legal(op), (rid, i, op)
        if op[0] in ("step", "step_queued", "reset", "series"):
            assert m.theta is not None                   # nothing steps before set_params
        if op[0] in ("series", "lw_series"):
            assert op[1] in L.SERIES_T and op[1] <= s["tmax"]
        m.apply(op)
        if op[0] in ("read", "refused") or not m.hist:
            continue
        res = memo.of(m)
        assert res["lls"].shape == (s["R"], m.t) and np.isfinite(res["lls"]).all(), (rid, i, op)
        for st in res["states"]:
            assert np.isfinite(st["x"]).all() and (st["S"] > 0 if "cdf" in st else np.isfinite(st["theta"]).all()), (rid, i, op)
        if m.series_rec is not None:
            assert np.isfinite(memo.per_step(m)).all()
    _TIME["oracle_s"] += time.perf_counter() - t0
    _TIME["runs"] += 1


def test_oracle_time_is_printed():
    print(f"LIFECYCLE memoised oracle evaluation of {_TIME['runs']} runs: {_TIME['oracle_s']:.1f} s")
    assert _TIME["runs"] in (0, len(RUNS))               # 0: this test was selected alone


HAND = {
    # (shape, [(op, (t, len(hist), ycap, tcap, gcap, gamma_t0, gamma_rows), events)]) written out from pf_api.hip by hand
    "wl2-512": [
        (("set_params", "one"), (0, 0, 1, 1, 1, 0, 0), []),
        (("step", 2, 0, True), (2, 2, 1, 1, 64, 0, 64), ["regrow:gamma", "redraw:set_params"]),
        (("series", 5, 0, True), (5, 5, 5, 5, 64, 0, 0), ["regrow:ybuf", "regrow:per_step", "recapture:no graph", "series:graph:odd"]),
        (("step", 1, 2, True), (6, 6, 5, 5, 64, 5, 64), ["redraw:series"]),
        (("set_seed", 9), (0, 0, 5, 5, 64, 5, 0), []),
        (("step", 1, 3, False), (1, 1, 5, 5, 64, 0, 64), ["redraw:set_seed"]),
    ],
    "small-100": [
        (("set_params", "rows"), (0, 0, 1, 1, 1, 0, 0), []),
        (("series", 6, 0, False), (6, 6, 6, 6, 6, 0, 0), ["regrow:ybuf", "regrow:per_step", "regrow:gamma", "series:small:even"]),
        (("set_small_series", False), (6, 6, 6, 6, 6, 0, 0), []),
        (("series", 6, 1, False), (6, 6, 6, 6, 6, 0, 0), ["recapture:no graph", "series:graph:even"]),
        (("series", 6, 2, False), (6, 6, 6, 6, 6, 0, 0), ["replay", "series:graph:even"]),
        (("set_stream", True), (6, 6, 6, 6, 6, 0, 0), ["drop:set_stream"]),
        (("series", 5, 2, False), (5, 5, 6, 6, 6, 0, 0), ["recapture:no graph", "series:graph:odd"]),
        (("set_tuning", 1024), (5, 5, 6, 6, 6, 0, 0), []),
        (("series", 5, 2, False), (5, 5, 6, 6, 6, 0, 0), ["recapture:nt", "series:graph:odd"]),
    ],
    "lw-300-form0-rs1": [
        (("lw_filter", 2, 0), (2, 2, 1, 1, 64, 1, 64), ["regrow:gamma", "redraw:first"]),
        (("lw_series", 65, 0, True), (65, 65, 65, 65, 65, 1, 0), ["regrow:ybuf", "regrow:per_step", "regrow:gamma", "series:eager:odd"]),
        (("lw_filter", 1, 2), (66, 66, 65, 65, 65, 65, 64), ["redraw:series"]),
        (("lw_reset",), (0, 0, 65, 65, 65, 65, 0), []),
        (("lw_filter", 2, 3), (2, 2, 65, 65, 65, 1, 64), ["redraw:reset"]),
    ],
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_model_bookkeeping_against_a_hand_written_table(name):
    m = L.HandleModel(L.SHAPES[name])
    for op, want, events in HAND[name]:
        got_ev = m.apply(op)
        assert (m.t, len(m.hist), m.ycap, m.tcap, m.gcap, m.gamma_t0, m.gamma_rows) == want, (op, want)
        assert got_ev == events, (op, got_ev)


def test_paths_file_is_current():
    with open(os.path.join(L.ROOT, "profiles", "lifecycle_paths.txt")) as f:
        assert f.read() == L.paths_report(), "regenerate: python tests/lifecycle_cases.py > profiles/lifecycle_paths.txt"
