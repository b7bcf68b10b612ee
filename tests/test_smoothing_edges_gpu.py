"""The smoothing calls on the routes and inputs tests/test_smoothing_gpu.py does not reach (tests/smooth_edge_cases.py holds the list and
what every case expects; tests/README_smoothing_edges.md maps each gap to its test).  The helpers and the references are those of
test_smoothing_gpu.py: a stepped handle of the same library for lineages (bit for bit), expect_ref's exact rational value and derived
budgets for the smoothed rows.  No tolerance of its own."""
import ctypes as C
import io
import os
import pickle
import subprocess
import sys
from contextlib import redirect_stdout
from fractions import Fraction

import numpy as np
import pytest

import bs_edge_cases as bc
import expect_ref as er
import series_expect_cases as sc
import smooth_edge_cases as ec
import test_smoothing_gpu as tsg
from test_smoothing_gpu import all_lineages, check_smoothed, oracle, ref_for, sa  # noqa: F401  (sa, oracle: the fixtures)
from test_liu_west_edges_gpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
T = ec.T
ALL4 = sc.ALL4
BUDGETS = os.environ.get("SSME_SMOOTH_EDGE_BUDGETS")         # a file to append "case: worst error / budget" lines to (profiles/)
_WORKERS = {}


def bank_on(sa, route, model, theta, rs, sched, graph, y, z, first=0, total=0):
    """A recording handle on a named route, run over the series; asserts the shape and (tiled level-2 routes) route_of's table."""
    n, tile, small, split = ec.ROUTES[route]
    theta = np.asarray(theta, dtype=np.float64)
    bank = sa.ParticleFilterBank(model, n, theta.shape[0], sc.SEED, rs, sched, tile=tile, first_filter_id=first, n_filters_total=total)
    if split is not None:
        bank.set_debug(False, False, split_level2=split)
    bank.set_params(theta)
    bank.set_small_series(small)
    bank.set_graph_mode(graph)
    bank.record_series_history()
    if route in ec.ROUTE_TABLE:
        case = ec.route_case(sched, theta.shape[0])
        assert bc.route_of(case, ec.BS_ROUTES[route], "general", rs) == ec.ROUTE_TABLE[route], route
        assert (bank.tile, bank.n_tiles) == (ec.ROUTE_TABLE[route][3], ec.ROUTE_TILES[route]), (route, bank.tile, bank.n_tiles)
    want = sc.expected_route(n, tile, small)
    got = bank.series_route()
    assert got[0] == want[0] and (want[1] is None or got[1] == want[1]), (route, got, want)
    ll = bank.run_series(y, z)
    return bank, ll


def stepped_ref(sa, route, model, theta, rs, sched, y, z):
    n, tile, _, _ = ec.ROUTES[route]
    return ref_for(sa, model, theta, n, tile, rs, sched, y, z)


def note(line):
    print(line)
    if BUDGETS:
        with open(BUDGETS, "a") as f:
            f.write(line + "\n")


def counted_check(monkeypatch, oracle, bank, ref, name, skip=()):
    """check_smoothed, with the (filter, row, functional) triples it compared against the exact value counted, and its worst
    error / budget noted."""
    calls = []
    real = er.expect_fixed_point

    def counting(h, st, method=None):
        calls.append(len(h))
        return real(h, st, method)
    monkeypatch.setattr(er, "expect_fixed_point", counting)
    buf = io.StringIO()
    with redirect_stdout(buf):
        sm = check_smoothed(oracle, bank, ref, name, skip=skip)
    monkeypatch.setattr(er, "expect_fixed_point", real)
    note(buf.getvalue().strip())
    return sm, sum(calls)


# ---- 1. smoothed expectations on the routes that were never swept ---------------------------------------------------------------------
@pytest.mark.parametrize("sched", [1, 3])
@pytest.mark.parametrize("route", ec.SMOOTHED_ROUTES)
def test_smoothed_expectations_on_unswept_routes(sa, oracle, monkeypatch, route, sched):
    """k_sm_sweep<4> (tiles of 1024), <8> on several tiles, <2> on 129 tiles, and the one-tile pair kernel's history; graph and eager."""
    y, z = tsg.series(sc.MODEL_SVOL)
    ref = stepped_ref(sa, route, sc.MODEL_SVOL, ec.TH2, 0, sched, y, z)
    bank, _ = bank_on(sa, route, sc.MODEL_SVOL, ec.TH2, 0, sched, True, y, z)
    sm, n = counted_check(monkeypatch, oracle, bank, ref, f"smoothed {route} sched={sched}")
    assert n == 2 * T * 4 and np.isfinite(sm).all()
    bank.close()
    # launched eagerly: the bits of the graph's rows, which were just checked against the exact value
    bank, _ = bank_on(sa, route, sc.MODEL_SVOL, ec.TH2, 0, sched, False, y, z)
    eager = bank.smoothed_expectations(ALL4)
    same_bits(eager, sm, f"{route} sched={sched}: eager == graph")
    same_bits(eager[T - 1], bank.expectations_multi(ALL4), f"{route} sched={sched}: eager, row T-1 == expectations_multi")
    bank.close()


# ---- 2. lineages on every level-2 route of the tiled step ------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("route", ec.LINEAGE_ROUTES)
def test_lineages_on_level2_routes(sa, route, sched):
    """The history rows as x_in / x_out / anc of the general k_filter_step on the block-wide level-2, the forced split, the tables,
    the split by size (T = 3) and tiles of 1024 / 2048: lineages of ALL final particles equal the stepped reference, bit for bit;
    the smoothed rows' last one is expectations_multi."""
    steps = ec.steps_of(route)
    y, z = tsg.series(sc.MODEL_SVOL, None, steps)
    ref = stepped_ref(sa, route, sc.MODEL_SVOL, ec.TH2, 0, sched, y, z)
    bank, _ = bank_on(sa, route, sc.MODEL_SVOL, ec.TH2, 0, sched, True, y, z)
    x, idx = all_lineages(bank)
    assert idx.shape == (2, bank.n, steps)
    np.testing.assert_array_equal(idx, ref["idx"], err_msg=f"{route} sched={sched}: lineage indices")
    same_bits(x, ref["x"], f"{route} sched={sched}: lineage states")
    assert (idx[:, :, 0] != idx[:, :, -1]).any()
    sm = bank.smoothed_expectations(ALL4)
    same_bits(sm[steps - 1], bank.expectations_multi(ALL4), f"{route} sched={sched}: row T-1 == expectations_multi")
    assert np.isfinite(sm).all()
    bank.close()


# ---- 3. degenerate series ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ec.DEGENERATE_ROUTES)
@pytest.mark.parametrize("case", ec.DEGENERATE, ids=[c["name"] for c in ec.DEGENERATE])
def test_degenerate_series(sa, oracle, monkeypatch, case, route):
    """What the case list states (test_smoothing_edges_cpu.py derives it from the oracle): lineage indices equal the stepped reference
    for EVERY filter, states too for the live ones and NaN for the dead ones; smoothed rows NaN exactly for the dead filters; the
    calls return SSME_OK (the bindings raise on anything else); the rational check covers every live filter."""
    y, z = ec.series(case)
    name = f"{case['name']}@{route}"
    ref = stepped_ref(sa, route, case["model"], case["theta"], 0, case["sched"], y, z)
    dead = set(case["dead"])
    for r in range(case["R"]):                                # the reference's own final state says the same
        assert (not ref["hist"]["final"][r]["S"] > 0) == (r in dead), (name, r)
    if case["x_nan_from"] is not None:
        assert np.isnan(ref["x"][:, :, case["x_nan_from"]:]).all() and np.isfinite(ref["x"][:, :, :case["x_nan_from"]]).all()
    else:
        assert np.isfinite(ref["x"]).all()
    if case["coalesced_before"] is not None:
        s = case["coalesced_before"]
        assert all(len(np.unique(ref["idx"][r, :, t])) == 1 for r in range(case["R"]) for t in range(s)) and len(np.unique(ref["idx"][0, :, s])) > 1
    bank, _ = bank_on(sa, route, case["model"], case["theta"], 0, case["sched"], True, y, z)
    same_bits(bank.per_step(), ref["hist"]["ll"].T, name + ": per-step log-likelihoods")
    x, idx = all_lineages(bank)
    np.testing.assert_array_equal(idx, ref["idx"], err_msg=name + ": lineage indices")
    for r in range(case["R"]):
        if r in dead:
            assert np.isnan(x[r]).all(), (name, r)
        else:
            same_bits(x[r], ref["x"][r], f"{name} filter {r}: lineage states")
    xd = bank.sample_trajectories(3)                          # drawn terminals: SSME_OK, NaN for the dead
    for r in range(case["R"]):
        assert np.isnan(xd[r]).all() if r in dead else np.isfinite(xd[r]).all(), (name, r)
    sm, n = counted_check(monkeypatch, oracle, bank, ref, "degenerate " + name, skip=tuple(dead))
    assert n == ec.checked_triples(case)
    for r in range(case["R"]):
        assert np.isnan(sm[:, :, r]).all() if r in dead else np.isfinite(sm[:, :, r]).all(), (name, r)
    if case["zero_scale"] and bank.n_tiles > 1:
        for r in range(case["R"]):
            st = er.make_state(oracle, ref["hist"]["final"][r], bank.tile, bank.n)
            assert ((st["s"] == 0.0) & (np.asarray(st["A"]) > 0)).any(), name
    bank.close()


# ---- 4. a part of a bank: first_filter_id != 0 -----------------------------------------------------------------------------------------
TH8 = tuple((1.0 + 0.02 * i, 0.9 + 0.01 * i, 0.2 + 0.01 * i) for i in range(8))


@pytest.mark.parametrize("route", ["lane-500", "tiled-1027-t512"])
def test_split_bank_draws_like_the_whole_bank(sa, route):
    """first_filter_id = 5, n_filters_total = 8, R = 3: the drawn terminals (counter: filter id), the trajectories and the forecast's
    start draw are those of filters 5..7 of one handle of 8."""
    y, z = tsg.series(sc.MODEL_SVOL)
    whole, llw = bank_on(sa, route, sc.MODEL_SVOL, TH8, 0, 1, True, y, z)
    part, llp = bank_on(sa, route, sc.MODEL_SVOL, TH8[5:], 0, 1, True, y, z, first=5, total=8)
    assert (part.tile, part.n_tiles) == (whole.tile, whole.n_tiles)
    same_bits(llp, llw[5:], route + ": log-likelihoods")
    K = 257
    xw, iw = whole.sample_trajectories(K, indices=True)
    xp, ip = part.sample_trajectories(K, indices=True)
    np.testing.assert_array_equal(ip, iw[5:], err_msg=route + ": drawn lineages")
    same_bits(xp, xw[5:], route + ": drawn states")
    _, sw = whole.sim_future_obs(1, start=True)
    _, sp = part.sim_future_obs(1, start=True)
    np.testing.assert_array_equal(sp, sw[5:], err_msg=route + ": start draw")
    np.testing.assert_array_equal(ip[:, :, T - 1], sp[:, :K])
    assert not np.array_equal(ip[0], iw[0]) and len(np.unique(ip[0, :, T - 1])) > 1        # the filter id is in the counter
    same_bits(part.smoothed_expectations(ALL4), whole.smoothed_expectations(ALL4)[:, :, 5:], route + ": smoothed rows")
    whole.close()
    part.close()


# ---- 5. T changes on one handle: stale rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lane-500", "tiled-1027-t512"])
def test_changing_T_on_one_handle(sa, route):
    """T = 7, then 3, then 7 on one handle (the rows of the longer series stay allocated: rows 3..6 are stale during the short one):
    every read-out equals that of a fresh handle; after the T = 3 run, T = 7 is SSME_ERR_INVALID_ARG."""
    from ssme_amd import _capi
    L = _capi.lib()
    ys = {n: tsg.series(sc.MODEL_SVOL, None, n)[0] for n in (7, 3)}
    ys[3] = ys[3] + 0.5                                                     # another series, not a prefix of the long one
    fresh = {}
    for n in (7, 3):
        b, ll = bank_on(sa, route, sc.MODEL_SVOL, ec.TH2, 0, 1, True, ys[n], None)
        fresh[n] = (ll, all_lineages(b), b.sample_trajectories(64, indices=True), b.smoothed_expectations(ALL4))
        b.close()
    bank, ll = bank_on(sa, route, sc.MODEL_SVOL, ec.TH2, 0, 1, True, ys[7], None)
    for i, n in enumerate((7, 3, 7)):
        if i:
            ll = bank.run_series(ys[n], None)
        name = f"{route} run {i} (T = {n})"
        want = fresh[n]
        same_bits(ll, want[0], name + ": log-likelihoods")
        x, idx = all_lineages(bank)
        np.testing.assert_array_equal(idx, want[1][1], err_msg=name)
        same_bits(x, want[1][0], name + ": lineages")
        xd, idd = bank.sample_trajectories(64, indices=True)
        np.testing.assert_array_equal(idd, want[2][1], err_msg=name)
        same_bits(xd, want[2][0], name + ": drawn trajectories")
        same_bits(bank.smoothed_expectations(ALL4), want[3], name + ": smoothed rows")
        if n == 3:
            ids, buf = (C.c_int32 * 1)(0), np.zeros(7 * bank.r * 4)
            assert L.ssme_pf_get_smoothed_expectations(bank._h, ids, 1, _capi.dptr(buf), 7) == _capi.ERR_INVALID_ARG
            assert L.ssme_pf_sample_trajectories(bank._h, 1, None, _capi.dptr(buf), None, 7) == _capi.ERR_INVALID_ARG
            assert L.ssme_pf_get_smoothed_expectations(bank._h, ids, 1, _capi.dptr(buf), 3) == _capi.OK
    bank.close()


# ---- 6. across the 64-row Gamma chunk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lane-500", "tiled-1027-t512"])
def test_lineages_across_the_gamma_chunk(sa, route):
    """T = 65, multinomial resampler (its sorted uniforms come from Gamma rows made 64 steps at a time), history on."""
    steps = 65
    y, z = tsg.series(sc.MODEL_SVOL, None, steps)
    ref = stepped_ref(sa, route, sc.MODEL_SVOL, ec.TH2, 0, 1, y, z)
    bank, _ = bank_on(sa, route, sc.MODEL_SVOL, ec.TH2, 0, 1, True, y, z)
    x, idx = all_lineages(bank)
    np.testing.assert_array_equal(idx, ref["idx"], err_msg=route + ": lineage indices")
    same_bits(x, ref["x"], route + ": lineage states")
    assert (idx[:, :, 63] != idx[:, :, 64]).any() and (idx[:, :, 62] != idx[:, :, 63]).any()      # the draws of t = 64 and t = 63 moved lineages
    sm = bank.smoothed_expectations(ALL4)
    same_bits(sm[steps - 1], bank.expectations_multi(ALL4), route + ": row T-1 == expectations_multi")
    bank.close()


# ---- 7. vector models (libraries with a user model: a process of their own) ----------------------------------------------------------------
def _worker(tmp_path_factory, mode, lib, header):
    """smooth_worker.py in `mode` on the library `lib` (built by the build step from tests/models/<header>.h), once."""
    if mode not in _WORKERS:
        try:
            from ssme_amd import build
            env = dict(os.environ)
            env["SSME_PF_LIB"] = build.build_user_model(os.path.join(ROOT, "tests", "models", header + ".h"), lib)
            out = str(tmp_path_factory.mktemp("smooth_edges_" + mode) / "res.pkl")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "smooth_worker.py"), out, mode], env=env, check=True, timeout=240)
            with open(out, "rb") as f:
                _WORKERS[mode] = pickle.load(f)
        except Exception as e:          # remembered, not retried
            _WORKERS[mode] = e
    if isinstance(_WORKERS[mode], Exception):
        raise RuntimeError(f"the worker failed and is not started again: {_WORKERS[mode]!r}") from _WORKERS[mode]
    return _WORKERS[mode]


def test_smoothed_expectations_of_a_vector_model(oracle, tmp_path_factory):
    """svol_two_factor.h (dim_x = 2) on the lane, pair and tiled routes: the sweep reads plane 0 of a row of dx planes.  Exact
    rational reference on component 0 of the host lineage; last row == expectations_multi."""
    res = _worker(tmp_path_factory, "smoothed", "two_factor", "svol_two_factor")
    assert len(res) == 6
    for name, r in res.items():
        assert r["route"][0] == r["want_route"][0], name
        sm, steps = r["sm"], r["want_x"].shape[2]
        assert sm.shape == (steps, 4, r["want_x"].shape[0]) and r["want_x"].shape[3] == 2
        same_bits(sm[steps - 1], r["em"], name + ": row T-1 == expectations_multi")
        worst, n = 0.0, 0
        for f in range(sm.shape[2]):
            st = er.make_state(oracle, dict(r["final"][f], x=r["final"][f]["x"][0]), r["tile"], r["n"])
            for t in range(steps):
                h = np.stack([er.builtin_h(oracle, k, r["want_x"][f, :, t, 0]) for k in ALL4])
                h1 = np.stack([er.builtin_h(oracle, k, r["want_x"][f, :, t, 1]) for k in ALL4])
                exact = er.expect_fixed_point(h, st, "fraction")
                b_tree = er.budget_sum(r["tile"], r["n_tiles"], "expect", er.s_abs(h, st))
                for k in ALL4:
                    err = float(abs(Fraction(float(sm[t, k, f])) - exact[k]))
                    assert err <= b_tree[k], (name, f, t, k, err, b_tree[k])
                    worst = max(worst, err / b_tree[k] if b_tree[k] > 0 else 0.0)
                    n += 1
                # the cases can tell the planes apart: component 1 has another mean
                assert abs(float(er.expect_fixed_point(h1, st, "longdouble")[0]) - sm[t, 0, f]) > 100 * b_tree[0], (name, f, t)
        assert n == sm.size
        note(f"vector {name}: worst error / tree budget = {worst:.3f}")


def test_lineages_of_a_three_plane_model(tmp_path_factory):
    """lin_gauss_3d.h: k_sm_trajectories<3> and the DX = 3 history writes of the whole-series kernels and the tiled step."""
    res = _worker(tmp_path_factory, "dx3", "lin_gauss_3d", "lin_gauss_3d")
    assert len(res) == 6
    for name, r in res.items():
        assert r["route"][0] == r["want_route"][0], name
        assert r["x"].shape[-1] == 3 and r["bytes"] == T * r["x"].shape[0] * r["npad"] * 28, name
        np.testing.assert_array_equal(r["idx"], r["want_idx"], err_msg=name + ": lineage indices")
        same_bits(r["x"], r["want_x"], name + ": all three state planes")
        assert not np.array_equal(r["x"][..., 0], r["x"][..., 1]) and not np.array_equal(r["x"][..., 1], r["x"][..., 2]), name


def test_user_functionals_with_the_history_on(tmp_path_factory):
    """svol_two_factor_h.h on the tiled route: k_user_expect_partials_row reads the history row; the recorded user expectations with
    the history on equal those with it off, bit for bit."""
    res = _worker(tmp_path_factory, "user_h", "two_factor_h", "svol_two_factor_h")
    assert len(res) == 2
    for name, r in res.items():
        assert r["route"][0] == sc.ROUTE_TILED, name
        assert r["on"].shape == r["off"].shape and r["on"].shape[0] == T and r["on"].shape[1] == 7 and np.isfinite(r["off"]).all()
        same_bits(r["on"], r["off"], name + ": series_user_expectations, history on == off")
        same_bits(r["ll_on"], r["ll_off"], name + ": log-likelihoods")
        np.testing.assert_array_equal(r["idx"], r["want_idx"], err_msg=name + ": lineage indices")
        same_bits(r["x"], r["want_x"], name + ": lineages while the user functionals are recorded")
