"""Smoothing (ssme_pf_set_series_history, ssme_pf_sample_trajectories, ssme_pf_get_smoothed_expectations) against the step API.

The reference of every test is a second handle of the same configuration stepped with step() under set_debug(record_ancestors) and
downloaded after every step; tests/smooth_ref.py chases the genealogy in numpy.  Lineages (states and indices) are compared bit for
bit; the smoothed means against the exact rational value of tests/expect_ref.py for the host lineage's states and the final
fixed-point weights, within expect_ref's derived budgets (the sweep uses k_expect_partials' summation tree, so they apply to every
row), and their last row bit for bit against expectations_multi.  T = 7, R = 3 filters with distinct theta unless a test says otherwise.
Every test here fails without the feature: the entry points do not exist there."""
import ctypes as C
import os
import pickle
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import expect_ref as er
import series_expect_cases as sc
import smooth_ref as sr
from test_liu_west_edges_gpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
T = 7
ALL4 = sc.ALL4
# (name, N, tile_particles, set_small_series): the lane kernel at its smallest and at the shipped example's size, the pair kernel,
# the tiled route forced on a one-tile filter, three 512-tiles with a ragged last one, three 2048-tiles
ROUTES = (("lane-5", 5, 0, True), ("lane-500", 500, 0, True), ("pair-1030", 1030, 0, True), ("tiled-500-forced", 500, 0, False),
          ("tiled-1027-t512", 1027, 512, True), ("tiled-4100-t2048", 4100, 2048, True))
BY_NAME = {r[0]: r for r in ROUTES}
_REF = {}
_WORKER = {}


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None
    return ssme_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    O.build()
    return O


def series(model, last=None, steps=T):
    y, z = sc.stock_series(model, steps)
    if last is not None:
        y[-1] = last
    return y, z


def ref_for(sa, model, theta, n, tile, rs, sched, y, z, dtype=0):
    """The stepped reference of a configuration (independent of route and execution policy): computed once, shared, never modified."""
    key = (model, tuple(map(tuple, np.atleast_2d(theta))), n, tile, rs, sched, tuple(y), None if z is None else tuple(z), dtype)
    if key not in _REF:
        bank = sc.make_bank(sa, model, n, theta, rs, sched, tile, dtype=dtype)
        hist = sr.stepped_history(bank, y, z)
        bank.close()
        x, idx = sr.reference(hist, sched)
        _REF[key] = dict(hist=hist, x=x, idx=idx)
    return _REF[key]


def recorded_bank(sa, model, theta, n, tile, small, rs, sched, graph, y, z, dtype=0):
    bank = sc.make_bank(sa, model, n, theta, rs, sched, tile, dtype=dtype)
    bank.set_small_series(small)
    bank.set_graph_mode(graph)
    bank.record_series_history()
    want = sc.expected_route(n, tile, small)
    got = bank.series_route()
    assert got[0] == want[0] and (want[1] is None or got[1] == want[1]), (n, tile, got, want)      # recording keeps the route
    assert bank.series_history_bytes(len(y)) == len(y) * bank.r * bank.tile * bank.n_tiles * (8 * bank._dims()[0] + 4)
    ll = bank.run_series(y, z)
    return bank, ll


def all_lineages(bank):
    term = np.tile(np.arange(bank.n, dtype=np.uint32), (bank.r, 1))
    return bank.sample_trajectories(bank.n, terminal=term, indices=True)


def check_lineage(sa, model, theta, route, rs, sched, graph, name, last=None):
    _, n, tile, small = BY_NAME[route]
    y, z = series(model, last)
    ref = ref_for(sa, model, theta, n, tile, rs, sched, y, z)
    bank, _ = recorded_bank(sa, model, theta, n, tile, small, rs, sched, graph, y, z)
    x, idx = all_lineages(bank)
    bank.close()
    assert x.shape == (len(theta), n, T, 1) and idx.shape == (len(theta), n, T)
    np.testing.assert_array_equal(idx, ref["idx"], err_msg=name + ": lineage indices")
    same_bits(x, ref["x"], name + ": lineage states")
    if sched == 1 and n > 5:
        assert (idx[:, :, 0] != idx[:, :, -1]).any(), name + ": the genealogy is not the identity"


def policies(route):
    return (True, False) if route.startswith("tiled") else (True,)


# ---- 1. lineage, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [1, 3])
@pytest.mark.parametrize("route", [r[0] for r in ROUTES])
def test_lineage_equals_host_genealogy(sa, route, sched):
    """SVOL, every route; the tiled route as a graph and eagerly."""
    for graph in policies(route):
        check_lineage(sa, sc.MODEL_SVOL, sc.TH_SVOL3, route, 0, sched, graph, f"{route} sched={sched} graph={graph}")


@pytest.mark.parametrize("sched", [1, 3])
@pytest.mark.parametrize("rs", [0, 1, 2, 3], ids=["multinomial", "systematic", "stratified", "multinomial-iid"])
def test_lineage_every_resampler(sa, rs, sched):
    check_lineage(sa, sc.MODEL_SVOL, sc.TH_SVOL3, "pair-1030", rs, sched, True, f"pair-1030 rs={rs} sched={sched}")


@pytest.mark.parametrize("route", ["lane-500", "pair-1030", "tiled-1027-t512"])
def test_lineage_leverage_model_with_covariates(sa, route):
    for sched in (1, 3):
        for graph in policies(route):
            check_lineage(sa, sc.MODEL_SVOL_LEVERAGE, sc.TH_LEV3, route, 0, sched, graph, f"leverage {route} sched={sched} graph={graph}")


def _worker(tmp_path_factory):
    if "res" not in _WORKER:
        try:
            from ssme_amd import build
            env = dict(os.environ)
            env["SSME_PF_LIB"] = build.build_user_model(os.path.join(ROOT, "tests", "models", "svol_two_factor.h"), "two_factor")
            out = str(tmp_path_factory.mktemp("smooth_two_factor") / "res.pkl")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "smooth_worker.py"), out], env=env, check=True, timeout=240)
            with open(out, "rb") as f:
                _WORKER["res"] = pickle.load(f)
        except Exception as e:          # remembered, not retried
            _WORKER["res"] = e
    if isinstance(_WORKER["res"], Exception):
        raise RuntimeError(f"the worker failed and is not started again: {_WORKER['res']!r}") from _WORKER["res"]
    return _WORKER["res"]


def test_lineage_vector_user_model_both_planes(tmp_path_factory):
    """tests/models/svol_two_factor.h (dim_x = 2) on the lane kernel, the pair kernel and the tiled route, resamp_sched 1 and 3."""
    res = _worker(tmp_path_factory)
    assert len(res) == 6
    for name, r in res.items():
        assert r["route"][0] == r["want_route"][0], name
        assert r["x"].shape[-1] == 2 and r["bytes"] == T * r["x"].shape[0] * r["npad"] * 20, name
        np.testing.assert_array_equal(r["idx"], r["want_idx"], err_msg=name + ": lineage indices")
        same_bits(r["x"], r["want_x"], name + ": both state planes")
        assert not np.array_equal(r["x"][..., 0], r["x"][..., 1]), name


# ---- 2. terminal draw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lane-500", "pair-1030", "tiled-1027-t512"])
def test_terminal_draw_is_the_forecasts_start_draw(sa, route):
    _, n, tile, small = BY_NAME[route]
    y, z = series(sc.MODEL_SVOL)
    ref = ref_for(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, 0, 1, y, z)
    bank, _ = recorded_bank(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, small, 0, 1, True, y, z)
    _, start = bank.sim_future_obs(1, start=True)
    for K in (1, n):
        x, idx = bank.sample_trajectories(K, indices=True)
        np.testing.assert_array_equal(idx[:, :, T - 1], start[:, :K], err_msg=f"{route} K={K}")
        # the drawn trajectories are the lineages of the drawn final particles
        for r in range(bank.r):
            np.testing.assert_array_equal(idx[r], ref["idx"][r][start[r, :K]], err_msg=f"{route} K={K} filter {r}")
            same_bits(x[r], ref["x"][r][start[r, :K]], f"{route} K={K} filter {r}: states")
    assert len(np.unique(start[0])) > 1
    bank.close()


# ---- 3. smoothed expectations ----------------------------------------------------------------------------------------------------------
def check_smoothed(oracle, bank, ref, name, skip=()):
    """Row T-1 == expectations_multi (bits); every row within the budgets of the exact rational value for the host lineage's states."""
    steps = ref["x"].shape[2]
    sm = bank.smoothed_expectations(ALL4)
    assert sm.shape == (steps, 4, bank.r)
    same_bits(sm[steps - 1], bank.expectations_multi(ALL4), name + ": row T-1 == expectations_multi")
    worst = 0.0
    for r in range(bank.r):
        if r in skip:
            continue
        st = er.make_state(oracle, ref["hist"]["final"][r], bank.tile, bank.n)
        for t in range(steps):
            h = np.stack([er.builtin_h(oracle, k, ref["x"][r, :, t, 0]) for k in ALL4])
            exact = er.expect_fixed_point(h, st, "fraction")
            b_fp = er.budget_fixed_point(h, st)                                     # the bound the feature's specification names
            b_tree = er.budget_sum(bank.tile, bank.n_tiles, "expect", er.s_abs(h, st))    # ... and the summation tree's own
            for k in ALL4:
                err = float(abs(Fraction(float(sm[t, k, r])) - exact[k]))
                worst = max(worst, err / b_tree[k] if b_tree[k] > 0 else 0.0)
                assert err <= b_fp[k], (name, r, t, k, err, b_fp[k])
                assert err <= b_tree[k], (name, r, t, k, err, b_tree[k])
    print(f"{name}: worst error / tree budget = {worst:.3f}")
    return sm


@pytest.mark.parametrize("sched", [1, 3, T + 1], ids=["sched1", "sched3", "never-resampled"])
@pytest.mark.parametrize("route", ["lane-500", "tiled-1027-t512"])
def test_smoothed_expectations(sa, oracle, route, sched):
    _, n, tile, small = BY_NAME[route]
    y, z = series(sc.MODEL_SVOL)
    ref = ref_for(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, 0, sched, y, z)
    bank, _ = recorded_bank(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, small, 0, sched, True, y, z)
    if sched > T:
        # never resampled: the lineage is the identity and the rows are weighted means of the downloaded x_t under the final weights
        assert (ref["idx"] == np.arange(n, dtype=np.uint32)[None, :, None]).all()
        for r in range(3):
            same_bits(ref["x"][r, :, :, 0].T, np.stack(ref["hist"]["xs"][r]), "identity lineage")
    sm = check_smoothed(oracle, bank, ref, f"{route} sched={sched}")
    same_bits(bank.smoothed_expectations(ALL4), sm, "two calls, same bits")
    same_bits(bank.smoothed_expectations((2,))[:, 0], sm[:, 2], "one functional alone")
    bank.close()


# ---- 4. nothing else moved -----------------------------------------------------------------------------------------------------------
def _pass(bank, y, z):
    ll = bank.run_series(y, z)
    return dict(ll=ll, per=bank.per_step(), sts=[bank.state(f, logw=False) for f in range(bank.r)], traj=bank.series_expectations())


def _same_pass(a, b, name):
    same_bits(a["ll"], b["ll"], name + ": log-likelihoods")
    same_bits(a["per"], b["per"], name + ": per_step()")
    same_bits(a["traj"], b["traj"], name + ": recorded series expectations")
    for f, (s, t) in enumerate(zip(a["sts"], b["sts"])):
        same_bits(s["x"], t["x"], f"{name} filter {f}: particles")
        np.testing.assert_array_equal(s["cdf"], t["cdf"], err_msg=f"{name} filter {f}: cdf")
        np.testing.assert_array_equal(s["A"], t["A"], err_msg=f"{name} filter {f}: tile sums")
        same_bits(s["mb"], t["mb"], f"{name} filter {f}: tile maxima")
        assert s["S"] == t["S"], name


@pytest.mark.parametrize("route", ["lane-500", "pair-1030", "tiled-1027-t512"])
def test_recording_changes_nothing_else_and_history_life_cycle(sa, route):
    from ssme_amd import _capi
    L = _capi.lib()
    _, n, tile, small = BY_NAME[route]
    y, z = series(sc.MODEL_SVOL)
    for graph in policies(route):
        name = f"{route} graph={graph}"
        bank = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3, 0, 1, tile)
        bank.set_small_series(small)
        bank.set_graph_mode(graph)
        bank.record_series_expectations(ALL4)
        off = _pass(bank, y, z)
        ids, buf = (C.c_int32 * 1)(0), np.zeros(T * bank.r)
        xbuf = np.zeros(bank.r * T)
        smoothed = lambda: L.ssme_pf_get_smoothed_expectations(bank._h, ids, 1, _capi.dptr(buf), T)
        sampled = lambda: L.ssme_pf_sample_trajectories(bank._h, 1, None, _capi.dptr(xbuf), None, T)
        assert smoothed() == _capi.ERR_STATE and sampled() == _capi.ERR_STATE, name + ": recording was off"
        bank.record_series_history()
        on = _pass(bank, y, z)
        _same_pass(on, off, name + ": history on == off")
        x1, i1 = all_lineages(bank)
        f1 = bank.sim_future_obs(2)                       # forecasts, getters and downloads leave the history in force
        bank.expectations_multi(ALL4)
        bank.state(0, logw=False)
        x2, i2 = all_lineages(bank)
        same_bits(x2, x1, name + ": two calls, same bits")
        np.testing.assert_array_equal(i2, i1)
        same_bits(bank.sim_future_obs(2), f1, name + ": the forecast is untouched by the smoothing calls")
        assert L.ssme_pf_get_smoothed_expectations(bank._h, ids, 1, _capi.dptr(buf), T - 1) == _capi.ERR_INVALID_ARG
        # every call that moves the handle on discards the history
        for what, move in (("step", lambda: bank.step(y[0], None)), ("reset", bank.reset), ("set_seed", lambda: bank.set_seed(sc.SEED)),
                           ("set_params", lambda: bank.set_params(np.asarray(sc.TH_SVOL3)))):
            assert smoothed() == _capi.OK, f"{name}: before {what}"
            move()
            assert smoothed() == _capi.ERR_STATE and sampled() == _capi.ERR_STATE, f"{name}: after {what}"
            on2 = _pass(bank, y, z)                        # the setting survived: this run records again
            _same_pass(on2, off, f"{name}: after {what}, recording again")
        bank.record_series_history(False)
        off2 = _pass(bank, y, z)
        _same_pass(off2, off, name + ": off again")
        assert smoothed() == _capi.ERR_STATE and sampled() == _capi.ERR_STATE, name + ": run_series with recording off"
        bank.record_series_history(True)
        _same_pass(_pass(bank, y, z), off, name + ": on again")
        x3, i3 = all_lineages(bank)
        same_bits(x3, x1, name + ": on again, same lineages")
        np.testing.assert_array_equal(i3, i1)
        bank.close()


# ---- 5. degenerate inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lane-500", "pair-1030", "tiled-1027-t512"])
def test_bad_filter_gets_nan_and_neighbours_are_unaffected(sa, oracle, route):
    _, n, tile, small = BY_NAME[route]
    theta = (sc.TH_SVOL3[0], (-1.0, 0.95, 0.25), sc.TH_SVOL3[2])            # beta = -1: log g = -inf, no weight
    y, z = series(sc.MODEL_SVOL)
    ref = ref_for(sa, sc.MODEL_SVOL, theta, n, tile, 0, 1, y, z)
    bank, _ = recorded_bank(sa, sc.MODEL_SVOL, theta, n, tile, small, 0, 1, True, y, z)
    x, idx = all_lineages(bank)
    assert np.isnan(x[1]).all(), route
    for r in (0, 2):
        np.testing.assert_array_equal(idx[r], ref["idx"][r], err_msg=f"{route} filter {r}")
        same_bits(x[r], ref["x"][r], f"{route} filter {r}")
    xd = bank.sample_trajectories(3)                                       # drawn terminals: SSME_OK, NaN for the filter without weight
    assert np.isnan(xd[1]).all() and np.isfinite(xd[0]).all() and np.isfinite(xd[2]).all()
    sm = check_smoothed(oracle, bank, ref, route + " bad row", skip=(1,))
    assert np.isnan(sm[:, :, 1]).all() and np.isfinite(sm[:, :, 0]).all() and np.isfinite(sm[:, :, 2]).all()
    bank.close()


@pytest.mark.parametrize("shape", [("lane-500", 1, None), ("tiled-1027-t512", 1, None), ("n1", T, None), ("n1-tiled", T, None),
                                   ("lane-500", T, 1e3), ("tiled-1027-t512", T, 1e3)],
                         ids=["T1-lane", "T1-tiled", "N1-lane", "N1-tiled", "one-heavy-particle-lane", "one-heavy-particle-tiled"])
def test_degenerate_shapes(sa, oracle, shape):
    """T = 1; N = 1; a last observation of 1000, after which ONE particle carries all the final weight."""
    route, steps, last = shape
    _, n, tile, small = {"n1": ("n1", 1, 0, True), "n1-tiled": ("n1-tiled", 1, 0, False)}.get(route) or BY_NAME[route]
    y, z = series(sc.MODEL_SVOL, last, steps)
    ref = ref_for(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, 0, 1, y, z)
    heavy = []
    if last is not None:
        # the final weights are q_j exp(m_b - m): one nonzero per filter (a tile's own maximum has q = 2^41, the tile's scale is zero)
        for r in range(3):
            st = er.make_state(oracle, ref["hist"]["final"][r], tile or 2048, n)
            w = st["q"] * st["s"][st["tix"]]
            assert np.count_nonzero(w) == 1
            heavy.append(int(np.flatnonzero(w)[0]))
    bank, _ = recorded_bank(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, small, 0, 1, True, y, z)
    x, idx = all_lineages(bank)
    np.testing.assert_array_equal(idx, ref["idx"])
    same_bits(x, ref["x"], str(shape))
    check_smoothed(oracle, bank, ref, str(shape))
    xd, idd = bank.sample_trajectories(1, indices=True)
    _, start = bank.sim_future_obs(1, start=True)
    np.testing.assert_array_equal(idd[:, :, steps - 1], start[:, :1])
    if last is not None:                                                   # every draw ends at the one particle with weight
        for r in range(3):
            assert idd[r, 0, steps - 1] == heavy[r]
    bank.close()


# ---- 6. SSME_F32 handles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lane-500", "tiled-1027-t512"])
def test_f32_handle_rounds_inputs_and_outputs(sa, route):
    _, n, tile, small = BY_NAME[route]
    y, z = series(sc.MODEL_SVOL)
    th32 = np.asarray(sc.TH_SVOL3, dtype=np.float32).astype(np.float64)
    y32 = y.astype(np.float32).astype(np.float64)
    b64, _ = recorded_bank(sa, sc.MODEL_SVOL, th32, n, tile, small, 0, 1, True, y32, None)
    b32, _ = recorded_bank(sa, sc.MODEL_SVOL, np.asarray(sc.TH_SVOL3), n, tile, small, 0, 1, True, y, None, dtype=1)
    x64, i64 = all_lineages(b64)
    x32, i32 = all_lineages(b32)
    np.testing.assert_array_equal(i32, i64)
    same_bits(x32, x64.astype(np.float32).astype(np.float64), route + ": trajectories rounded to float")
    same_bits(b32.smoothed_expectations(ALL4), b64.smoothed_expectations(ALL4).astype(np.float32).astype(np.float64), route + ": rows rounded to float")
    b64.close()
    b32.close()


# ---- 7. refusals with a live handle; the debug ancestors of a recording run ------------------------------------------------------------
@pytest.mark.parametrize("route", ["lane-500", "tiled-1027-t512"])
def test_argument_refusals_with_a_live_handle(sa, route):
    """The block of tests/test_smoothing_cpu.py that needs a handle, on the machine that always has one: K, terminal indices, n,
    functional ids and NULL outputs are refused, and a handle that has recorded nothing answers SSME_ERR_STATE."""
    from ssme_amd import _capi
    from test_smoothing_cpu import refusals_with_a_handle
    _, n, tile, small = BY_NAME[route]
    bank = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3, 0, 1, tile)
    bank.set_small_series(small)
    refusals_with_a_handle(_capi.lib(), bank._h, n=n, r=3)
    # the same refusals once a history IS in force: they are checked before it is looked at
    y, z = series(sc.MODEL_SVOL)
    bank.record_series_history()
    bank.run_series(y, z)
    L, ids, buf = _capi.lib(), (C.c_int32 * 1)(7), np.zeros(bank.r * T * 4)
    assert L.ssme_pf_get_smoothed_expectations(bank._h, ids, 1, _capi.dptr(buf), T) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories(bank._h, n + 1, None, _capi.dptr(buf), None, T) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories(bank._h, 1, None, _capi.dptr(buf), None, T + 1) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_sample_trajectories(bank._h, 1, None, _capi.dptr(buf), None, T) == _capi.OK
    bank.close()


@pytest.mark.parametrize("steps", [7, 8, 2], ids=["last-step-resamples", "last-step-does-not", "no-draw-at-all"])
@pytest.mark.parametrize("route", ["lane-500", "tiled-1027-t512"])
def test_debug_ancestors_of_a_recording_run(sa, route, steps):
    """set_debug(record_ancestors) together with the history, resamp_sched = 3: state(ancestors=True) after a recording run is what
    it is after a non-recording run -- the indices of the last step that resampled (t = 6), also when the last step did not."""
    _, n, tile, small = BY_NAME[route]
    y, z = series(sc.MODEL_SVOL, None, steps)
    for graph in policies(route):
        got = []
        for rec in (False, True):
            bank = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3, 0, 3, tile)
            bank.set_small_series(small)
            bank.set_graph_mode(graph)
            bank.set_debug(record_ancestors=True, keep_logw=False)
            bank.record_series_history(rec)
            bank.run_series(y, z)
            got.append([bank.state(f, ancestors=True, logw=False) for f in range(bank.r)])
            bank.close()
        for f, (a, b) in enumerate(zip(*got)):
            np.testing.assert_array_equal(b["anc"], a["anc"], err_msg=f"{route} T={steps} graph={graph} filter {f}: debug ancestors")
            same_bits(b["x"], a["x"], f"{route} T={steps} graph={graph} filter {f}: particles")
