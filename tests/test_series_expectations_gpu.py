"""Recorded series (ssme_pf_set_series_expectations): the filtered expectations of EVERY step of run_series, bit for bit against the
step API.  Row t of series_expectations() / series_user_expectations() must be what expectations_multi() / user_expectations()
return after step t of a fresh handle stepped with step() -- on the whole-series routes (pf_small.h, which forms the rows in LDS by the
expectation kernels' summation trees), on the tiled route (graph and eager, in-kernel and split level-2) and for the functionals of
user-model headers (one process per library: tests/series_expect_worker.py).  The lists are tests/series_expect_cases.py.

Every comparison is exact (same_bits: NaN for NaN) except test_anchor_exact_rational, which applies the budgets of tests/expect_ref.py
as tests/test_expectations_gpu.py applies them to a single step.  Every test here fails without the feature: the entry points do
not exist there."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import expect_cases as ec
import expect_ref as er
import series_expect_cases as sc
from test_expectations_gpu import check_rows, compare_state
from test_liu_west_edges_gpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "models")
pytestmark = pytest.mark.gpu
WORKER_TIMEOUT = 240
_DONE = {}


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None
    return ssme_amd


def _route_ok(bank, n, tile, small=True):
    want = sc.expected_route(n, tile, small)
    got = bank.series_route()
    assert got[0] == want[0] and (want[1] is None or got[1] == want[1]), (n, tile, got, want)


def _against_stepping(sa, model, theta, n, tile, split, rs, sched, functionals, name):
    y, z = sc.stock_series(model)
    bank = sc.make_bank(sa, model, n, theta, rs, sched, tile, split)
    bank.record_series_expectations(functionals)
    _route_ok(bank, n, tile)                       # what a RECORDING handle launches
    ll, traj, _ = sc.recorded(bank, y, z, functionals)
    bank.close()
    want, _ = sc.stepped(sa, model, n, theta, y, z, functionals, rs=rs, sched=sched, tile=tile, split=split)
    assert traj.shape == (len(y), len(functionals), 1 if np.ndim(theta) == 1 else len(theta))
    assert np.isfinite(traj).all(), name
    same_bits(traj, want, name)


# ---- 1. trajectory == stepping, built-ins, stock library ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: f"N{s[0]}-tile{s[1]}-split{s[2]}")
def test_trajectory_equals_stepping_builtins(sa, shape):
    """SVOL, R = 3 with one theta row per filter, all four functionals at once; all four resamplers x resamp_sched 1 and 3."""
    n, tile, split = shape
    for rs in sc.RESAMPLERS:
        for sched in sc.SCHEDULES:
            _against_stepping(sa, sc.MODEL_SVOL, sc.TH_SVOL3, n, tile, split, rs, sched, sc.ALL4, f"N={n} tile={tile} split={split} rs={rs} sched={sched}")


@pytest.mark.parametrize("model", list(sc.MODELS), ids=["svol", "leverage-z", "lin-gauss"])
@pytest.mark.parametrize("shape", sc.OTHER_SHAPES, ids=lambda s: f"N{s[0]}")
def test_trajectory_equals_stepping_models_single_filter_single_functional(sa, model, shape):
    """Every built-in model (the leverage model with its covariate), R = 1, SSME_H_VOL alone and R = 3 with a permuted list."""
    n, tile, split = shape
    for rs in (0, 1):
        for sched in sc.SCHEDULES:
            _against_stepping(sa, model, sc.MODELS[model][0], n, tile, split, rs, sched, (2,), f"model {model} N={n} rs={rs} sched={sched} VOL alone")
        _against_stepping(sa, model, sc.MODELS[model], n, tile, split, rs, 1, (3, 0, 2), f"model {model} N={n} rs={rs} three functionals, R = 3")


# ---- 2. recording changes nothing else -----------------------------------------------------------------------------------------------
def _pass(bank, y, z, R):
    ll = bank.run_series(y, z)
    sts = [bank.state(f, logw=False) for f in range(R)]
    return dict(ll=ll, per=bank.per_step(), sts=sts)


def _same_pass(a, b, name):
    same_bits(a["ll"], b["ll"], name + ": log-likelihoods")
    same_bits(a["per"], b["per"], name + ": per_step()")
    for f, (s, t) in enumerate(zip(a["sts"], b["sts"])):
        same_bits(s["x"], t["x"], f"{name} filter {f}: particles")
        np.testing.assert_array_equal(s["cdf"], t["cdf"], err_msg=f"{name} filter {f}: cdf")
        np.testing.assert_array_equal(s["A"], t["A"], err_msg=f"{name} filter {f}: tile sums")
        same_bits(s["mb"], t["mb"], f"{name} filter {f}: tile maxima")
        same_bits([s["m"]], [t["m"]], f"{name} filter {f}: m")
        assert s["S"] == t["S"], name


@pytest.mark.parametrize("n", [500, 1500, 3000])
def test_recording_changes_nothing_else(sa, n):
    """off -> on -> off on one handle: sums, per_step(), state and scalars are the same bits; eager == graph; set_small_series(0)
    gives the same trajectory."""
    y, z = sc.stock_series(sc.MODEL_SVOL)
    bank = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3)
    off = _pass(bank, y, z, 3)
    bank.record_series_expectations(sc.ALL4)
    on = _pass(bank, y, z, 3)
    traj = bank.series_expectations()
    bank.record_series_expectations(())
    off2 = _pass(bank, y, z, 3)
    _same_pass(on, off, f"N={n}: recording on == off")
    _same_pass(off2, off, f"N={n}: off again == off")
    # the tiled route on the same handle, graph then eager
    bank.record_series_expectations(sc.ALL4)
    bank.set_small_series(False)
    assert bank.series_route()[0] == sc.ROUTE_TILED
    tiled_g = _pass(bank, y, z, 3)
    traj_g = bank.series_expectations()
    bank.set_graph_mode(False)
    tiled_e = _pass(bank, y, z, 3)
    traj_e = bank.series_expectations()
    bank.close()
    _same_pass(tiled_g, off, f"N={n}: tiled, graph")
    _same_pass(tiled_e, off, f"N={n}: tiled, eager")
    same_bits(traj_g, traj, f"N={n}: set_small_series(0), graph == default route")
    same_bits(traj_e, traj, f"N={n}: eager == graph")


# ---- 3. graph replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [sc.MODEL_SVOL, sc.MODEL_SVOL_LEVERAGE], ids=["other-y", "leverage-other-z"])
def test_graph_replay_second_series(sa, model):
    """Two run_series of the same T on one recording handle (the second replays the captured graph) with other y (and z): the second
    trajectory is that of a fresh handle, and of stepping."""
    n = 3000
    y1, z1 = sc.stock_series(model)
    y2, z2 = sc.stock_series(model, shift=40)
    bank = sc.make_bank(sa, model, n, sc.MODELS[model])
    _, first, _ = sc.recorded(bank, y1, z1)
    _, second, _ = sc.recorded(bank, y2, z2)
    bank.close()
    fresh = sc.make_bank(sa, model, n, sc.MODELS[model])
    _, want, _ = sc.recorded(fresh, y2, z2)
    fresh.close()
    same_bits(second, want, "replayed graph == fresh handle")
    same_bits(second, sc.stepped(sa, model, n, sc.MODELS[model], y2, z2)[0], "replayed graph == stepping")
    assert not np.array_equal(first, second)


# ---- 4. user functionals (one process per library) -------------------------------------------------------------------------------------
def _worker(lib, tmp_path_factory):
    """What the worker pickled for a library: started once per session; a worker that failed is not started again, and none after it."""
    first = next((e for e in _DONE.values() if isinstance(e, Exception)), None)
    if lib not in _DONE and first is not None:
        _DONE[lib] = first
    if lib not in _DONE:
        try:
            from ssme_amd import build
            env = dict(os.environ)
            header = sc.NO_H_LIB["header"] if lib == sc.NO_H_LIB["lib"] else sc.USER_LIBS[lib]["header"]
            env["SSME_PF_LIB"] = build.build_user_model(os.path.join(MODELS, header + ".h"), lib)
            out = str(tmp_path_factory.mktemp(f"se_{lib}") / "res.pkl")
            subprocess.run([sys.executable, os.path.join(ROOT, "tests", "series_expect_worker.py"), lib, out], env=env, check=True,
                           timeout=WORKER_TIMEOUT)
            with open(out, "rb") as f:
                _DONE[lib] = pickle.load(f)
        except Exception as e:          # remembered, not retried
            _DONE[lib] = e
    if isinstance(_DONE[lib], Exception):
        raise RuntimeError(f"a worker failed and none is started after it ({lib}): {_DONE[lib]!r}") from _DONE[lib]
    return _DONE[lib]


@pytest.mark.parametrize("lib", list(sc.USER_LIBS))
def test_user_functionals_equal_stepping(lib, tmp_path_factory):
    """Built-ins and the header's n_h functionals recorded together, N = 100 .. 2049, every row against stepping; h receives the
    covariates of row t."""
    r = _worker(lib, tmp_path_factory)
    s = sc.USER_LIBS[lib]
    for n in sc.USER_SIZES:
        for rs, sched in ((0, 1), (1, 3)):
            d = r[("rows", n, rs, sched)]
            name = f"{lib} N={n} rs={rs} sched={sched}"
            want = sc.expected_route(n)
            assert d["route"][0] == want[0] and (want[1] is None or d["route"][1] == want[1]), (name, d["route"])
            assert d["utraj"].shape == (sc.USER_T, s["n_h"], len(s["theta"])) and np.isfinite(d["utraj"]).all(), name
            same_bits(d["utraj"], d["uref"], name + ": user functionals")
            same_bits(d["traj"], d["ref"], name + ": built-ins recorded with them")
        same_bits(r[("user-only", n)], r[("rows", n, 0, 1)]["utraj"], f"{lib} N={n}: user functionals alone")
        same_bits(r[("tiled", n)], r[("rows", n, 0, 1)]["utraj"], f"{lib} N={n}: set_small_series(0)")


@pytest.mark.parametrize("lib", list(sc.USER_LIBS))
def test_user_graph_replay_reads_covariates_on_the_device(lib, tmp_path_factory):
    """The tiled route's graph is replayed for a second series with other covariates: the recorded launches read row t of the uploaded
    covariates (svol_reg_cov, svol_two_factor_cov: dim_cov; the others: the scalar covariate), so the second trajectory is stepping's."""
    r = _worker(lib, tmp_path_factory)
    d = r["replay"]
    same_bits(d["second_u"], d["uref"], f"{lib}: replayed graph, user functionals == stepping")
    same_bits(d["second_b"], d["ref"], f"{lib}: replayed graph, built-ins == stepping")
    same_bits(d["noz_u"], d["uref_noz"], f"{lib}: replayed for a series WITHOUT covariates (another graph): zeros")
    if sc.USER_LIBS[lib]["z"]:
        assert not np.array_equal(d["first_u"], d["second_u"])


def test_user_flag_on_a_header_without_functionals(tmp_path_factory):
    """SSME_MODEL_USER0 handles of a library whose header declares no functionals (n_h == 0): user != 0 is SSME_ERR_UNSUPPORTED, with
    or without built-ins beside it, and the built-ins still record."""
    from ssme_amd import _capi
    st = _worker(sc.NO_H_LIB["lib"], tmp_path_factory)["status"]
    assert st["user-with-n_h-0"] == _capi.ERR_UNSUPPORTED and st["user-only-with-n_h-0"] == _capi.ERR_UNSUPPORTED
    assert st["builtins-with-n_h-0"] == _capi.OK and st["get-builtins"] == _capi.OK and st["get-user"] == _capi.ERR_STATE


@pytest.mark.parametrize("lib", sc.BAD_ROW_LIBS)
def test_user_degenerate_rows_and_statuses(lib, tmp_path_factory):
    """Every library whose model has a `bad` theta row in user_edge_cases.HEADERS: that row in the middle filter of three."""
    r = _worker(lib, tmp_path_factory)
    from ssme_amd import _capi
    for n in sc.BAD_ROW_SIZES:
        d = r[("bad-row", n)]
        same_bits(d["utraj"], d["uref"], f"{lib} N={n}: bad theta row in the middle, user functionals")
        same_bits(d["traj"], d["ref"], f"{lib} N={n}: bad theta row in the middle, built-ins")
        assert np.isnan(d["utraj"][:, :, 1]).all() and np.isfinite(d["utraj"][:, :, 0]).all() and np.isfinite(d["utraj"][:, :, 2]).all()
    assert r["status"]["user-on-builtin-model"] == _capi.ERR_UNSUPPORTED
    assert r["status"]["user-get-without-user"] == _capi.ERR_STATE


# ---- 5. degenerate inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sc.degenerate_rows(), ids=lambda r: r[0])
def test_degenerate_rows(sa, row):
    """Weights that are all NaN, all zero or gone to -inf in one filter of three (or in all from one step on): the NaN rows and the
    healthy neighbours' rows equal stepping, and the call returns SSME_OK."""
    name, model, theta, y_set, sched, T = row
    for n, tile in ((300, 0), (1500, 0), (3000, 0)):
        y, z = sc.stock_series(model, T=T)
        for t, v in y_set.items():
            y[t] = v
        bank = sc.make_bank(sa, model, n, theta, sched=sched)
        _, traj, _ = sc.recorded(bank, y, z)
        bank.close()
        want, _ = sc.stepped(sa, model, n, theta, y, z, sched=sched)
        same_bits(traj, want, f"{name} N={n}")
        assert np.isnan(traj).any() and np.isfinite(traj).any(), name
        if not y_set:
            assert np.isnan(traj[:, :, 1]).all() and np.isfinite(traj[:, :, (0, 2)]).all(), name
        if sched == 3:                                   # NaN rows from the NaN observation up to the next resampling step, finite after
            first = min(y_set)
            assert np.isnan(traj[first:6]).all() and np.isfinite(traj[:first]).all() and np.isfinite(traj[6]).all(), name


@pytest.mark.parametrize("n", [300, 1500, 3000])
def test_zero_observations_and_one_step(sa, n):
    th = sc.TH_SVOL3
    y0 = np.array([0.0, -0.0, 0.0, 0.0])
    for y in (y0, sc.spy()[:1].copy(), np.array([0.0])):
        bank = sc.make_bank(sa, sc.MODEL_SVOL, n, th)
        _, traj, _ = sc.recorded(bank, y, None)
        bank.close()
        assert traj.shape == (len(y), 4, 3)
        same_bits(traj, sc.stepped(sa, sc.MODEL_SVOL, n, th, y, None)[0], f"N={n} y={y.tolist()}")


# ---- 6. one longer run -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [500, 1500])
def test_longer_run_volatility_path(sa, n):
    """The first 256 rows of spy_returns.csv, SSME_H_VOL: the volatility path a user plots."""
    y = sc.spy()[:256].copy()
    bank = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3[0])
    _, traj, _ = sc.recorded(bank, y, None, (2,))
    bank.close()
    assert traj.shape == (256, 1, 1) and np.isfinite(traj).all() and (traj > 0).all()
    same_bits(traj, sc.stepped(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3[0], y, None, (2,))[0], f"N={n} T=256")


# ---- 7. an anchor that does not pass through the step path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False], ids=["whole-series", "tiled"])
def test_anchor_exact_rational(sa, oracle, small):
    """N = 100, T = 6: every recorded row within the budgets tests/expect_ref.py derives for the exact rational value built from the
    ORACLE's state at that step (E_q within budget_sum, E_exact within budget_sum + budget_fixed_point), as
    tests/test_expectations_gpu.py applies them to one step."""
    case = ec._case("series-anchor-100", 100, T=6, every_step=True)
    y, _ = ec.observations(case)
    bank = sa.ParticleFilterBank(case["model"], case["n"], case["R"], case["seed"], case["rs"], case["sched"], tile=case["tile"])
    bank.set_params(np.asarray(case["theta"], dtype=np.float64))
    bank.set_small_series(small)
    bank.record_series_expectations(sc.ALL4)
    ll = bank.run_series(y)
    traj = bank.series_expectations()
    seen = 0
    for t, tile, ofs, _ in ec.walk_oracle(oracle, case):
        st = er.make_state(oracle, ofs[0].state(), tile)
        check_rows(f"series-anchor t={t}", traj[t, :, 0], ec.builtin_rows(oracle, st["x"]), st, "expect")
        seen += 1
    assert seen == 6 and ll[0] == ofs[0].loglik
    compare_state(bank, 0, ofs[0], tile, "series-anchor: state after the series")
    bank.close()


# ---- 8. statuses -----------------------------------------------------------------------------------------------------------------
def test_statuses_and_f32(sa):
    from ssme_amd import _capi
    L = _capi.lib()
    i32p = C.POINTER(C.c_int32)
    ids = (C.c_int32 * 5)(0, 1, 2, 3, 0)
    bad_id, neg_id = (C.c_int32 * 1)(4), (C.c_int32 * 1)(-1)
    buf = np.zeros(8 * 4 * 3)
    y, _ = sc.stock_series(sc.MODEL_SVOL)
    bank = sc.make_bank(sa, sc.MODEL_SVOL, 500, sc.TH_SVOL3)
    h = bank._h
    assert L.ssme_pf_set_series_expectations(None, ids, 1, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_expectations(h, bad_id, 1, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_expectations(h, neg_id, 1, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_expectations(h, ids, 5, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_expectations(h, ids, -1, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_expectations(h, None, 1, 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_set_series_expectations(h, ids, 1, 1) == _capi.ERR_UNSUPPORTED          # user functionals on a built-in model
    assert L.ssme_pf_set_series_expectations(h, None, 0, 0) == _capi.OK
    # nothing recorded yet; NULL arguments; T
    assert L.ssme_pf_get_series_expectations(h, _capi.dptr(buf), 1) == _capi.ERR_STATE
    assert L.ssme_pf_get_series_user_expectations(h, _capi.dptr(buf), 1) == _capi.ERR_STATE
    bank.run_series(y)
    assert L.ssme_pf_get_series_expectations(h, _capi.dptr(buf), 1) == _capi.ERR_STATE          # get after a non-recording run
    bank.record_series_expectations((2, 0))
    assert L.ssme_pf_get_series_expectations(h, _capi.dptr(buf), 1) == _capi.ERR_STATE          # set alone records nothing
    bank.run_series(y)
    assert L.ssme_pf_get_series_expectations(None, _capi.dptr(buf), 1) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_series_expectations(h, None, 1) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_series_expectations(h, _capi.dptr(buf), 0) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_series_expectations(h, _capi.dptr(buf), len(y) + 1) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_get_series_user_expectations(h, _capi.dptr(buf), 1) == _capi.ERR_STATE     # nothing recorded of that kind
    full = bank.series_expectations()
    head = np.zeros((3, 2, 3))
    assert L.ssme_pf_get_series_expectations(h, _capi.dptr(head), 3) == _capi.OK                # rows 0 .. T-1 of a longer series
    same_bits(head, full[:3], "the first three rows")
    # sticky across set_params, set_seed and reset; step neither records nor clears
    bank.set_params(np.asarray(sc.TH_SVOL3))
    bank.set_seed(sc.SEED)
    bank.reset()
    bank.run_series(y)
    same_bits(bank.series_expectations(), full, "sticky: set_params, set_seed, reset")
    bank.step(0.1)
    same_bits(bank.series_expectations(), full, "step neither records nor clears")
    want, _ = sc.stepped(sa, sc.MODEL_SVOL, 500, sc.TH_SVOL3, y, None, (2, 0))
    same_bits(full, want, "two functionals in another order")
    bank.record_series_expectations(())
    bank.run_series(y)
    assert L.ssme_pf_get_series_expectations(h, _capi.dptr(buf), 1) == _capi.ERR_STATE
    bank.close()
    # a sharded handle
    cfg = _capi.Config(model=_capi.MODEL_SVOL, n_particles=4 * 2048, n_filters=1, dtype=0, resampler=0, resamp_sched=1, seed=1, device=0)
    hs = C.c_void_p()
    assert L.ssme_pf_shard_create(C.byref(cfg), 0, 2, C.byref(hs)) == _capi.OK
    assert L.ssme_pf_set_series_expectations(hs, ids, 1, 0) == _capi.ERR_STATE
    L.ssme_pf_destroy(hs)
    # SSME_F32: rows rounded to float, and equal to the F32 handle's stepping
    for n in (500, 3000):
        b32 = sc.make_bank(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3, dtype=_capi.F32)
        _, t32, _ = sc.recorded(b32, y, None)
        b32.close()
        assert np.array_equal(t32, t32.astype(np.float32).astype(np.float64))
        same_bits(t32, sc.stepped(sa, sc.MODEL_SVOL, n, sc.TH_SVOL3, y, None, dtype=_capi.F32)[0], f"F32 N={n}")
