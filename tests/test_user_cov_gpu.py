"""GPU suite for user models with covariates (ssme_amd/csrc/model_api.h: dim_cov, first / first_logw; DESIGN.md sections 1 and 10).

Every library runs ONCE per session in a process of its own (tests/user_cov_worker.py with SSME_PF_LIB; a process binds one
libssme_pf.so) and the tests compare what it wrote with the oracle closures and numpy restatements of tests/user_cov_ref.py, to the
bit.  Shapes: T = 6 rows of spy_returns.csv, covariates from a fixed-seed normal draw, (N, tile) = (500, -) one ragged tile and the
whole-series kernel, (2500, 512) five tiles with a ragged last one, (2500, 2048) two tiles; resamp_sched 1 and 2; multinomial and
systematic; R = 2 filters with different parameter rows, filter 1 compared.

The functionals are compared with expect_ref.expect_fixed_point within expect_ref.budget_fixed_point (derived there)."""
import functools
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import expect_ref as er
import user_cov_ref as ucr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "tests", "models")
HEADERS = ("svol_reg_cov", "svol_reg_cov_nofirst", "svol_leverage_cov1", "svol_two_factor_cov")
CONFIGS = [(n, tile, sched, rs) for n, tile in ucr.SHAPES for sched in (1, 2) for rs in (0, 1)]
T = ucr.T_STEPS


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a HIP device"
    import ssme_amd
    return ssme_amd


@functools.lru_cache(maxsize=None)
def _run(name):
    """The worker's output for one library: built once, run once per session."""
    from ssme_amd import build
    import tempfile
    hdr, lib = ("svol_leverage_user", "leverage_user") if name == "leverage_plain" else (name, name)
    so = build.build_user_model(os.path.join(MODELS, hdr + ".h"), lib)
    out = os.path.join(tempfile.mkdtemp(prefix="user_cov_"), name + ".npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "user_cov_worker.py"), name, out], env=dict(os.environ, SSME_PF_LIB=so),
                   check=True, timeout=600)
    res = dict(np.load(out))
    shutil.rmtree(os.path.dirname(out), ignore_errors=True)
    return res


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_ORACLE = {}


def _oracle(oracle, spy, name, n, tile, sched, rs, with_z=True):
    """(per-step log-likelihoods, series log-likelihood, state) of filter 1 from the oracle closures; computed once and shared."""
    key = (name, n, tile, sched, rs, with_z)
    if key not in _ORACLE:
        m = ucr.MODELS[name]
        y, Z, th = ucr.observations(spy, m["dy"]), (ucr.covariates(m["K"]) if with_z else None), m["theta"][1]
        if m["dx"] == 1 and m["dy"] == 1 and m["first"] is None:
            f = ucr.scalar_oracle(oracle, name, th, Z, n, ucr.SEED, 1, rs, sched, tile)
            per = np.array([f.cov_step(t, y[t]) for t in range(T)])
            ll = f.loglik
        else:
            f = ucr.vector_oracle(oracle, name, th, Z, n, ucr.SEED, 1, rs, sched, tile, T)
            ll, per = f.cov_run(y)
        st = f.state()
        st["x"] = np.asarray(st["x"]).reshape(m["dx"], n)
        _ORACLE[key] = (per, ll, st)
    return _ORACLE[key]


def _same_state(r, key, st, dx, what):
    n = st["cdf"].size
    np.testing.assert_array_equal(_bits(r[key + "_x"].reshape(dx, n)), _bits(st["x"]), err_msg=what + ": x, all planes")
    np.testing.assert_array_equal(_bits(r[key + "_logw"]), _bits(st["logw"]), err_msg=what + ": logw")
    np.testing.assert_array_equal(r[key + "_cdf"], st["cdf"], err_msg=what + ": cdf")
    np.testing.assert_array_equal(r[key + "_anc"], st["anc"], err_msg=what + ": ancestors")


@pytest.mark.parametrize("n,tile,sched,rs", CONFIGS)
@pytest.mark.parametrize("name", HEADERS)
def test_parity_with_the_oracle_closures(sa, oracle, spy, name, n, tile, sched, rs):
    """x (all planes), logw, cdf, ancestors, per-step and series log-likelihood are the oracle's bits: through step (covariates by
    value) and through run_series (covariates from the table); at N = 500 with the whole-series kernel on and off."""
    r, m = _run(name), ucr.MODELS[name]
    per, ll, st = _oracle(oracle, spy, name, n, tile, sched, rs)
    key = f"{n}_{tile}_{sched}_{rs}"
    np.testing.assert_array_equal(_bits(r[key + "_lls"]), _bits(per), err_msg="step API: log conditional likelihoods")
    _same_state(r, key + "_step", st, m["dx"], "step API")
    tags = ["_ser"] + (["_small"] if n <= 2048 and m["dx"] == 1 and m["dy"] == 1 else [])
    assert (key + "_small_ll" in r) == (len(tags) == 2)
    for tag in tags:
        np.testing.assert_array_equal(_bits(r[key + tag + "_per"][1]), _bits(per), err_msg=tag + ": per-step terms")
        np.testing.assert_array_equal(_bits(r[key + tag + "_ll"][1]), _bits(np.array([ll])), err_msg=tag + ": series log-likelihood")
        _same_state(r, key + tag, st, m["dx"], "run_series" + tag)
    assert not np.array_equal(r[key + "_lls"], r[key + "_ser_per"][0])        # filter 0 has other parameters


@pytest.mark.parametrize("n,tile", ucr.SHAPES)
@pytest.mark.parametrize("name", HEADERS)
def test_null_covariates_are_zeros(sa, oracle, spy, name, n, tile):
    """z = NULL gives the bits of z = zeros, by value and from the table -- and those of the oracle without covariates."""
    r, m = _run(name), ucr.MODELS[name]
    key = f"{n}_{tile}_1_0"
    for part in ("ser_ll", "lls", "ser_x", "ser_cdf", "ser_logw", "step_x", "step_cdf", "step_logw", "step_anc"):
        a, b = r[f"{key}_null_{part}"], r[f"{key}_zeros_{part}"]
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), part
    per, ll, st = _oracle(oracle, spy, name, n, tile, 1, 0, with_z=False)
    np.testing.assert_array_equal(_bits(r[key + "_null_lls"]), _bits(per))
    _same_state(r, key + "_null_step", st, m["dx"], "z = NULL")
    assert not np.array_equal(r[key + "_null_lls"], r[key + "_lls"])


@pytest.mark.parametrize("n,tile", ucr.SHAPES)
def test_the_pointer_grammar_draws_the_same_random_numbers(sa, n, tile):
    """The K = 1 restatement of the leverage model returns, from its own library, the bits svol_leverage_user.h's library returns."""
    a, b = _run("svol_leverage_cov1"), _run("leverage_plain")
    ka, kb = f"{n}_{tile}_1_0", f"{n}_{tile}"
    np.testing.assert_array_equal(_bits(a[ka + "_lls"]), _bits(b[kb + "_lls"]))
    np.testing.assert_array_equal(_bits(a[ka + "_ser_ll"]), _bits(b[kb + "_series"]))
    np.testing.assert_array_equal(_bits(a[ka + "_ser_per"]), _bits(b[kb + "_per"]))
    for part in ("x", "logw", "cdf", "anc"):
        for pa, pb in (("_step_", "_step_"), ("_ser_", "_ser_")):
            u, v = a[ka + pa + part], b[kb + pb + part]
            assert np.array_equal(u.view(np.uint64) if u.dtype == np.float64 else u, v.view(np.uint64) if v.dtype == np.float64 else v), part


def _check_functionals(oracle, name, dev, r, key, zc, n, tile, what):
    m = ucr.MODELS[name]
    st_dev = dict(x=r[key + "_x"], logw=r[key + "_logw"], cdf=r[key + "_cdf"], A=r[key + "_A"], mb=r[key + "_mb"], m=float(r[key + "_m"][0]))
    x = np.asarray(st_dev["x"]).reshape(m["dx"], n)
    st = er.make_state(oracle, dict(st_dev, x=x[0]), tile)
    h = ucr.h_rows(oracle, name, m["theta"][1], x, zc)
    eq = er.expect_fixed_point(h, st)
    bud = er.budget_fixed_point(h, st)
    assert dev.shape == (m["n_h"], 2)
    for k in range(m["n_h"]):
        err = float(abs(Fraction(float(dev[k, 1])) - eq[k]))
        print(what, name, key, "h", k, "device", dev[k, 1], "E_q", float(eq[k]), "error", err, "budget_fixed_point", bud[k])
        assert err <= bud[k], (what, k, dev[k, 1], float(eq[k]), err, bud[k])


@pytest.mark.parametrize("n,tile", ucr.SHAPES)
@pytest.mark.parametrize("name", [h for h in HEADERS if ucr.MODELS[h]["n_h"]])
def test_functionals_receive_the_covariates_of_the_last_step(sa, oracle, name, n, tile):
    """ssme_pf_get_user_expectations after a step with covariates, after a run_series with covariates (the last row's apply) and after
    a run_series with z = NULL (zeros), against the exact ratio on the downloaded state."""
    r, m = _run(name), ucr.MODELS[name]
    key, Z = f"{n}_{tile}_1_0", ucr.covariates(m["K"])
    _check_functionals(oracle, name, r[key + "_ue_step"], r, key + "_step", Z[T - 1], n, tile, "after step")
    _check_functionals(oracle, name, r[key + "_ue_series"], r, key + "_ser", Z[T - 1], n, tile, "after run_series")
    _check_functionals(oracle, name, r[key + "_ue_series_null"], r, key + "_null_ser", np.zeros(m["K"]), n, tile, "after run_series(z = NULL)")
    # a functional that reads a covariate moves with it
    assert not np.array_equal(r[key + "_ue_series"][m["n_h"] - 1], r[key + "_ue_series_null"][m["n_h"] - 1])


@pytest.mark.parametrize("n,tile", [(500, 2048), (2500, 512)])
@pytest.mark.parametrize("name", ["svol_reg_cov", "svol_two_factor_cov", "svol_leverage_cov1"])
def test_forecast_with_future_covariates(sa, oracle, name, n, tile):
    """ssme_pf_sim_future_obs_cov, H = 3, with states and start indices, is the numpy restatement's bits; two calls from one origin
    return the same bits; a filter step after the forecast returns what it returns without it."""
    r, m = _run(name), ucr.MODELS[name]
    key = f"fc_{n}"
    st = dict(x=r[key + "_state_x"], cdf=r[key + "_state_cdf"], A=r[key + "_state_A"], mb=r[key + "_state_mb"], rshift=int(r[key + "_state_rshift"][0]))
    start, xs, ys = ucr.forecast_cov(oracle, name, m["theta"][1], st, n, tile, ucr.SEED, 1, 4, r["Zf"])
    H = 3
    np.testing.assert_array_equal(r[key + "_start"][1], start)
    np.testing.assert_array_equal(_bits(r[key + "_x"][1].reshape(H, m["dx"], n)), _bits(xs))
    np.testing.assert_array_equal(_bits(r[key + "_y"][1].reshape(H, m["dy"], n)), _bits(ys))
    assert np.isfinite(ys).all()
    for part in ("_y", "_x", "_start"):
        a, b = r[key + part], r[key + part + "2"]
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), part
    np.testing.assert_array_equal(_bits(r[key + "_next_after"]), _bits(r[key + "_next_plain"]))
    for part in ("x", "logw", "cdf"):
        a, b = r[f"{key}_next_after_state_{part}"], r[f"{key}_next_plain_state_{part}"]
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), part


def test_contract_of_the_covariate_entry_points(sa):
    from ssme_amd import _capi
    r = _run("svol_reg_cov")
    assert r["fc_before_step"].tolist() == [_capi.ERR_STATE]
    assert r["fc_null_z"].tolist() == [_capi.ERR_INVALID_ARG]
    assert r["fc_num_steps"].tolist() == [_capi.ERR_INVALID_ARG] * 2
    assert r["fc_plain_on_cov"].tolist() == [_capi.ERR_UNSUPPORTED]                # ssme_pf_sim_future_obs on a dim_cov model
    assert r["fc_builtin"].tolist() == [_capi.ERR_UNSUPPORTED]                     # a model without dim_cov
    assert _run("leverage_plain")["fc_cov_status"].tolist() == [_capi.ERR_UNSUPPORTED]
    # a dim_cov header without the observation draw: it filters as svol_reg_cov_nofirst.h does, and cannot be forecast
    nd = _run("svol_reg_cov_nodraw")
    assert nd["fc_cov_status"].tolist() == [_capi.ERR_UNSUPPORTED]
    np.testing.assert_array_equal(_bits(nd["lls"]), _bits(_run("svol_reg_cov_nofirst")["500_2048_1_0_lls"]))
    assert r["shard_create"].tolist() == [_capi.ERR_UNSUPPORTED]
    # a `bad` filter: NaN samples, SSME_OK; the other filter of the handle is healthy
    assert r["fc_bad_status"].tolist() == [_capi.OK]
    assert np.isnan(r["fc_bad_y"][0]).all() and np.isfinite(r["fc_bad_y"][1]).all()
    # the stock library: no dim_cov, so the covariate forecast is unsupported
    bank = sa.ParticleFilterBank(sa.MODEL_SVOL, 500, 1, 1)
    bank.set_params([1.0, 0.95, 0.25])
    bank.step(0.3)
    with pytest.raises(_capi.SsmeError) as ei:
        bank.sim_future_obs(2, z_future=np.zeros((2, 1)))
    assert ei.value.status == _capi.ERR_UNSUPPORTED
    bank.close()


def test_f32_handles_round_all_covariates_on_entry(sa):
    """An SSME_F32 handle's outputs are floats and equal the double handle run on float-rounded y, z and theta."""
    r = _run("svol_reg_cov")
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    for k in ("lls", "ue", "series", "fc"):
        a, b = r["f32_" + k], r["f64r_" + k]
        assert np.all(np.isfinite(a)) and np.array_equal(a, f32(a)), k
        np.testing.assert_array_equal(_bits(a), _bits(f32(b)), err_msg=k)
    assert not np.array_equal(r["f64r_lls"], f32(r["f64r_lls"]))


def test_adaptor_equals_the_python_path(sa, spy, tmp_path):
    """user_bswc_gpu<500, 1, 1, 3>::filter(y, z, fs) and getModelExpectations() against ParticleFilterBank with the same seed and
    filter id (tests/cpp/test_user_cov_adaptor.cpp): log conditional likelihoods, device functionals, a forecast and the host
    functionals h(x, z) (the same sum over ParticleFilterBank.weights in the same order), all to the bit."""
    from test_user_cov_cpu import build_adaptor_program, cov_lib
    exe = build_adaptor_program()
    Z, y = ucr.covariates(3), ucr.observations(spy, 1)
    rows = tmp_path / "rows.txt"
    rows.write_text("".join("%r %r %r %r\n" % (float(y[t]), *(float(v) for v in Z[t])) for t in range(T)))
    out = subprocess.check_output([exe, str(rows)], text=True, timeout=600)
    vals = dict(line.split(" ", 1) for line in out.strip().splitlines())
    assert int(vals["dim_cov"]) == 3 and int(vals["has_first"]) == 1 and int(vals["short_covs_throw"]) == 1
    script = tmp_path / "py_path.py"
    script.write_text(
        "import sys, numpy as np\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nimport ssme_amd, user_cov_ref as ucr\n"
        "spy = np.loadtxt(%r)\nZ, y = ucr.covariates(3), ucr.observations(spy, 1)\n"
        "b = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 500, 1, 77, first_filter_id=1)\nb.set_params([0.9, 0.1, 0.3, -0.2, 0.25, -0.05])\n"
        "for t in range(%d): print('ll_%%d' %% t, float(b.step(y[t], Z[t])[0]).hex())\n"
        "ue = b.user_expectations()\nfor k in range(3): print('me_%%d' %% k, float(ue[k, 0]).hex())\n"
        "fc = b.sim_future_obs(2, z_future=[[0.5, -0.25, 1.0], [-1.5, 0.75, 0.125]])\n"
        "print('fc_size', fc.size); print('fc_0', float(fc.ravel()[0]).hex()); print('fc_last', float(fc.ravel()[-1]).hex())\n"
        "b.close()\nb = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, 500, 1, 77, first_filter_id=1)\nb.set_params([0.9, 0.1, 0.3, -0.2, 0.25, -0.05])\n"
        "for t in range(%d): b.step(y[t], Z[t])\n"
        "x, w = b.weights(0)\nn0 = n1 = den = 0.0\n"
        "for i in range(500):\n    n0 += float(x[i]) * float(w[i]); n1 += (float(x[i]) + 0.25 * float(Z[-1, 2])) * float(w[i]); den += float(w[i])\n"
        "print('host_0', (n0 / den).hex()); print('host_1', (n1 / den).hex())\n"
        % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "spy_returns.csv"), T, T))
    py = subprocess.check_output([sys.executable, str(script)], text=True, timeout=600, env=dict(os.environ, SSME_PF_LIB=cov_lib("svol_reg_cov")))
    want = dict(line.split(" ", 1) for line in py.strip().splitlines())
    assert len(want) == T + 3 + 3 + 2          # log conditional likelihoods, device functionals, forecast probes, host functionals
    for k, v in want.items():
        if k == "fc_size":
            assert int(vals[k]) == int(v)
        else:
            assert float.fromhex(vals[k].strip()) == float.fromhex(v.strip()), (k, vals[k], v)
    assert float.fromhex(vals["host_1"].strip()) != float.fromhex(vals["host_0"].strip())        # fs[1] reads z[2] of the step
