"""CPU suite for user models with covariates (ssme_amd/csrc/model_api.h: dim_cov, first / first_logw) -- no device.

  * every new test header builds for gfx950 under build.py's resource check and reports what it declares (dim_cov, has_first,
    has_gsamp, n_h); the stock library and headers without dim_cov report 0;
  * dim_cov = 5, first without first_logw, and dim_cov with the scalar-zcov prop do not compile;
  * the reference method pins itself: oracle.UserVectorModelFilter at dx = dy = 1 with z = arange(T) equals oracle.UserModelFilter
    driven step by step, to the bit;
  * the numpy restatement of the covariate forecast reproduces forecast_user_ref for the K = 1 leverage restatement when Z_f[k] is the
    previous simulated observation of one particle;
  * a C++ program using user_bswc_gpu compiles and links against a covariate library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import forecast_user_ref as fur
import user_cov_ref as ucr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "models")
# header, dim_cov, has_first, has_gsamp, n_h, (dim_x, dim_y)
HEADERS = [("svol_reg_cov", 3, 1, 1, 3, (1, 1)), ("svol_reg_cov_nofirst", 3, 0, 1, 3, (1, 1)), ("svol_leverage_cov1", 1, 0, 1, 0, (1, 1)),
           ("svol_two_factor_cov", 4, 1, 1, 4, (2, 2)), ("svol_reg_cov_nodraw", 3, 0, 0, 0, (1, 1))]


def cov_lib(name):
    from ssme_amd import build
    return build.build_user_model(os.path.join(MODELS, name + ".h"), name)


def build_adaptor_program():
    """tests/cpp/test_user_cov_adaptor.cpp against the library built with tests/models/svol_reg_cov.h."""
    so = cov_lib("svol_reg_cov")
    exe = os.path.join(ROOT, "tests", "cpp", "test_user_cov_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_user_cov_adaptor.cpp"),
                           "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    return exe


@pytest.mark.parametrize("name,k,first,gsamp,n_h,dims", HEADERS)
def test_covariate_headers_build_and_report_what_they_declare(name, k, first, gsamp, n_h, dims):
    """build_user_model runs build.py's own check on every kernel of the library (no scratch memory, no VGPR spills)."""
    L = C.CDLL(cov_lib(name))
    assert L.ssme_pf_user_model_dim_cov() == k
    assert L.ssme_pf_user_model_has_first() == first
    assert L.ssme_pf_user_model_has_gsamp() == gsamp
    assert L.ssme_pf_user_model_n_h() == n_h
    dx, dy = C.c_int32(), C.c_int32()
    assert L.ssme_pf_user_model_dims(C.byref(dx), C.byref(dy)) == 0 and (dx.value, dy.value) == dims
    assert hasattr(L, "ssme_pf_sim_future_obs_cov")


def test_libraries_without_dim_cov_report_none():
    import ssme_amd
    from ssme_amd import build, _capi
    L = _capi.lib()
    assert L.ssme_pf_user_model_dim_cov() == 0 and L.ssme_pf_user_model_has_first() == 0                 # the stock library
    assert ssme_amd.user_model_dim_cov() == 0 and "user_model_dim_cov" in ssme_amd.filters.__all__
    for n in ("ssme_pf_user_model_dim_cov", "ssme_pf_user_model_has_first", "ssme_pf_sim_future_obs_cov"):
        assert n in _capi.EXPORTS and hasattr(L, n)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssme_pf.h")).read(), flags=re.S)
    for n in ("ssme_pf_user_model_dim_cov", "ssme_pf_user_model_has_first"):
        assert re.search(r"\bint\s+%s\s*\(\s*void\s*\)" % n, src)
    assert re.search(r"\bint\s+ssme_pf_sim_future_obs_cov\s*\(", src)
    for header, name in (("svol_student_t.h", "student_t"), ("svol_two_factor_g.h", "two_factor_g")):      # unchanged headers
        U = C.CDLL(build.build_user_model(os.path.join(MODELS, header), name))
        assert U.ssme_pf_user_model_dim_cov() == 0 and U.ssme_pf_user_model_has_first() == 0 and U.ssme_pf_user_model_n_theta() > 0


_WRAP = ('#pragma once\n#define ssme_user_model0 base_callbacks\n#include "%s"\n#undef ssme_user_model0\n'
         'struct ssme_user_model0 : base_callbacks {\n%s\n};\n')
_NEGATIVE = {
    # dim_cov out of range
    "dim_cov_5": ("svol_reg_cov_nofirst.h", "    static constexpr int dim_cov = 5;", "dim_cov of a user model: 1 .. 4"),
    # first without first_logw
    "first_alone": ("svol_reg_cov_nofirst.h",
                    "    static __device__ __forceinline__ void first(const ssme::ModelConst& c, const double* zn, const double*, const double*, double* x0,\n"
                    "                                                 const ssme::ExpTabEntry*) { x0[0] = c.a2 * zn[0]; }",
                    "both first and first_logw"),
    # dim_cov with the scalar-covariate prop of the other grammar
    "scalar_prop": ("svol_reg_cov_nofirst.h",
                    "    static __device__ __forceinline__ double prop(const ssme::ModelConst& c, double x, double zn, double zcov, const ssme::ExpTabEntry*) {\n"
                    "        return c.a0 * x + zn * c.a3 + zcov; }", None),
}


@pytest.mark.parametrize("case", sorted(_NEGATIVE))
def test_headers_outside_the_grammar_do_not_compile(tmp_path, case):
    from ssme_amd import build
    base, body, message = _NEGATIVE[case]
    hdr = tmp_path / (case + ".h")
    hdr.write_text(_WRAP % (os.path.join(MODELS, base), body))
    cmd = [build.hipcc()] + build.FLAGS + ['-DSSME_USER_MODEL_HEADER="%s"' % hdr] + build.SOURCES + ["-o", str(tmp_path / (case + ".so"))]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode != 0
    assert "error" in res.stdout
    if message:
        assert "static assertion failed" in res.stdout and message in res.stdout


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("rs,sched", [(0, 1), (1, 2)])
def test_the_two_oracles_agree_on_a_scalar_covariate_model(oracle, spy, rs, sched):
    """UserVectorModelFilter at dx = dy = 1 with z = arange(T) (the closures look Z[t] up) equals UserModelFilter driven step by step:
    per-step log-likelihood, x, cdf and ancestors at N = 500, T = 6 to the bit."""
    n, T, name = 500, ucr.T_STEPS, "svol_reg_cov_nofirst"
    y, Z, th = ucr.observations(spy, 1), ucr.covariates(3), ucr.TH_REG[1]
    a = ucr.scalar_oracle(oracle, name, th, Z, n, ucr.SEED, 1, rs, sched, 2048)
    lls = np.array([a.cov_step(t, y[t]) for t in range(T)])
    b = ucr.vector_oracle(oracle, name, th, Z, n, ucr.SEED, 1, rs, sched, 2048, T)
    ll, per = b.cov_run(y)
    assert np.array_equal(_bits(lls), _bits(per))
    sa, sb = a.state(), b.state()
    assert np.array_equal(_bits(sa["x"]), _bits(sb["x"][0]))
    assert np.array_equal(sa["cdf"], sb["cdf"]) and np.array_equal(sa["anc"], sb["anc"])
    # and the covariates matter: without them the log-likelihoods differ
    c = ucr.scalar_oracle(oracle, name, th, None, n, ucr.SEED, 1, rs, sched, 2048)
    assert not np.array_equal(lls, np.array([c.cov_step(t, y[t]) for t in range(T)]))


def _synthetic_state(rng, n, tile):
    q = rng.integers(1, 2 ** 41, size=n, dtype=np.int64)
    q[rng.random(n) < 0.3] = 0
    starts = np.arange(0, n, tile)
    for s in starts:
        q[s + rng.integers(0, min(tile, n - s))] = 2 ** 41
    cdf = np.concatenate([np.cumsum(q[s:s + tile]) for s in starts]).astype(np.uint64)
    npad = starts.size * tile
    return dict(x=rng.normal(size=n), cdf=cdf, A=np.add.reduceat(q, starts).astype(np.uint64), mb=-rng.random(starts.size) * 3.0,
                rshift=52 - int(np.ceil(np.log2(npad))))


@pytest.mark.parametrize("n,tile", [(501, 2048), (3 * 512 + 7, 512)])
def test_covariate_forecast_reference_reproduces_the_previous_observation_convention(oracle, n, tile):
    """The K = 1 restatement of the leverage model, fed per particle the previous simulated observation as Z_f[k], returns the bits of
    forecast_user_ref (whose covariate IS the previous simulated observation); fed the path of ONE particle as an exogenous series it
    reproduces that particle."""
    seed, rep, t0, H, th = 0x1234567887654321, 5, 4, 4, [0.95, -0.4, 0.3, -0.6]
    st = _synthetic_state(np.random.default_rng(n), n, tile)
    start, xs, ys = fur.forecast_user(oracle, "svol_leverage_user", th, st, n, tile, seed, rep, t0, H, last_obs=0.37)
    zf_all = [[np.full(n, 0.37)]] + [[ys[k - 1, 0]] for k in range(1, H)]
    s2, x2, y2 = ucr.forecast_cov(oracle, "svol_leverage_cov1", th, st, n, tile, seed, rep, t0, zf_all, per_particle=True)
    assert np.array_equal(start, s2) and np.array_equal(_bits(xs), _bits(x2)) and np.array_equal(_bits(ys), _bits(y2))
    i = n // 3
    zf = np.array([[0.37]] + [[ys[k - 1, 0, i]] for k in range(1, H)])
    s3, x3, y3 = ucr.forecast_cov(oracle, "svol_leverage_cov1", th, st, n, tile, seed, rep, t0, zf)
    assert np.array_equal(start, s3)
    assert np.array_equal(_bits(xs[:, :, i]), _bits(x3[:, :, i])) and np.array_equal(_bits(ys[:, :, i]), _bits(y3[:, :, i]))
    assert not np.array_equal(ys[1:], y3[1:])                      # other particles see another covariate


def test_adaptor_program_with_covariates_compiles():
    assert os.path.exists(build_adaptor_program())
