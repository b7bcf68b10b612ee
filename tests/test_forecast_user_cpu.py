"""CPU suite for forecasts of user models (ssme_amd/csrc/model_api.h: gsamp / gsamp_vec) -- no device.

  * every test header that declares the draw builds for gfx950 under build.py's resource check (no scratch memory, the
    dim_x = dim_y = 4 horizon kernel included) and reports ssme_pf_user_model_has_gsamp() == 1; headers without it and the stock
    library report 0;
  * the new query is declared, exported and bound;
  * a vector header that declares only the scalar gsamp does not compile, and the message names gsamp_vec;
  * the reference (tests/forecast_user_ref.py) returns the bits of forecast_ref.forecast_bs for the leverage model, and draws the
    eight normals of a (4, 4) particle from words 0-1 and 2-3 of streams 161 and 164;
  * a C++ program using user_bs_gpu<N, 2, 2>::sim_future_obs compiles and links against the two-factor library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import forecast_ref as fr
import forecast_user_ref as fur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "models")
SEED = 0x1234567887654321
WITH_DRAW = [("svol_leverage_user.h", "leverage_user", (1, 1)), ("svol_two_factor_g.h", "two_factor_g", (2, 2)),
             ("svol_two_factor_lev_g.h", "two_factor_lev_g", (2, 2)),
             ("lin_gauss_3d_g.h", "lin_gauss_3d_g", (3, 1)), ("lin_gauss_4d_g.h", "lin_gauss_4d_g", (4, 4))]


def build_adaptor_program():
    """tests/cpp/test_user_forecast.cpp against the library built with tests/models/svol_two_factor_g.h."""
    from ssme_amd import build
    so = build.build_user_model(os.path.join(MODELS, "svol_two_factor_g.h"), "two_factor_g")
    exe = os.path.join(ROOT, "tests", "cpp", "test_user_forecast")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_user_forecast.cpp"),
                           "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    return exe


@pytest.mark.parametrize("header,name,dims", WITH_DRAW)
def test_models_with_the_draw_build_and_report_it(header, name, dims):
    """build_user_model runs build.py's own check on every kernel of the library, k_fc_start_vec and k_fc_horizon_user included: no
    scratch memory, no VGPR spills (it raises otherwise)."""
    from ssme_amd import build
    L = C.CDLL(build.build_user_model(os.path.join(MODELS, header), name))
    assert L.ssme_pf_user_model_has_gsamp() == 1
    dx, dy = C.c_int32(), C.c_int32()
    assert L.ssme_pf_user_model_dims(C.byref(dx), C.byref(dy)) == 0 and (dx.value, dy.value) == dims


def test_libraries_without_the_draw_report_none():
    from ssme_amd import build, _capi
    assert _capi.lib().ssme_pf_user_model_has_gsamp() == 0                   # the stock library
    for header, name in (("svol_student_t.h", "student_t"), ("svol_two_factor.h", "two_factor")):      # the unchanged headers
        L = C.CDLL(build.build_user_model(os.path.join(MODELS, header), name))
        assert L.ssme_pf_user_model_has_gsamp() == 0 and L.ssme_pf_user_model_n_theta() > 0


def test_the_query_is_declared_exported_and_bound():
    import ssme_amd
    from ssme_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssme_pf.h")).read(), flags=re.S)
    n = "ssme_pf_user_model_has_gsamp"
    assert re.search(r"\bint\s+%s\s*\(\s*void\s*\)" % n, src)
    L = _capi.lib()
    assert n in _capi.EXPORTS and hasattr(L, n)
    assert L.ssme_pf_user_model_has_gsamp.argtypes in (None, [], ()) and L.ssme_pf_user_model_has_gsamp.restype is C.c_int
    assert ssme_amd.user_model_has_gsamp() is False and "user_model_has_gsamp" in ssme_amd.filters.__all__


def test_a_vector_model_with_the_scalar_form_does_not_compile(tmp_path):
    from ssme_amd import build
    hdr = tmp_path / "wrong_form.h"
    hdr.write_text('#pragma once\n#define ssme_user_model0 wrong_form_callbacks\n#include "%s"\n#undef ssme_user_model0\n'
                   'struct ssme_user_model0 : wrong_form_callbacks {\n'
                   '    static __device__ __forceinline__ double gsamp(const ssme::ModelConst&, double x, double zo, const ssme::ExpTabEntry*) { return x + zo; }\n'
                   '};\n' % os.path.join(MODELS, "svol_two_factor.h"))
    cmd = [build.hipcc()] + build.FLAGS + ['-DSSME_USER_MODEL_HEADER="%s"' % hdr] + build.SOURCES + ["-o", str(tmp_path / "wrong_form.so")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode != 0
    assert "static assertion failed" in res.stdout and "gsamp_vec" in res.stdout


def _synthetic_state(rng, n, tile, dx=1):
    """A filter's download with random integer weights: x, tile-local cdf, tile sums, tile maxima, the level-2 fixed point."""
    q = rng.integers(1, 2 ** 41, size=n, dtype=np.int64)
    q[rng.random(n) < 0.3] = 0
    starts = np.arange(0, n, tile)
    for s in starts:
        q[s + rng.integers(0, min(tile, n - s))] = 2 ** 41
    cdf = np.concatenate([np.cumsum(q[s:s + tile]) for s in starts]).astype(np.uint64)
    npad = starts.size * tile
    x = rng.normal(size=n) if dx == 1 else rng.normal(size=(dx, n))
    return dict(x=x, cdf=cdf, A=np.add.reduceat(q, starts).astype(np.uint64), mb=-rng.random(starts.size) * 3.0,
                rshift=52 - int(np.ceil(np.log2(npad))))


@pytest.mark.parametrize("n,tile,H", [(1, 2048, 3), (501, 2048, 5), (3 * 512 + 7, 512, 2)])
def test_reference_returns_the_bits_of_the_built_in_leverage_reference(oracle, n, tile, H):
    rng = np.random.default_rng(n)
    st = _synthetic_state(rng, n, tile)
    th = [0.95, -0.4, 0.3, -0.6]
    a = fr.forecast_bs(oracle, fr.MODEL_SVOL_LEVERAGE, th, st, n, tile, SEED, 5, 4, H, last_obs=0.37)
    b = fur.forecast_user(oracle, "svol_leverage_user", th, st, n, tile, SEED, 5, 4, H, last_obs=0.37)
    assert np.array_equal(a[0], b[0])
    assert b[1].shape == (H, 1, n) and b[2].shape == (H, 1, n) and np.isfinite(b[2]).all()
    assert np.array_equal(a[1].view(np.uint64), b[1][:, 0].view(np.uint64))
    assert np.array_equal(a[2].view(np.uint64), b[2][:, 0].view(np.uint64))


def test_reference_draws_eight_normals_from_two_calls(oracle):
    """(4, 4): zs[0], zo[0] = words 0-1 and zs[1], zo[1] = words 2-3 of stream 161; zs[2], zo[2] and zs[3], zo[3] the same of stream
    164.  The first pair is forecast_ref.horizon_normals; the others come from one explicit Philox call each."""
    i, t0, rep, k = np.array([0, 1, 77, 6150]), 4, 5, 3
    zs, zo = fur.user_normals(oracle, i, t0, rep, k, SEED, 4)
    assert len(zs) == 4 and len(zo) == 4
    a, b = fr.horizon_normals(oracle, i, t0, rep, k, SEED)
    assert np.array_equal(zs[0], a) and np.array_equal(zo[0], b)
    assert fur.STREAM_SIM2 == 164 and fr.STREAM_SIM == 161
    for c, stream in enumerate((161, 164)):
        w = fr.philox4x32_10(i, t0, rep, stream + (k << 8), SEED & 0xffffffff, SEED >> 32)
        for half in (0, 1):
            a, b = fr.pair_normals(oracle, w[:, 2 * half], w[:, 2 * half + 1])
            assert np.array_equal(zs[2 * c + half], a) and np.array_equal(zo[2 * c + half], b)
    flat = np.stack(zs + zo)
    assert np.unique(flat).size == flat.size                                  # eight different numbers per particle
    # fewer components: a prefix of the same numbers, and no second call below three
    for dm in (1, 2, 3):
        s, o = fur.user_normals(oracle, i, t0, rep, k, SEED, dm)
        assert len(s) == dm and all(np.array_equal(s[d], zs[d]) and np.array_equal(o[d], zo[d]) for d in range(dm))


def test_reference_of_a_dead_filter_is_nan(oracle):
    st = dict(cdf=np.zeros(7, dtype=np.uint64), A=np.zeros(1, dtype=np.uint64), mb=np.array([-np.inf]), rshift=41, x=np.zeros((2, 7)))
    start, x, y = fur.forecast_user(oracle, "svol_two_factor_g", [1.1, 0.95, 0.9, 0.2, 0.15, -0.4], st, 7, 2048, SEED, 0, 3, 2)
    assert not start.any() and x.shape == (2, 2, 7) and np.isnan(x).all() and np.isnan(y).all()


def test_adaptor_program_with_sim_future_obs_compiles():
    assert os.path.exists(build_adaptor_program())
