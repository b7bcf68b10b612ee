"""CPU suite for the functionals a user model declares in its header (ssme_amd/csrc/model_api.h: n_h, h): the test models build
for gfx950 under build.py's resource checks, the libraries report their n_h, the bound on n_h is enforced at compile time, the
new C-ABI entry points are declared, exported and bound, and a C++ program using user_bs_gpu::getModelExpectations() compiles."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "models")
NEW = ("ssme_pf_user_model_n_h", "ssme_pf_get_user_expectations", "ssme_pf_swarm_aggregate_user")


def build_adaptor_program():
    """tests/cpp/test_user_functionals.cpp against the library built with tests/models/svol_two_factor_h.h."""
    from ssme_amd import build
    so = build.build_user_model(os.path.join(MODELS, "svol_two_factor_h.h"), "two_factor_h")
    exe = os.path.join(ROOT, "tests", "cpp", "test_user_functionals")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_user_functionals.cpp"),
                           "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    return exe


@pytest.mark.parametrize("header,name,n_h,dims", [("svol_student_t_h.h", "student_t_h", 4, (1, 1)), ("svol_two_factor_h.h", "two_factor_h", 7, (2, 2))])
def test_models_with_functionals_build_and_report_n_h(header, name, n_h, dims):
    """build_user_model runs build.py's own check on every kernel of the library, the new expectation kernels included: no scratch
    memory, no VGPR spills (it raises otherwise)."""
    from ssme_amd import build
    L = C.CDLL(build.build_user_model(os.path.join(MODELS, header), name))
    assert L.ssme_pf_user_model_n_h() == n_h
    dx, dy = C.c_int32(), C.c_int32()
    assert L.ssme_pf_user_model_dims(C.byref(dx), C.byref(dy)) == 0 and (dx.value, dy.value) == dims
    for n in NEW:
        assert hasattr(L, n)


def test_libraries_without_functionals_report_none():
    from ssme_amd import build, _capi
    assert _capi.lib().ssme_pf_user_model_n_h() == 0                         # the stock library
    L = C.CDLL(build.build_user_model(os.path.join(MODELS, "svol_two_factor.h"), "two_factor"))      # the unchanged header
    assert L.ssme_pf_user_model_n_h() == 0 and L.ssme_pf_user_model_n_theta() == 6


def test_more_than_16_functionals_do_not_compile(tmp_path):
    from ssme_amd import build
    hdr = tmp_path / "too_many.h"
    hdr.write_text('#pragma once\n#define ssme_user_model0 too_many_callbacks\n#include "%s"\n#undef ssme_user_model0\n'
                   'struct ssme_user_model0 : too_many_callbacks {\n    static constexpr int n_h = 17;\n'
                   '    static __device__ __forceinline__ void h(const ssme::ModelConst&, const double* x, double, const ssme::ExpTabEntry*, double* out) {\n'
                   '#pragma unroll\n        for (int k = 0; k < 17; ++k) out[k] = x[0];\n    }\n};\n' % os.path.join(MODELS, "svol_student_t.h"))
    cmd = [build.hipcc()] + build.FLAGS + ['-DSSME_USER_MODEL_HEADER="%s"' % hdr] + build.SOURCES + ["-o", str(tmp_path / "too_many.so")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode != 0
    assert "n_h of a user model: 1 .. 16" in res.stdout


def test_new_entry_points_are_declared_exported_and_bound():
    import re
    from ssme_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssme_pf.h")).read(), flags=re.S)
    L = _capi.lib()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert n in _capi.EXPORTS and hasattr(L, n)
    dp = C.POINTER(C.c_double)
    assert L.ssme_pf_user_model_n_h.argtypes in (None, [], ())
    assert list(L.ssme_pf_get_user_expectations.argtypes) == [C.c_void_p, dp]
    assert list(L.ssme_pf_swarm_aggregate_user.argtypes) == [C.c_void_p, C.c_int32, dp, dp]
    # argument checks come before any device call
    assert L.ssme_pf_get_user_expectations(None, None) == _capi.ERR_INVALID_ARG
    assert L.ssme_pf_swarm_aggregate_user(None, 0, None, None) == _capi.ERR_INVALID_ARG
    import ssme_amd
    assert callable(ssme_amd.ParticleFilterBank.user_expectations) and callable(ssme_amd.ParticleFilterBank.swarm_aggregate_user)


def test_adaptor_program_with_model_expectations_compiles():
    assert os.path.exists(build_adaptor_program())
