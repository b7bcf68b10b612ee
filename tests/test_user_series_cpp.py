"""ssme_gpu::user_log_like_evaluator (include/ssme_gpu/bsfilter_gpu.hpp) through tests/cpp/test_user_series.cpp: the program compiles
with -Wall -Wextra against the libraries of svol_two_factor.h and svol_two_factor_cov.h, its argument checks throw what the header
says (no device needed), and on the device its replicates' log-likelihoods and its log-mean-exp are ParticleFilterBank's at the same
seed, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import user_cov_ref as ucr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = (("two_factor", "svol_two_factor", 0), ("svol_two_factor_cov", "svol_two_factor_cov", 4))
T, SEED, N, R = 24, 987654321, 500, 4
THETA = [1.1, 0.95, 0.9, 0.2, 0.15, -0.4]


def build_program(lib, header, k):
    from ssme_amd import build
    so = build.build_user_model(os.path.join(ROOT, "tests", "models", header + ".h"), lib)
    exe = os.path.join(ROOT, "tests", "cpp", f"test_user_series_{lib}")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", f"-DDIMCOV={k}", os.path.join(ROOT, "tests", "cpp", "test_user_series.cpp"),
                          "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and not out.stdout.strip(), out.stdout
    return exe, so


@pytest.mark.parametrize("lib,header,k", LIBS)
def test_program_compiles_clean_and_argument_checks_throw(lib, header, k):
    exe, _ = build_program(lib, header, k)
    vals = dict(line.split() for line in subprocess.check_output([exe], text=True, timeout=60).strip().splitlines())
    assert vals == {"wrong_dimx_throws": "1", "wrong_dimcov_throws": "1", "empty_throws": "1", "ragged_throws": "1"}


@pytest.mark.gpu
@pytest.mark.parametrize("lib,header,k", LIBS)
def test_evaluator_equals_the_python_path(lib, header, k, spy, tmp_path):
    exe, so = build_program(lib, header, k)
    y = ucr.observations(spy, 2, T)
    Z = ucr.covariates(k, T) if k else None
    rows = tmp_path / "rows.txt"
    rows.write_text("".join(" ".join(repr(float(v)) for v in (list(y[t]) + (list(Z[t]) if k else []))) + "\n" for t in range(T)))
    got = dict(line.split() for line in subprocess.check_output([exe, str(rows), str(SEED)], text=True, timeout=120).strip().splitlines())
    assert int(got["rows"]) == T and int(got["device_ms_positive"]) == 1
    assert (int(got["route"]), int(got["threads"])) == (1, 512)            # SSME_ROUTE_SERIES_LANE: one launch per evaluation
    script = tmp_path / "py_path.py"
    script.write_text(
        "import sys, numpy as np\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nimport ssme_amd, user_cov_ref as ucr\n"
        "spy = np.loadtxt(%r)\ny = ucr.observations(spy, 2, %d)\nZ = ucr.covariates(%d, %d) if %d else None\n"
        "b = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, %d, %d)\nb.set_seed(%d)\nb.set_params(%r)\n"
        "ll = b.run_series(y, Z)\nfor r in range(%d): print('ll_%%d' %% r, float(ll[r]).hex())\nprint('lme', b.log_mean_exp().hex())\n"
        "print('route', *b.series_route())\n"
        % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "spy_returns.csv"), T, k, T, k, N, R, SEED, THETA, R))
    py = subprocess.check_output([sys.executable, str(script)], text=True, timeout=120, env=dict(os.environ, SSME_PF_LIB=so))
    want = dict(line.split(" ", 1) for line in py.strip().splitlines())
    assert want["route"].split() == ["1", "512"]
    for key in [f"ll_{r}" for r in range(R)] + ["lme"]:
        a, b = float.fromhex(got[key]), float.fromhex(want[key].strip())
        assert np.isfinite(a) and a == b, (key, got[key], want[key])
    assert len({got[f"ll_{r}"] for r in range(R)}) == R, "replicates differ"
