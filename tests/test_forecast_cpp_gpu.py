"""Forecasts through the header-only C++ adaptor (include/ssme_gpu/bsfilter_gpu.hpp; tests/cpp/test_forecast.cpp): member
sim_future_obs and swarm simFutureObs return the bits of the C ABI call, in the shape [member][time][particle].  Built the way
tests/test_cpp_adaptor.py builds its programs; the CPU test only compiles and links."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_forecast")
NAMES = ["svol_leverage_gpu", "svol_bs_member_gpu", "swarm_context members", "svol_lw_1_par_gpu", "svol_lw_2_par_gpu", "swarm_with_covs_gpu",
         "swarm_gpu", "swarm_context lagging member"]


def _build():
    from ssme_amd import build
    so = build.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_forecast.cpp"),
                           "-o", EXE, so, "-Wl,-rpath," + os.path.dirname(so)])
    return EXE


def test_forecast_adaptor_compiles_and_links():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_forecast_adaptor_returns_the_c_abi_bits():
    exe = _build()
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout
    assert p.stdout.strip().splitlines() == [n + " ok" for n in NAMES], p.stdout
