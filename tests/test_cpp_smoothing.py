"""The smoothing methods of the C++ evaluators (include/ssme_gpu/bsfilter_gpu.hpp: record_history, sample_trajectories,
smoothed_expectations): tests/cpp/test_smoothing.cpp compiles with g++ against the C ABI (on CPU: tests/test_smoothing_cpu.py); on the GPU it compares what the
methods return with the bits of a handle driven through the C ABI alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_smoothing")
LINES = ("log_mean_exp", "logliks", "trajectories", "smoothed", "terminal_is_forecast_start", "last_row_is_filtered",
         "second_evaluation_differs", "off_refuses")


def _build():
    from ssme_amd import build
    so = build.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_smoothing.cpp"),
                           "-o", EXE, so, "-Wl,-rpath," + os.path.dirname(so)])
    return EXE


@pytest.mark.gpu
def test_evaluator_smoothing_equals_c_abi_bits():
    exe = _build()
    out = subprocess.check_output([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], text=True, timeout=120)
    vals = dict(line.split(" ", 1) for line in out.strip().splitlines())
    assert {k: vals.get(k, "missing").strip() for k in LINES} == {k: "ok" for k in LINES}, out
