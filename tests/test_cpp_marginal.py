"""The marginal smoothing methods of the C++ evaluators (include/ssme_gpu/bsfilter_gpu.hpp: smoothing_weights,
marginal_smoothed_expectations): tests/cpp/test_marginal.cpp compiles with g++ against the C ABI (on CPU: tests/test_marginal_cpu.py);
on the GPU it compares what the methods return with the bits of a handle driven through the C ABI alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_marginal")
LINES = ("logliks", "means", "weights_first_step", "weights_last_step", "last_row_is_final_weights", "first_row_has_spread",
         "second_evaluation_differs", "off_refuses")


def build_program():
    from ssme_amd import build
    so = build.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_marginal.cpp"),
                           "-o", EXE, so, "-Wl,-rpath," + os.path.dirname(so)])
    return EXE


@pytest.mark.gpu
def test_evaluator_marginal_smoothing_equals_c_abi_bits():
    exe = build_program()
    out = subprocess.check_output([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], text=True, timeout=120)
    vals = dict(line.split(" ", 1) for line in out.strip().splitlines())
    assert {k: vals.get(k, "missing").strip() for k in LINES} == {k: "ok" for k in LINES}, out
