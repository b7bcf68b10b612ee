"""Recorded Liu-West series through the C ABI from C++ (tests/cpp/test_lw_series_expect.cpp): the setter's refusals, a recording run on
both routes with equal rows, the last row against ssme_lw_get_expectations, the [T][n][R] layout with a permuted id list.  Built the
way tests/test_lw_series_cpp_gpu.py builds its program; test_lw_series_expect_cpu.py compiles and links it without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_lw_series_expect")


def build_program():
    from ssme_amd import build
    so = build.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_lw_series_expect.cpp"),
                           "-o", EXE, so, "-Wl,-rpath," + os.path.dirname(so)])
    return EXE


@pytest.mark.gpu
def test_lw_series_expect_c_abi_from_cpp():
    exe = build_program()
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 2 + 2 * 10 and all(line.endswith(" ok") for line in lines), p.stdout
