"""The whole-series Liu-West route through the C ABI from C++ (tests/cpp/test_lw_series.cpp): route query, setter, run_series on both
routes with equal results.  Built the way tests/test_cpp_adaptor.py builds its programs; the CPU test only compiles and links."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_lw_series")


def _build():
    from ssme_amd import build
    so = build.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_lw_series.cpp"),
                           "-o", EXE, so, "-Wl,-rpath," + os.path.dirname(so)])
    return EXE


def test_lw_series_program_compiles_and_links():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_lw_series_c_abi_from_cpp():
    exe = _build()
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 2 + 2 * 9 and all(line.endswith(" ok") for line in lines), p.stdout
