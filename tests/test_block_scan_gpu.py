"""block_scan_f64 (csrc/pf_kernels.h: the first element of a pair by subtraction, no lane-shifted copy of the wave scan).

tests/cpp/test_block_scan.hip carries a verbatim copy of the scan these lines replaced and compares the bits of every thread's incl and total
with it and with a host prefix sum, one workgroup per case, at NT = 64 .. 1024 threads and NK = 1, 2, 4 pairs per thread where NK NT / 64 <= 16:
all zero, all 2^41, one non-zero value at the first, the last and a wave-boundary position, random integers below 2^41 (dense and sparse)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(nt, nk) for nt in (64, 128, 256, 512, 1024) for nk in (1, 2, 4) if nk * nt // 64 <= 16]
SCAN_CASES = ["all-zero", "all-2p41", "one-first", "one-last", "one-wave-last", "one-wave-first", "random", "random-sparse"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """tests/cpp/test_block_scan.hip built (into pytest's temporary directory) and run once."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path_factory.mktemp("block_scan") / "test_block_scan")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_block_scan.hip"), "-o", exe], timeout=300)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr)
    scan, done = {}, None
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "scan":
            assert (w[2], w[4], w[6], w[8], w[10]) == ("nt", "nk", "values", "mismatch", "expect"), line
            scan[(w[1], int(w[3]), int(w[5]))] = (int(w[7]), int(w[9]), int(w[11]))
        elif w[0] == "done":
            done = int(w[1])
    assert done == len(scan), (done, len(scan))
    return scan


@pytest.mark.parametrize("nt,nk", SHAPES)
def test_block_scan_equals_the_shifted_form_and_the_host_sum(lines, nt, nk):
    scan = lines
    assert sorted(k[0] for k in scan if k[1:] == (nt, nk)) == sorted(SCAN_CASES)
    for name in SCAN_CASES:
        values, mismatch, expect = scan[(name, nt, nk)]
        assert values == 2 * nt * nk + nt, (name, nt, nk, values)
        assert mismatch == 0, f"{name} at NT = {nt}, NK = {nk}: {mismatch} values differ in bits from the form with the lane-shifted copy"
        assert expect == 0, f"{name} at NT = {nt}, NK = {nk}: {expect} values differ in bits from the host's prefix sum"
