"""The smoothing kernels alone (ssme_amd/csrc/smooth.h), on histories written by hand: tests/cpp/test_smooth_kernels.hip is built once
with the library's code-generation flags and run once on the case file of tests/smooth_kernel_cases.py; everything is compared here.

  lineages   k_sm_trajectories<1..4>: states (all planes) and indices bit for bit against smooth_ref.genealogy with the clamp to N - 1,
             NaN states and in-range indices for a filter without weight;
  sweep (a)  k_sm_sweep<2|4|8>: on dyadic states and integer weights the tile numerators of the functionals 0, 1, 3 equal the integer
             reference bit for bit, and with equal tile maxima k_sm_final's rows equal one division of the exact sums;
  sweep (b)  every row t of k_sm_sweep / k_sm_final equals k_expect_partials / k_expect_final on the host's gather x_t[B_t(j)], bit for bit;
  poison     the run with NaN / 0xFFFFFFFF in every place the kernels must not look at equals the run with zeros there, bit for bit.
No tolerance anywhere: every comparison is of bits."""
import os
import subprocess

import numpy as np
import pytest

import smooth_kernel_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CASES = kc.cases()
NAMES = [c["name"] for c in CASES]
_RUN = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(got, want, what):
    """Bit for bit, NaN for NaN (a NaN's payload is not part of the contract); returns the number of values compared."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=what + ": NaN pattern")
    np.testing.assert_array_equal(_bits(got)[~gn], _bits(want)[~wn], err_msg=what)
    return got.size


def _run(tmp_path_factory):
    if "res" not in _RUN:
        try:
            import torch
            assert torch.cuda.is_available(), "GPU tests need a HIP device"
            from ssme_amd import build
            flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared") and not f.startswith("-Wl,")]
            assert {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-mfma", "-fno-fast-math"} <= set(flags)
            cpp = os.path.join(ROOT, "tests", "cpp")
            exe = os.path.join(cpp, "test_smooth_kernels")
            subprocess.check_call([build.hipcc()] + flags + [os.path.join(cpp, "test_smooth_kernels.hip"), "-o", exe])
            d = tmp_path_factory.mktemp("smooth_kernels")
            cases, out = str(d / "cases.bin"), str(d / "out.bin")
            kc.write_cases(cases, CASES)
            p = subprocess.run([exe, cases, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180)
            assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
            _RUN["res"] = dict(stdout=p.stdout, outs=kc.read_outputs(out, CASES))
        except BaseException as e:          # remembered, not retried: the program runs once
            _RUN["res"] = e
    if isinstance(_RUN["res"], BaseException):
        raise RuntimeError(f"the program failed and is not started again: {_RUN['res']!r}") from _RUN["res"]
    return _RUN["res"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return _run(tmp_path_factory)


def _pair(run, name):
    i = NAMES.index(name)
    return CASES[i], run["outs"][i]


def test_program_reported_every_case(run):
    lines = run["stdout"].split("\n")
    assert [l for l in lines if l.startswith("case ")] == [f"case {i} done" for i in range(2 * len(CASES))]
    assert f"all {2 * len(CASES)} done" in lines and len(run["outs"]) == len(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_lineages_bit_for_bit(run, name):
    """States of every plane and lineage indices of K given terminals; a filter without weight has NaN states and the same in-range
    indices as a live one would have (include/ssme_pf.h)."""
    c, outs = _pair(run, name)
    live = [r for r in range(c["R"]) if r not in c["dead"]]
    for o in outs:
        if c["states"] == "code":           # a wrong value says which (t, d, r, j) the kernel read
            bad = np.argwhere(o["x"][live] != c["x_ref"][live])
            assert not len(bad), (name, "at (r, k, t, d)", tuple(bad[0]), "the kernel read (t, d, r, j)",
                                  kc.decode(o["x"][live][tuple(bad[0])], c["dx"], c["R"], c["npad"]))
        np.testing.assert_array_equal(o["idx"], c["idx_ref"], err_msg=name + ": lineage indices")
        n = o["idx"].size + same_bits(o["x"], c["x_ref"], name + ": lineage states")
        assert n == c["R"] * c["K"] * c["T"] * (1 + c["dx"])
        assert (o["idx"] < c["N"]).all()
        for r in range(c["R"]):
            if r in c["dead"]:
                assert np.isnan(o["x"][r]).all(), (name, r)
            else:
                assert np.isfinite(o["x"][r]).all(), (name, r)


@pytest.mark.parametrize("name", NAMES)
def test_sweep_tree_for_tree(run, name):
    """smooth.h's claim: row t of k_sm_sweep / k_sm_final is what k_expect_partials / k_expect_final return for the array x_t[B_t(.)]
    with the final step's cdf, tile sums and maxima -- all four functionals, every state kind, zero tile scales and NaN maxima."""
    c, outs = _pair(run, name)
    B, nf = c["B"], len(c["fids"])
    for o in outs:
        n = same_bits(o["part"][:, :, :B, :], o["apart"][:, :, :B, :], name + ": tile numerators")
        n += same_bits(o["out"], o["aout"], name + ": rows")
        assert n == c["T"] * c["R"] * (B * 4 + nf)
        # tiles [B, Bs) belong to nobody: both kernels leave them as the program blanked them
        assert (_bits(o["part"][:, :, B:, :]) == 0xFFFFFFFFFFFFFFFF).all() and (_bits(o["apart"][:, :, B:, :]) == 0xFFFFFFFFFFFFFFFF).all()
        if c["tmax"] == "nan":
            assert np.isnan(o["out"][:, :, c["R"] - 1]).all() and np.isfinite(o["out"][:, :, :c["R"] - 1]).all(), name
        else:
            assert np.isfinite(o["out"]).all(), name


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["states"] == "dyadic"])
def test_sweep_exact_on_integers(run, name):
    """Dyadic states, integer weights: the numerators of the functionals 0, 1, 3 are exact in any order, so they equal the integer
    reference bit for bit (independent of any device arithmetic); with equal tile maxima the rows are one division of exact sums."""
    c, outs = _pair(run, name)
    want = kc.exact_parts(c)
    cols = [i for i, f in enumerate(c["fids"]) if f != 2]
    assert [c["fids"][i] for i in cols] == [0, 1, 3]
    for o in outs:
        n = same_bits(o["part"][:, :, :c["B"], :][..., cols], want[..., cols], name + ": exact numerators")
        assert n == c["T"] * c["R"] * c["B"] * 3
        if c["tmax"] == "equal":
            rows = kc.exact_out(c)
            assert same_bits(o["out"][:, cols, :], rows[:, cols, :], name + ": exact rows") == c["T"] * 3 * c["R"]


@pytest.mark.parametrize("name", NAMES)
def test_poison_changes_no_bit(run, name):
    """Columns [N, Npad), tiles [B, Bs) and the hanc rows no draw wrote: NaN / 0xFFFFFFFF there or zeros there, the same outputs."""
    c, (a, b) = _pair(run, name)
    n = 0
    for k in kc.sizes(c):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{name}: {k}")
        n += a[k].size
    assert n == sum(kc.sizes(c).values())
