"""block_max_nanprop / wave_max_f64 (csrc/pf_kernels.h: one barrier, the NaN flag in the wave's own LDS slot, v_max_f64 without the
canonicalising pair) and the level-2 head of k_filter_step at its entry counts.

tests/cpp/test_block_max.hip carries a verbatim copy of the form these functions replaced (dmaxnum, __syncthreads_or) and compares the
bits of every thread's return value, one workgroup per case, at 64, 128, 256, 512 and 1024 threads: all -inf; one finite value at thread
0, 63, 64, NT - 64, NT - 1; +inf; one flag at each of those threads among finite values, the flag in every thread (dnan() = 0x7ff8000000000000
exactly); -0 and +0 in two waves and in adjacent lanes of one wave, both orders; denormals; a seeded random fill with and without 1 % flags;
and 256 calls in one launch on two alternating LDS buffers with inputs that change per call (the reuse of a buffer across ONE barrier).

Through the filter: one case per level-2 entry count of the step kernel's head (2048 / NT = 4 entries per thread at NT = 512; legs e >= 1 are
uniform branches that a filter of at most NT tiles never enters): B = 512 (every entry in leg 0, the flagship shape), 513 (one entry in leg 1)
and 1024 (leg 1 full), the in-kernel level-2 forced, per-step log-likelihoods equal to the oracle's with ==.  The NaN / -inf maxima and the
other tile sizes are pinned by test_bootstrap_edges_gpu.py, test_liu_west_edges_gpu.py, test_long_series_gpu.py and the one-tile tests."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTS = (64, 128, 256, 512, 1024)
SPOT_CASES = ["single-finite-%d" % s for s in range(5)] + ["single-flag-%d" % s for s in range(5)]
CASES = ["all-neginf", "posinf", "posinf-among-neginf", "flag-with-posinf", "all-flags", "all-flags-all-neginf", "zeros-one-wave-neg-first",
         "zeros-one-wave-pos-first", "zeros-row-edge", "zeros-row-edge-rev", "negzero-only", "all-negzero", "denormals", "denormal-max-in-normals",
         "negative-denormals", "random", "random-flags-1pct", "loop-256"] + SPOT_CASES
TWO_WAVE_CASES = ["zeros-two-waves-neg-first", "zeros-two-waves-pos-first", "zeros-two-waves-mid"]          # blocks of more than one wave


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None        # the in-tree HIP library is what runs
    return ssme_amd


@pytest.fixture(scope="module")
def block_max_lines(tmp_path_factory):
    """tests/cpp/test_block_max.hip built (into pytest's temporary directory) and run once:
    {(case, NT): (threads, mismatches against the old form, mismatches against the host)}."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = str(tmp_path_factory.mktemp("block_max") / "test_block_max")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                           "-Wno-unused-value", "-Wno-unused-result", os.path.join(cpp, "test_block_max.hip"), "-o", exe], timeout=300)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr)
    out, done = {}, None
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            assert (w[2], w[4], w[6], w[8]) == ("nt", "threads", "mismatch", "expect"), line
            out[(w[1], int(w[3]))] = (int(w[5]), int(w[7]), int(w[9]))
        elif w[0] == "done":
            done = int(w[1])
    assert done == len(out), (done, len(out))
    return out


@pytest.mark.parametrize("nt", NTS)
def test_block_max_equals_the_three_barrier_form_in_every_thread(block_max_lines, nt):
    names = CASES + (TWO_WAVE_CASES if nt > 64 else [])
    assert sorted(k[0] for k in block_max_lines if k[1] == nt) == sorted(names)
    for name in names:
        threads, mismatch, expect = block_max_lines[(name, nt)]
        assert threads == nt * (256 if name == "loop-256" else 1), (name, nt, threads)
        assert mismatch == 0, f"{name} at {nt} threads: {mismatch} return values differ in bits from the dmaxnum / __syncthreads_or form"
        assert expect == 0, f"{name} at {nt} threads: {expect} return values are not the expected maximum / dnan()"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,T,tiles", [(1 << 20, 4, 512), ((1 << 20) + 2048, 3, 513), (1 << 21, 3, 1024)])
def test_level2_head_entry_counts_match_the_oracle(sa, oracle, spy, n, T, tiles):
    y = spy[:T]
    th = [1.0, 0.95, 0.25]
    b = sa.ParticleFilterBank(sa.MODEL_SVOL, n, 1, 20260101, tile=2048)
    assert (b.tile, b.n_tiles) == (2048, tiles)
    b.set_debug(False, False, split_level2=False)
    b.set_params(th)
    ll = b.run_series(y)[0]
    per = b.per_step()[0][:T].copy()
    b.close()
    lo, po = oracle.Filter(oracle.MODEL_SVOL, n, th, 20260101, rep=0, tile=2048).run_series(y)
    assert np.all(np.isfinite(po))
    assert np.all(per == po) and np.array_equal(_bits(per), _bits(po)), (tiles, per.tolist(), po.tolist())
    assert ll == lo
