"""GPU suite for the functionals a user model declares in its header (ssme_amd/csrc/model_api.h: n_h, h; kernels in
ssme_amd/csrc/user_expect.h): ssme_pf_get_user_expectations / ssme_pf_swarm_aggregate_user through ParticleFilterBank and through the
C++ adaptor.  Every model runs in a process of its own (tests/user_h_worker.py with SSME_PF_LIB), each with its own timeout.

Tolerances are those of test_expectations*: rtol 1e-12 for positive functionals; for the sign-changing ones (x1, x2, x1 x2) the same
1e-12 times sum |h w| / sum w, so that a mean near zero is not judged relatively."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "tests", "models")


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a HIP device"
    import ssme_amd
    return ssme_amd


def _lib(name):
    from ssme_amd import build
    return build.build_user_model(os.path.join(MODELS, {"student_t_h": "svol_student_t_h.h", "two_factor_h": "svol_two_factor_h.h"}[name]), name)


def _worker(name, mode, tmp_path, timeout=600):
    out = str(tmp_path / (mode + ".npz"))
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "user_h_worker.py"), mode, out], env=dict(os.environ, SSME_PF_LIB=_lib(name)),
                   check=True, timeout=timeout)
    return np.load(out)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_scalar_model_functionals_equal_the_built_ins(sa, tmp_path):
    """h = (x, x^2, exp(x / 2), 42) in user form against expectations_multi([0, 1, 2, 3]) of the same handle: N in {700, 5000}, R = 3,
    all four resamplers, resamp_sched in {1, 3}."""
    r = _worker("student_t_h", "scalar", tmp_path)
    for n in (700, 5000):
        for rs in (0, 1, 2, 3):
            for sched in (1, 3):
                key = f"{n}_{rs}_{sched}"
                ue, em = r["ue_" + key], r["em_" + key]
                assert ue.shape == (4, 3) and np.all(np.isfinite(ue)), key
                print(key, "max rel diff", np.max(np.abs(ue - em) / np.abs(em)), "42 row", np.max(np.abs(ue[3] - 42.0)))
                np.testing.assert_allclose(ue, em, rtol=1e-12, atol=0, err_msg=key)
                np.testing.assert_allclose(ue[3], 42.0, rtol=0, atol=1e-12, err_msg=key)


def _host_rows(x, w, z):
    x1, x2 = x[0], x[1]
    return [x1, x2, x1 * x1, x1 * x2, x2 * x2, np.exp(0.5 * (x1 + x2)), np.full_like(x1, z + 1.0)]


def test_vector_model_functionals_against_the_host_sum(sa, tmp_path):
    """Seven functionals of the whole two-component state against the host sum over bank.weights(r): one tile and several with a ragged
    last one, every tile size; the covariate row is z + 1; the x1 row is what SSME_H_X gives (component 0)."""
    r = _worker("two_factor_h", "vector", tmp_path)
    for n in (1000, 40000):
        for tile in (512, 1024, 2048):
            key = f"{n}_{tile}"
            ue, z = r["ue_" + key], float(r["z_" + key][0])
            assert ue.shape == (7, 2) and z != 0.0
            for f in range(2):
                x, w = r[f"x{f}_" + key], r[f"w{f}_" + key]
                for k, hv in enumerate(_host_rows(x, w, z)):
                    want = (hv * w).sum() / w.sum()
                    scale = (np.abs(hv) * w).sum() / w.sum()
                    print(key, "filter", f, "h", k, "dev", ue[k, f], "host", want, "err / scale", abs(ue[k, f] - want) / scale)
                    assert abs(ue[k, f] - want) <= 1e-12 * scale, (key, f, k, ue[k, f], want)
            np.testing.assert_allclose(ue[6], z + 1.0, rtol=1e-12, atol=0)
            np.testing.assert_allclose(ue[0], r["ex0_" + key], rtol=1e-12, atol=0)
            # after a whole series: the covariate of its last time index, or 0 without covariates
            np.testing.assert_allclose(r["ue_series_z_" + key][6], 3.5, rtol=1e-12, atol=0)
            np.testing.assert_allclose(r["ue_series_noz_" + key][6], 1.0, rtol=1e-12, atol=0)


def test_results_are_bitwise_reproducible(sa, tmp_path):
    """Two calls, 256 / 512 / 1024 threads per tile, and filter r of a bank against a one-filter handle with first_filter_id = r
    and n_filters_total = R: identical bits."""
    r = _worker("two_factor_h", "determinism", tmp_path)
    ref = r["a_512"]
    assert ref.shape == (7, 3) and np.all(np.isfinite(ref))
    for nt in (256, 512, 1024):
        np.testing.assert_array_equal(_bits(r[f"a_{nt}"]), _bits(r[f"b_{nt}"]), err_msg=f"two calls, {nt} threads")
        np.testing.assert_array_equal(_bits(r[f"a_{nt}"]), _bits(ref), err_msg=f"{nt} threads per tile")
    for f in range(3):
        np.testing.assert_array_equal(_bits(r[f"single_{f}"][:, 0]), _bits(ref[:, f]), err_msg=f"filter {f} in a handle of its own")
    assert not np.array_equal(ref[:, 0], ref[:, 1])


def test_swarm_means_as_the_reference_pool_computes_them(sa, tmp_path):
    """swarm_aggregate_user(0) and (num_threads = 3) over R = 7 members against the means formed from user_expectations() and the
    step's log conditional likelihoods, as test_swarm_aggregate_as_the_reference_pool_computes_it does for the built-ins."""
    r = _worker("two_factor_h", "swarm", tmp_path)
    R, T = 7, 3
    lcl, ex = r["lcl"], r["ue"]
    assert ex.shape == (7, R)
    plain_ll, plain_ex = float(r["ll_0"][0]), r["ex_0"]
    assert abs(plain_ll - lcl.mean()) <= 1e-14 * abs(lcl.mean())
    np.testing.assert_allclose(plain_ex, ex.mean(axis=1), rtol=1e-13, atol=0)
    ll3, ex3 = float(r["ll_3"][0]), r["ex_3"]
    groups = [np.arange(R)[np.arange(R) % T == j] for j in range(T)]
    want_ll = np.mean([lcl[g].mean() for g in groups])
    want_ex = [np.mean([ex[f][g].mean() for g in groups]) for f in range(7)]
    assert abs(ll3 - want_ll) <= 1e-13 * abs(want_ll)
    np.testing.assert_allclose(ex3, want_ex, rtol=1e-13, atol=0)
    assert abs(ll3 - plain_ll) > 1e-9 * abs(plain_ll)                       # 7 members on 3 threads: not the plain mean
    assert abs(ex3[2] - plain_ex[2]) > 1e-9 * abs(plain_ex[2])
    assert abs(float(r["ll_7"][0]) - plain_ll) <= 1e-14 * abs(plain_ll)
    np.testing.assert_allclose(r["ex_7"], plain_ex, rtol=1e-13, atol=0)


def test_contract_of_the_entry_points(sa, tmp_path):
    from ssme_amd import _capi
    # the stock library has no user model: unsupported
    bank = sa.ParticleFilterBank(sa.MODEL_SVOL, 1000, 1, 1)
    bank.set_params([1.0, 0.95, 0.25])
    bank.step(0.3)
    assert _capi.lib().ssme_pf_user_model_n_h() == 0
    for call in (bank.user_expectations, bank.swarm_aggregate_user):
        with pytest.raises(_capi.SsmeError) as ei:
            call()
        assert ei.value.status == _capi.ERR_UNSUPPORTED
    bank.close()
    r = _worker("student_t_h", "contract", tmp_path)
    assert r["before_step"].tolist() == [_capi.ERR_STATE] * 2
    assert r["sharded"].tolist() == [_capi.ERR_STATE] * 2
    assert r["builtin_model"].tolist() == [_capi.ERR_UNSUPPORTED] * 2
    for i in range(2):
        assert np.isnan(r[f"nan_ll_{i}"][0]) and r[f"nan_ue_{i}"].shape == (4, 1) and np.all(np.isnan(r[f"nan_ue_{i}"])), i
    for k in ("f32_ue", "f32_agg"):
        v = r[k]
        assert np.all(np.isfinite(v)) and np.array_equal(v, v.astype(np.float32).astype(np.float64)), k
    assert r["f32_ue"].shape == (4, 2) and np.all(r["f32_ue"][3] == 42.0)
    np.testing.assert_array_equal(_bits(r["ue_queued"]), _bits(r["ue_sync"]))
    np.testing.assert_array_equal(_bits(r["agg_queued"]), _bits(r["agg_sync"]))
    assert np.all(np.isfinite(r["ue_sync"])) and np.all(np.isfinite(r["agg_sync"]))


def test_adaptor_model_expectations_match_its_host_functionals(sa, spy):
    """user_bs_gpu<N, 2, 2>::getModelExpectations() against the same object's filter(y, fs) with the seven functions as host
    std::functions (tests/cpp/test_user_functionals.cpp)."""
    from test_user_functionals_cpu import build_adaptor_program
    exe = build_adaptor_program()
    out = subprocess.check_output([exe, os.path.join(ROOT, "tests", "golden", "spy_returns.csv")], text=True, timeout=600)
    vals = dict(line.split(" ", 1) for line in out.strip().splitlines())
    assert int(vals["n_h"]) == 7
    for k in range(7):
        dev, host, scale = float(vals[f"dev_{k}"]), float(vals[f"host_{k}"]), float(vals[f"scale_{k}"])
        print("h", k, "dev", dev, "host", host, "err / scale", abs(dev - host) / scale)
        assert abs(dev - host) <= 1e-12 * scale, (k, dev, host)
    assert abs(float(vals["dev_6"]) - 1.0) <= 1e-12     # filter(y) passes no covariate: z + 1 = 1
    assert vals["repeat"].strip() == "same"
