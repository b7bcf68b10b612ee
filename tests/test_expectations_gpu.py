"""The kernels that turn a filter's state into what callers read -- getExpectations(), the swarm aggregate, the Liu-West parameter
means, the downloadable weights -- against the exact reference of tests/expect_ref.py, at the shapes of tests/expect_cases.py.

Every case first bit-compares the particles and the integer cdf with the oracle, so that a failure below is the expectation kernels'.
Then every expectation is compared with E_q (the same fixed-point weights, exact arithmetic) within budget_sum -- the summation tree --
and with the unquantised E_exact within budget_sum + budget_fixed_point -- the fixed-point specification.  The budgets are derived in
expect_ref.py; each case prints `BUDGET name error budget k`.  No case runs in debug mode."""
import os
from fractions import Fraction

import numpy as np
import pytest

import expect_cases as ec
import expect_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None
    return ssme_amd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def record(name, err, budget, k):
    print(f"BUDGET {name} error {float(err):.3e} budget {float(budget):.3e} ratio {float(err) / float(budget) if budget else 0.0:.3f} k {k}")


def check_rows(name, dev, h, st, kernel, tile=None):
    """dev[k] against E_q within budget_sum and against E_exact within budget_sum + budget_fixed_point, for every row of h."""
    tile = st["tile"] if tile is None else tile
    B = st["A"].size
    k = er.k_sum(tile, B, kernel)
    eq, ex = er.expect_fixed_point(h, st), er.expect_exact_weights(h, st)
    bs = er.budget_sum(tile, B, kernel, er.s_abs(h, st))
    bfp = er.budget_fixed_point(h, st, ex)
    bad = []
    for i in range(len(h)):
        e_q = float(abs(Fraction(float(dev[i])) - eq[i])) if isinstance(eq[i], Fraction) else abs(float(np.longdouble(dev[i]) - eq[i]))
        e_x = abs(float(np.longdouble(dev[i]) - ex[i]))
        record(f"{name} h{i} vs E_q", e_q, bs[i], k)
        record(f"{name} h{i} vs E_exact", e_x, bs[i] + bfp[i], k)
        if not (e_q <= bs[i] and e_x <= bs[i] + bfp[i]):
            bad.append((i, float(dev[i]), e_q, bs[i], e_x, bfp[i]))
    assert not bad, (name, bad)


def check_weights(name, w_dev, oracle, st):
    want = er.weights_ref(oracle, st)
    tol = er.k_sum(st["tile"], 1, "weights") * er.U * want + 2.0 ** -1074
    err = np.abs(w_dev - want)
    worst = np.argmax(err - tol)
    record(f"{name} weights()", err[worst], tol[worst] if tol[worst] else 1.0, 2)
    assert (err <= tol).all(), (name, worst, w_dev[worst], want[worst])


def compare_state(bank, f, of, tile, what):
    g, o = bank.state(f, logw=False), of.state()
    np.testing.assert_array_equal(_bits(g["x"]), _bits(o["x"]), err_msg=what + ": particles")
    np.testing.assert_array_equal(g["cdf"], o["cdf"], err_msg=what + ": integer cdf")
    np.testing.assert_array_equal(g["A"], o["A"], err_msg=what + ": tile sums")
    np.testing.assert_array_equal(_bits(g["mb"]), _bits(o["mb"]), err_msg=what + ": tile maxima")
    assert _bits([g["m"]])[0] == _bits([o["m"]])[0], what + ": maximum"
    return o


def check_bank(sa, oracle, bank, ofs, tile, name):
    """Everything the bootstrap entry points offer, for every filter of the bank."""
    em = bank.expectations_multi([0, 1, 2, 3])
    perm = bank.expectations_multi([3, 0, 2, 1])
    for row, kind in enumerate((3, 0, 2, 1)):
        np.testing.assert_array_equal(_bits(perm[row]), _bits(em[kind]), err_msg=name + ": multi, another order")
        np.testing.assert_array_equal(_bits(bank.expectations(kind)), _bits(em[kind]), err_msg=name + ": single == multi")
    for r, of in enumerate(ofs):
        st = er.make_state(oracle, compare_state(bank, r, of, tile, f"{name} r={r}"), tile)
        assert bank.tile == tile
        check_rows(f"{name} r={r}", em[:, r], ec.builtin_rows(oracle, st["x"]), st, "expect")
        x, w = bank.weights(r)
        np.testing.assert_array_equal(_bits(x), _bits(st["x"]), err_msg=name + ": weights() particles")
        check_weights(f"{name} r={r}", w, oracle, st)
    return em


def make_bank(sa, case):
    bank = sa.ParticleFilterBank(case["model"], case["n"], case["R"], case["seed"], case["rs"], case["sched"], tile=case["tile"])
    bank.set_params(np.asarray(case["theta"], dtype=np.float64))
    return bank


@pytest.mark.parametrize("case", ec.bootstrap_cases(), ids=lambda c: c["name"])
def test_bootstrap_expectations_step_api(sa, oracle, case):
    bank = make_bank(sa, case)
    y, z = ec.observations(case)
    done = 0
    for t, tile, ofs, lls in ec.walk_oracle(oracle, case):
        while done <= t:
            got = bank.step(y[done], None if z is None else z[done])
            done += 1
        np.testing.assert_array_equal(_bits(got), _bits(lls), err_msg=f"{case['name']} t={t}: log conditional likelihoods")
        check_bank(sa, oracle, bank, ofs, tile, f"{case['name']} t={t}")
    bank.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", ec.series_cases(), ids=lambda c: c["name"])
def test_bootstrap_expectations_after_a_series(sa, oracle, case, graph):
    """run_series leaves the handle at buffer index T & 1: even and odd T, captured graph and eager launches, the one-launch small-series
    kernel (N <= 2048) and the tiled kernel -- against the oracle after the same series, and bit for bit against the step API."""
    y, _ = ec.observations(case)
    bank = make_bank(sa, case)
    bank.set_graph_mode(graph)
    ll = bank.run_series(y)
    for _, tile, ofs, _ in ec.walk_oracle(oracle, case):
        pass
    assert ll[0] == ofs[0].loglik
    em = check_bank(sa, oracle, bank, ofs, tile, f"{case['name']} {'graph' if graph else 'eager'}")
    ll2 = bank.run_series(y)                                        # a second pass on the same handle (graph replay)
    assert ll2[0] == ll[0]
    np.testing.assert_array_equal(_bits(bank.expectations_multi([0, 1, 2, 3])), _bits(em), err_msg="second pass")
    steps = make_bank(sa, case)
    for t in range(case["T"]):
        steps.step(y[t])
    np.testing.assert_array_equal(_bits(steps.expectations_multi([0, 1, 2, 3])), _bits(em), err_msg="step API == series API")
    np.testing.assert_array_equal(_bits(steps.weights(0)[1]), _bits(bank.weights(0)[1]), err_msg="weights(): step API == series API")
    steps.close()
    bank.close()


# ---- swarm aggregate -----------------------------------------------------------------------------------------------------------------
def _swarm_thetas(R):
    rng = np.random.default_rng(1)
    return np.stack([rng.uniform(.8, .99, R), rng.uniform(-.1, .1, R), rng.uniform(.5, 1.0, R), rng.uniform(-.5, -.01, R)], axis=1)


def check_swarm(name, R, rows, lcl, aggregate):
    """aggregate(num_threads) -> (mean ll, means[n]) against swarm_means_ref over the per-member rows."""
    allrows = np.concatenate([rows, lcl[None, :]])
    bud = er.budget_swarm(R, allrows) + 2.0 ** -59 * np.abs(allrows).max(axis=1)
    k = -(-R // 256) + 11
    plain, _ = er.swarm_means_ref(allrows, 0)
    seen = {}
    for nt in (0, 7, 256, 299, R, R + 5):
        ll, ex = aggregate(nt)
        dev = np.concatenate([np.asarray(ex, dtype=np.float64), [ll]])
        _, pooled = er.swarm_means_ref(allrows, nt)
        err = np.abs(dev.astype(np.longdouble) - pooled).astype(np.float64)
        worst = np.argmax(err / bud)
        record(f"{name} R={R} num_threads={nt}", err[worst], bud[worst], k)
        assert (err <= bud).all(), (name, R, nt, dev, pooled)
        seen[nt] = dev
    # more threads than members: the surplus threads have no member and the pool averages over those that have one -- T = R
    # (documented in include/ssme_pf.h), which is the plain mean
    np.testing.assert_array_equal(_bits(seen[R + 5]), _bits(seen[R]))
    assert (np.abs(seen[R].astype(np.longdouble) - plain) <= bud).all()
    for nt in (7, 256, 299):                                       # num_threads does not divide R: not the plain mean
        if R % nt:
            assert np.abs(seen[nt][-1] - seen[0][-1]) > 1e3 * bud[-1], (R, nt)


@pytest.fixture(scope="module")
def swarm_oracle_rows(oracle, spy):
    """Expectations of 300 oracle members, computed once."""
    R, n, T = 300, 600, 3
    th = _swarm_thetas(R)
    rows, lcl = np.empty((4, R)), np.empty(R)
    for r in range(R):
        of = oracle.Filter(oracle.MODEL_SVOL_LEVERAGE, n, th[r], 3, rep=r)
        for t in range(T):
            lcl[r] = of.step(spy[t], 0.0 if t == 0 else spy[t - 1])
        st = er.make_state(oracle, of.state(), 2048)
        rows[:, r] = [float(v) for v in er.expect_fixed_point(ec.builtin_rows(oracle, st["x"]), st, "longdouble")]
    return rows, lcl


@pytest.mark.parametrize("R", [300, 513])
def test_swarm_aggregate_beyond_256_members(sa, oracle, spy, swarm_oracle_rows, R):
    n, T = 600, 3
    bank = sa.ParticleFilterBank(sa.MODEL_SVOL_LEVERAGE, n, R, 3)
    bank.set_params(_swarm_thetas(R))
    for t in range(T):
        lcl = bank.step(spy[t], 0.0 if t == 0 else spy[t - 1])
    rows = bank.expectations_multi([0, 1, 2, 3])
    check_swarm("swarm", R, rows, lcl, lambda nt: bank.swarm_aggregate([0, 1, 2, 3], num_threads=nt))
    if R == 300:                                                    # ... and against rows that never saw the device
        orows, olcl = swarm_oracle_rows
        np.testing.assert_array_equal(_bits(lcl), _bits(olcl))
        # the device's member rows differ from the oracle members' E_q by at most budget_sum of one 2048-particle tile each (S_abs <= the
        # row's largest |E| is not available per member here, so the bound uses max_r E_q[|h|] computed from the oracle rows of the
        # positive functionals: rows 1, 2, 3 are positive, and |x| <= 1 + x^2 bounds row 0); a weighted mean keeps that bound
        k = er.k_sum(2048, 1, "expect")
        sabs = np.array([1.0 + orows[1].max(), orows[1].max(), orows[2].max(), 42.0])
        tol = er.budget_swarm(R, orows) + (k * er.U / (1.0 - k * er.U) + 2.0 ** -59) * sabs
        for nt in (0, 7, 299):
            ll, ex = bank.swarm_aggregate([0, 1, 2, 3], num_threads=nt)
            _, pooled = er.swarm_means_ref(orows, nt)
            err = np.abs(np.asarray(ex) - pooled.astype(np.float64))
            worst = np.argmax(err / tol)
            record(f"swarm R=300 num_threads={nt} vs oracle members", err[worst], tol[worst], k)
            assert (err <= tol).all(), (nt, ex, pooled)
    bank.close()


# ---- Liu-West ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.lw_cases(), ids=lambda c: c["name"])
def test_liu_west_expectations(sa, oracle, case):
    """expectations([0..7]), param_means() and weights() of both forms: k_lw_param_partials / k_lw_param_means (whose 16-tile batches
    and in-order tile sum set the budget) and k_lw_weights.  The device hands out no cdf here; weights() within two roundings of
    q_j exp(m_b - m) 2^-41 pins it."""
    tr, lo, hi = ec.lw_prior(case, oracle)
    n, T = case["n"], case["T"]
    cls = sa.svol_lw_2_par if case["form"] else sa.svol_lw_1_par
    g = cls(0.99, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=n, seed=11, transforms=tuple(tr), rs=case["rs"])
    of = oracle.LWFilter(n, 11, transforms=tr, lo=lo, hi=hi, form=case["form"], resamp_sched=case["rs"])
    y, z = ec.lw_series(T)
    for t in range(T):
        g.filter(y[t], z[t])
        ll = of.step(y[t], z[t])
        assert g.getLogCondLike() == ll, (case["name"], t)
        if not (case.get("every_step") or t == T - 1):
            continue
        so, gs = of.state(), g.state()
        np.testing.assert_array_equal(_bits(gs["x"]), _bits(so["x"]), err_msg="particles")
        np.testing.assert_array_equal(_bits(gs["theta"]), _bits(so["theta"]), err_msg="parameters")
        st = er.lw_state(oracle, so)
        x, thu, w = g.weights(0)
        np.testing.assert_array_equal(_bits(x), _bits(so["x"]))
        # untransformed parameters: the device's tr_inv uses the table exp, the oracle's entry point the series one, so the two are not
        # bit-equal.  Each is an exp within 2 ulp followed by at most two rounded operations (1 / (1 + e), 2 / (1 + e) - 1), about 4 ulp
        # of the true value each: they agree within 8 ulp of the result (a strided sample of about 4000 particles above that size).  The functional
        # values h_j of the reference are the device's doubles, which k_lw_param_partials forms with the same call.
        idx = np.arange(n) if n <= 4096 else np.unique(np.concatenate([np.arange(0, n, n // 4000), [n - 1]]))
        want = ec.lw_untransform(oracle, tr, so["theta"], idx)
        # the twice-Fisher inverse 1 - 2 / (1 + e) cancels: its error is absolute, 4 ulp of the intermediate 2 / (1 + e) <= 2
        scale = np.abs(want) + 2.0 * (np.asarray(tr) == 1)[:, None]
        assert (np.abs(thu[:, idx] - want) <= 8 * 2.0 ** -52 * scale).all(), "tr_inv"
        h = ec.lw_h_rows(oracle, so["x"], thu)
        name = f"{case['name']} t={t}"
        ex = g.expectations(list(range(8)))[:, 0]
        check_rows(name, ex, h, st, "lw")
        assert ex[3] == 42.0
        np.testing.assert_array_equal(_bits(g.param_means()[0]), _bits(ex[4:]), err_msg="param_means() == expectations([4..7])")
        check_weights(name, w, oracle, st)
    g.close()


# ---- user models: each library in a process of its own (tests/user_h_worker.py) -------------------------------------------------------
@pytest.fixture(scope="module")
def two_factor_run(tmp_path_factory):
    """One process runs every case of USER_CASES on the device and hands back states and expectations."""
    import subprocess
    import sys
    from ssme_amd import build
    so = build.build_user_model(os.path.join(ROOT, "tests", "models", "svol_two_factor_h.h"), "two_factor_h")
    out = str(tmp_path_factory.mktemp("uh") / "exact.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "user_h_worker.py"), "exact", out], env=dict(os.environ, SSME_PF_LIB=so), check=True,
                   timeout=300)
    return np.load(out)


@pytest.mark.parametrize("case", ec.USER_CASES, ids=lambda c: c["name"])
def test_two_factor_functionals_against_the_oracle_state(sa, oracle, spy, two_factor_run, case):
    """The seven functionals of tests/models/svol_two_factor_h.h with inputs that never saw the device: particles and cdf of the
    callback-driven oracle (bit-compared with the device's first), h in the header's operation sequence (oracle.exp_t for its table exp).
    One- and two-particle filters, odd ragged tails, wrapped final loops, outliers, schedule 3.  What these cases cannot tell apart: an
    upper bound of the 16-byte path that lets in the one particle beyond an odd tail (`j + 1 <= nvalid`), because the padded cdf repeats the
    tile total and that particle's integer weight is 0 -- the same bits."""
    from oracle_models import _two_factor_oracle
    r, key = two_factor_run, case["name"]
    y, zs = ec.user_observations(case)
    of = _two_factor_oracle(oracle, case["n"], 21, 0, 0, case["tile"], case["sched"])
    _, per = of.run_series(y, zs)
    np.testing.assert_array_equal(_bits(r["lls_" + key]), _bits(per), err_msg="log conditional likelihoods")
    o = of.state()
    np.testing.assert_array_equal(_bits(r["x_" + key]), _bits(o["x"]), err_msg="particles")
    np.testing.assert_array_equal(r["cdf_" + key], o["cdf"], err_msg="integer cdf")
    np.testing.assert_array_equal(r["A_" + key], o["A"])
    np.testing.assert_array_equal(_bits(r["mb_" + key]), _bits(o["mb"]))
    st = er.make_state(oracle, dict(o, x=o["x"][0]), case["tile"])
    x1, x2 = o["x"]
    h = np.stack([x1, x2, x1 * x1, x1 * x2, x2 * x2, oracle.exp_t(0.5 * (x1 + x2)), np.full_like(x1, zs[-1] + 1.0)])
    check_rows("two_factor_h " + key, r["ue_" + key][:, 0], h, st, "user")


@pytest.fixture(scope="module")
def two_factor_swarm_run(tmp_path_factory):
    import subprocess
    import sys
    from ssme_amd import build
    so = build.build_user_model(os.path.join(ROOT, "tests", "models", "svol_two_factor_h.h"), "two_factor_h")
    out = str(tmp_path_factory.mktemp("uh") / "swarm_big.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "user_h_worker.py"), "swarm_big", out], env=dict(os.environ, SSME_PF_LIB=so), check=True,
                   timeout=300)
    return np.load(out)


@pytest.mark.parametrize("R", [300, 513])
def test_swarm_aggregate_user_beyond_256_members(sa, two_factor_swarm_run, R):
    """swarm_aggregate_user: k_swarm_means over n_h = 7 rows and more than 256 members, num_threads in {0, 7, 256, 299, R, R + 5},
    against swarm_means_ref over the device's own per-member rows; num_threads > R is T = R."""
    r = two_factor_swarm_run
    check_swarm("swarm_aggregate_user", R, r[f"ue_{R}"], r[f"lcl_{R}"], lambda nt: (float(r[f"ll_{R}_{nt}"][0]), r[f"ex_{R}_{nt}"]))


# ---- the model at the documented maxima: dim_x = dim_y = 4, n_h = 16 (tests/models/lin_gauss_4d_h.h) -------------------------------
TH_4D = (0.9, 0.5, 0.7, 0.4, 1.1, 0.25)


@pytest.mark.parametrize("n,tile", [(1500, 2048), (6000, 512)])
def test_model_at_the_documented_maxima(sa, oracle, tmp_path, n, tile):
    """Four state and four observation components, sixteen functionals: particles (all four planes), log-weights, cdf, ancestors and the
    per-step log-likelihood against the oracle's restatement bit for bit; the sixteen expectations within the budgets of the exact
    reference; and the mean log-likelihood of 32 replicate filters against the sum of four scalar Kalman filters (exact for this model),
    with the criterion of test_vector_user_model_of_odd_shape_vs_oracle_and_kalman."""
    import subprocess
    import sys
    from oracle_models import _lin_gauss_4d_oracle, lin_gauss_4d_h_rows
    from ssme_amd import build
    so = build.build_user_model(os.path.join(ROOT, "tests", "models", "lin_gauss_4d_h.h"), "lin_gauss_4d_h")
    T, T_long, nseeds = 6, 40, 32
    phi, sigma, taus = TH_4D[0], TH_4D[1], TH_4D[2:]
    rng = np.random.default_rng(11)
    x = rng.normal(size=4) * sigma / np.sqrt(1.0 - phi * phi)
    y = np.empty((T_long, 4))
    for t in range(T_long):
        if t > 0:
            x = phi * x + rng.normal(size=4) * sigma
        y[t] = x + np.array(taus) * rng.normal(size=4)
    np.save(str(tmp_path / "y4.npy"), y)
    out = str(tmp_path / "u4.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "user_4d_worker.py"), out, str(n), str(tile), str(T), str(nseeds)],
                   env=dict(os.environ, SSME_PF_LIB=so), check=True, timeout=300)
    r = np.load(out)
    of = _lin_gauss_4d_oracle(oracle, n, 5, 0, 0, tile)
    ll, per = of.run_series(y[:T], r["z"])
    o = of.state()
    assert float(r["ll"][0]) == ll
    np.testing.assert_array_equal(_bits(r["per"][0]), _bits(per), err_msg="per-step log-likelihood")
    np.testing.assert_array_equal(_bits(r["x"]), _bits(o["x"]), err_msg="particles, four components")
    np.testing.assert_array_equal(_bits(r["logw"]), _bits(o["logw"]), err_msg="log-weights")
    np.testing.assert_array_equal(r["cdf"], o["cdf"], err_msg="integer cdf")
    np.testing.assert_array_equal(r["anc"], o["anc"], err_msg="ancestors")
    st = er.make_state(oracle, dict(o, x=o["x"][0]), tile)
    h = lin_gauss_4d_h_rows(oracle, o["x"], float(r["z"][-1]))
    assert r["ue"].shape == (16, 1)
    check_rows(f"lin_gauss_4d_h n{n}-tile{tile}", r["ue"][:, 0], h, st, "user")
    exact = sum(oracle.kalman_loglik(phi, sigma, taus[d], y[:, d])[0] for d in range(4))
    lls = r["lls"]
    se = lls.std(ddof=1) / np.sqrt(lls.size)
    print("kalman", exact, "mean of", nseeds, "filters", lls.mean(), "se", se)
    assert abs(lls.mean() - exact) < 4.0 * se + 0.02, (lls.mean(), exact, se)
