"""The case and route lists of tests/user_edge_cases.py through the oracle alone (no GPU): every (header, case, route) reaches what its
`expect` says ("the NaN steps are exactly these", S = 0, m = -inf, ancestors collapsed to particle 0, which planes are NaN from where),
every case has finite terms to be compared on, route_of() names the instantiations written out below, and the float closures of
user_edge_cases.py equal the numpy closures of user_cov_ref.py / oracle_models.py bit for bit on every case.
test_user_edges_gpu.py then asks the device for the oracle's bits on the same lists."""
import numpy as np
import pytest

import oracle_models as om
import user_cov_ref as ucr
import user_edge_cases as uc

PAIRS = [(h, p) for h in uc.HEADERS for p in uc.pairs(h)]
CHECK_N, CHECK_TILE = 200, 2048           # the shape at which the two sets of closures are compared


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what + ": NaN pattern")
    np.testing.assert_array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)], err_msg=what)


# (header, route, form, resampler) -> (kernel, NT, BIG, TILE, RS, WL2, level-2): written out from csrc/pf_api.hip by hand, not by route_of()
TABLE = {
    ("svol_reg_cov", "small-1", "hot", 0): ("k_filter_series_lane<64>", 64, False, 2048, None, None, "in the loop"),
    ("svol_reg_cov_nofirst", "small-64", "hot", 1): ("k_filter_series_lane<64>", 64, False, 2048, None, None, "in the loop"),
    ("svol_reg_cov", "small-100", "hot", 0): ("k_filter_series_lane<128>", 128, False, 2048, None, None, "in the loop"),
    ("svol_student_t", "small-200", "hot", 0): ("k_filter_series_lane<256>", 256, False, 2048, None, None, "in the loop"),
    ("svol_reg_cov", "small-300", "hot", 1): ("k_filter_series_lane<512>", 512, False, 2048, None, None, "in the loop"),
    ("svol_reg_cov", "small-1000", "hot", 0): ("k_filter_series_small<512,1>", 512, False, 2048, None, None, "in the loop"),
    ("svol_reg_cov_nofirst", "small-2000", "hot", 1): ("k_filter_series_small<512,2>", 512, False, 2048, None, None, "in the loop"),
    ("svol_reg_cov", "small-300", "general", 0): ("k_filter_step", 512, False, 2048, -1, True, "wave-by-wave in k_filter_step + fused accounting (ticket)"),
    # a vector model at N <= 2048: the tiled kernel, whatever the small-series switch says
    ("svol_two_factor_cov", "small-300", "hot", 0): ("k_filter_step", 512, False, 2048, 0, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("lin_gauss_3d", "small-2000", "hot", 1): ("k_filter_step", 512, False, 2048, 1, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("svol_two_factor", "edge-n1", "hot", 0): ("k_filter_step", 512, False, 2048, 0, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("svol_reg_cov", "edge-n2047", "hot", 1): ("k_filter_step", 512, False, 2048, 1, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("svol_two_factor_cov", "edge-n2049", "general", 3): ("k_filter_step", 512, False, 2048, -1, True, "wave-by-wave in k_filter_step + fused accounting (ticket)"),
    ("svol_two_factor_cov", "wl2-512", "hot", 0): ("k_filter_step", 256, False, 512, 0, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("svol_reg_cov", "wl2-512", "hot", 2): ("k_filter_step", 256, False, 512, -1, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("lin_gauss_3d", "wl2-2048", "hot", 1): ("k_filter_step", 512, False, 2048, 1, True, "wave-by-wave in k_filter_step + kf_finalize"),
    ("svol_two_factor", "split-forced-5", "hot", 0): ("k_filter_step", 256, True, 512, 0, False, "k_l2_scan_blocks x1 (l2_inkernel), ranges in k_filter_step"),
    ("svol_two_factor_cov", "split-forced-5", "general", 2): ("k_filter_step", 256, True, 512, -1, False, "k_l2_scan_blocks x1 (l2_inkernel), ranges in k_filter_step"),
    ("svol_two_factor", "tables-5", "hot", 1): ("k_filter_step", 256, True, 512, 1, False, "k_level2_plan"),
    ("svol_reg_cov", "tables-5", "general", 0): ("k_filter_step", 256, True, 512, -1, False, "k_level2_plan"),
}


def test_route_of_selects_the_listed_instantiations():
    import bs_edge_cases as bc
    all_routes = {r["name"]: r for r in bc.routes()}
    for (header, route, form, rs), want in TABLE.items():
        assert uc.route_of(header, uc.case_of(header, "nan-y"), all_routes[route], form, rs) == want, (header, route, form, rs)
    # step 0 and schedule 3 run the general kernel whatever the flags
    assert uc.route_of("svol_two_factor_cov", uc.case_of("svol_two_factor_cov", "nan-y"), uc.ROUTES["wl2-512"], "hot", 0, t=0)[4] == -1
    assert uc.route_of("svol_two_factor_cov", uc.case_of("svol_two_factor_cov", "nan-sched3-carried"), uc.ROUTES["wl2-512"], "hot", 0)[4] == -1
    # the covariate headers take every branch of launch_small_m in the hot form
    for header in ("svol_reg_cov", "svol_reg_cov_nofirst"):
        hot = {uc.route_of(header, c, r, "hot", 0)[0] for c, r in uc.pairs(header)}
        assert {f"k_filter_series_lane<{k}>" for k in (64, 128, 256, 512)} | {"k_filter_series_small<512,1>", "k_filter_series_small<512,2>"} <= hot
    # the answers of bs_edge_cases.route_of are unchanged for a scalar model
    for header in uc.SCALAR:
        for c, r in uc.pairs(header):
            assert uc.route_of(header, c, r, "hot", 1) == bc.route_of(dict(c, model=0), r, "hot", 1)


def test_the_chosen_pairs_cover_the_minimum():
    for header in uc.HEADERS:
        ids = {uc.pair_id(p) for p in uc.pairs(header)}
        names = {c["name"] for c in uc.cases(header)}
        cov = set(uc.COV_CASES.get(header, ()))
        assert cov <= names and ("nan-y1" in names) == (uc.HEADERS[header]["dy"] == 2)
        for r in uc.TILED_ROUTES:
            assert {f"{c}@{r}" for c in ({"nan-y", "inf-y", "huge-y"} | cov)} <= ids
        assert {f"{c}@wl2-512" for c in names} <= ids
        assert {f"nan-y@{r}" for r in uc.EDGE_ROUTES} <= ids
        assert ({f"bad-first@{r}" for r in uc.EDGE_ROUTES} <= ids) == (header in uc.VECTOR)
        assert ({f"{c}@{r}" for r in uc.SMALL_ROUTES for c in ({"nan-y"} | cov)} <= ids) == (header in uc.SCALAR)
        assert not (header in uc.VECTOR and any("@small-" in i for i in ids))
        for c in uc.cases(header):
            assert len(c["theta"]) == c["R"] >= 2 and len({tuple(t) for t in c["theta"]}) == c["R"], "different rows in every filter"
    # every use of a covariate in a header has its case: prop, logg, first
    assert {n.split("-")[2] for n in uc.COV_CASES["svol_reg_cov"] if n.startswith("nan-z")} == {"prop", "logg", "first"}
    assert {n.split("-")[2] for n in uc.COV_CASES["svol_two_factor_cov"] if n.startswith("nan-z")} == {"prop", "logg", "first"}


def _nan_steps(case, r):
    e = case["expect"]
    return tuple(e["nan_steps_r"][r] if "nan_steps_r" in e else e["nan_steps"])


def _prove(oracle, header, case, route, rs):
    run = uc.oracle_run(oracle, header, case, route, rs)
    n, tile, B, T = uc.shape(case, route)
    exp, R, name = case["expect"], case["R"], f"{header} {uc.pair_id((case, route))} rs={rs}"
    ll = np.array([lls for lls, _ in run])                                               # [T, R]
    for r in range(R):
        assert tuple(np.flatnonzero(np.isnan(ll[:, r]))) == _nan_steps(case, r), (name, r, ll[:, r])
        assert not np.isinf(ll[:, r]).any(), name
    # the condition: finite terms to compare -- two after the degenerate step in some filter, a healthy neighbour row, or the clean
    # pass that a clean_tail case appends on the same handle (only where the cloud stays NaN to the end for every theta)
    marks = [t for r in range(R) for t in _nan_steps(case, r)] + ([exp["big_step"]] if "big_step" in exp else [])
    after = max(int(np.isfinite(ll[min(marks) + 1:, r]).sum()) for r in range(R))
    healthy_row = "nan_steps_r" in exp and any(not s for s in exp["nan_steps_r"])
    assert after >= 2 or healthy_row or case["clean_tail"], (name, ll)
    assert case["clean_tail"] == (("x_nan_from" in exp or "x1_nan_from" in exp) and after < 2), name
    if case["clean_tail"]:
        tail = np.array([lls for lls, _ in uc.oracle_run(oracle, header, uc.clean(case), route, rs)])
        assert np.isfinite(tail).all() and tail.shape == ll.shape, name
    if healthy_row:
        # a bad theta row leaves its neighbours alone: every valid filter is the single-filter oracle at its rep
        y, Z = uc.series(header, case)
        for r in [r for r in range(R) if not exp["nan_steps_r"][r]]:
            solo = uc.StepFilter(oracle, header, case["theta"][r], n, r, rs, case["sched"], tile)
            _same([solo.step(y[t], None if Z is None else Z[t]) for t in range(T)], ll[:, r], f"{name}: filter {r} alone")
            assert np.isfinite(ll[:, r]).all()
    rr = next((r for r in range(R) if _nan_steps(case, r)), 0)
    sts = [run[t][1][rr] for t in range(T)]
    for t in exp.get("S0_at", ()):
        lw = sts[t]["logw"]
        assert sts[t]["S"] == 0 and (np.isnan(lw).any() or not (lw > -np.inf).any()), (name, t)
    if "S0_at" in exp:
        assert tuple(t for t in range(T) if sts[t]["S"] == 0) == tuple(exp["S0_at"]), name
    assert tuple(t for t in range(T) if sts[t]["m"] == -np.inf) == tuple(exp.get("m_neg_inf_at", ())), name
    for t in exp.get("collapsed_at", ()):
        assert not sts[t]["anc"].any(), (name, t, np.unique(sts[t]["anc"]))              # a cdf of zeros: every ancestor is particle 0
    if "big_step" in exp:
        assert ll[exp["big_step"], 0] < -40.0 and np.isfinite(ll).all(), name
    dx = uc.HEADERS[header]["dx"]
    for d in range(dx):
        frm = exp["x_nan_from"] if "x_nan_from" in exp else (exp.get("x1_nan_from") if d == 1 else None)
        for t in range(T):
            assert np.isnan(sts[t]["x"][d]).all() == (frm is not None and t >= frm), (name, d, t)
            assert np.isnan(sts[t]["x"][d]).any() == np.isnan(sts[t]["x"][d]).all(), (name, d, t)
    if case["sched"] > 1:
        for t in range(1, T):
            if t % case["sched"] == 0:
                assert sts[t]["anc"].max() < n


@pytest.mark.parametrize("hp", PAIRS, ids=lambda hp: f"{hp[0]}-{uc.pair_id(hp[1])}")
def test_pair_reaches_what_its_expect_says(oracle, hp):
    header, (case, route) = hp
    _prove(oracle, header, case, route, 0)
    if route["name"] == "wl2-512":
        _prove(oracle, header, case, route, 1)
    uc.forget_runs()


def _lin_gauss_3d_numpy(oracle, th, n, rep, rs, sched, tile):
    """tests/models/lin_gauss_3d.h as tests/test_parity_gpu.py restates it (numpy closures)."""
    phi, sig, tau = th[0], th[1:4], th[4]
    e1 = lambda f, v: float(f(np.array([v]))[0])
    a4 = 1.0 / np.sqrt(1.0 - phi * phi)
    a5, a6 = e1(oracle.log, tau), 1.0 / tau
    init = lambda zn: np.array([zn[0] * (sig[0] * a4), zn[1] * (sig[1] * a4), zn[2] * (sig[2] * a4)])
    prop = lambda xx, zn, zcov: np.array([phi * xx[0] + zn[0] * sig[0], phi * xx[1] + zn[1] * sig[1], phi * xx[2] + zn[2] * sig[2]])

    def logg(yy, xx):
        d = (yy[0] - ((xx[0] + xx[1]) + xx[2])) * a6
        return (-a5 - 0.91893853320467274178) - 0.5 * (d * d)
    return oracle.UserVectorModelFilter(n, uc.SEED, 3, 1, init, prop, logg, rep=rep, resampler=rs, resamp_sched=sched, tile=tile)


@pytest.mark.parametrize("header", list(uc.HEADERS))
def test_float_closures_equal_the_numpy_closures(oracle, header):
    """Every case of the header at N = 200, every filter: the per-step terms and the final state of user_edge_cases.StepFilter equal
    those of the closures the earlier tests use -- user_cov_ref.vector_oracle for the covariate headers (and scalar_oracle, which must
    agree with it, for the header without `first`), oracle_models / test_parity_gpu's restatements for the others (valid theta rows:
    they have no `bad` argument)."""
    s = uc.HEADERS[header]
    n, tile = CHECK_N, CHECK_TILE
    compared = 0
    for case in uc.cases(header):
        y, Z = uc.series(header, case)
        T = case["T"]
        for r in range(case["R"]):
            th = case["theta"][r]
            bad = tuple(th) == tuple(s["bad"])
            f = uc.StepFilter(oracle, header, th, n, r, 0, case["sched"], tile)
            with np.errstate(all="ignore"):
                per = [f.step(y[t], None if Z is None else Z[t]) for t in range(T)]
                st = f.state()
                if s["K"]:
                    g = ucr.vector_oracle(oracle, header, th, Z, n, uc.SEED, r, 0, case["sched"], tile, T)
                    ll, per2 = g.cov_run(y)
                    st2 = g.state()
                    if not s["first"]:
                        h = ucr.scalar_oracle(oracle, header, th, Z, n, uc.SEED, r, 0, case["sched"], tile)
                        _same([h.cov_step(t, y[t, 0]) for t in range(T)], per2, f"{header} {case['name']} r={r}: scalar_oracle == vector_oracle")
                        st3 = h.state()
                        _same(st3["x"], st2["x"][0], "scalar_oracle == vector_oracle: x")
                        np.testing.assert_array_equal(st3["cdf"], st2["cdf"])
                elif bad:
                    continue
                elif header == "svol_student_t":
                    g = om._student_t_oracle(oracle, n, uc.SEED, r, 0, tile, th=th)
                    if case["sched"] != 1:
                        continue                                  # (that restatement takes no schedule)
                    ll, per2 = g.run_series(y[:, 0])
                    st2 = g.state()
                    st2["x"] = st2["x"][None, :]
                elif header == "svol_two_factor":
                    g = om._two_factor_oracle(oracle, n, uc.SEED, r, 0, tile, case["sched"], th=th)
                    ll, per2 = g.run_series(y)
                    st2 = g.state()
                else:
                    g = _lin_gauss_3d_numpy(oracle, th, n, r, 0, case["sched"], tile)
                    ll, per2 = g.run_series(y)
                    st2 = g.state()
            name = f"{header} {case['name']} r={r}"
            _same(per, per2, name + ": per-step terms")
            _same(st["x"], np.asarray(st2["x"]).reshape(s["dx"], n), name + ": x, all planes")
            _same(st["logw"], st2["logw"], name + ": log-weights")
            np.testing.assert_array_equal(st["cdf"], st2["cdf"], err_msg=name)
            np.testing.assert_array_equal(st["anc"], st2["anc"], err_msg=name)
            compared += 1
    assert compared >= len(uc.cases(header))


def test_bookkeeping_series_differ_per_length(oracle):
    """The covariates of the bookkeeping runs are drawn per length, and a run with Z differs from the run with z = NULL: a stale or
    mis-strided row cannot reproduce the bits."""
    for header in uc.BOOK_HEADERS:
        K = uc.HEADERS[header]["K"]
        rows = [uc.book_series(header, T)[1] for T in (1, 2, 6, 40)]
        for a in rows:
            for b in rows:
                if a is not b:
                    assert not np.array_equal(a[0], b[0])
        assert rows[3].shape == (40, K) and len({float(v) for v in rows[2].ravel()}) == 6 * K
        a, b = uc.book_oracle(oracle, header, 300, 2048, 2, True)[0], uc.book_oracle(oracle, header, 300, 2048, 2, False)[0]
        assert np.isfinite(a).all() and np.isfinite(b).all() and not np.array_equal(a, b)
    uc.forget_runs()
