"""The particle-sharded drivers (csrc/pf_api.hip: ssme_pf_shard_*, ssme_lw_shard_*; csrc/shard_driver.h; k_shard_plan, k_level2_plan +
k_shard_window_check, the win_flag clamp of k_filter_step and the Liu-West stage kernels; ssme_amd/sharded.py) at the degenerate inputs
and edge layouts of tests/shard_edge_cases.py: NaN, 1e200, -1e160 and 1e3 observations, a NaN covariate, invalid theta, NaN steps under
a resampling schedule -- on ranks of one tile or ONE particle, a ragged last share, a halo margin that is the whole share, a collapse
whose reach is exactly the margin and one tile more, one rank, and the split level-2.  Every comparison is bit for bit: the C++ drivers
(ranks as threads over tests/cpp/mock_rccl.cpp, one harness process at a time, at most 4 rank threads) against the unsharded device
filter inside the harness (NaN equals the same NaN, -0 differs from +0) and against the oracle here (per-step values, the sum, the
concatenated final particles and integer cdf; NaN for NaN).  test_shard_edges_cpu.py proves without a GPU that each pair reaches its
branch and that shard_edge_cases.MUST_LEAVE -- the steps and ranks whose NEEDED reach exceeds the halo margin -- is the oracle's.

What the planners and the step kernel do when the weight sum is 0 (read from the code before the first run; S = the integer total):
  * level2_scan / k_level2_plan: a NaN tile maximum makes m NaN, all -inf makes m = -inf; dexp_scaled_t clamps the NaN argument (m_b - m
    with either NaN, or -inf - -inf) to 0, so A'_b = rint(A_b * 0) = 0, T'_j = 0 for every tile and S = 0: never NaN, never negative.
  * tile_target_bounds with S = 0: multinomial t_scale = 0 / G = 0, t_lo = ceil(pgam * 0) = 0, t_hi = 0 + (0 + 2) = 2; systematic and
    stratified t_scale = 0 / N = 0, t_lo = t_hi = 0.  count_less_pow2 counts T'_j < target over [0, Bpow2) (entries past B are +inf):
    lo = 0 always; hi = #{T'_j = 0 < 2} = B (clamped to B - 1) for multinomial, 0 for the other two.
  * k_shard_plan (exact path, up to 1024 tiles) takes t_lo of the rank's FIRST tile and t_hi of its LAST tile through the same
    tile_target_bounds and the same count over the same T': window [0, B - 1] (multinomial) or [0, 0].  k_filter_step's own range for
    tile b on the exact path comes from the same two counts of the same T' (lds_cnt, ballots of T'_j < t_lo / t_hi) with the same clamps
    to B - 1: [0, B - 1] or [0, 0] for EVERY tile, inside the planned window, and win_tile0 = lo = 0, so every address is >= 0.
    Above 1024 tiles k_level2_plan writes l2_lo / l2_hi per tile (count_less_pow2 for a thread's first tile, count_from afterwards:
    with T' = 0 everywhere count_from(prev = 0, 0) stops at its first probe, count_from(0, 2) gallops to Bpow2 and is clamped), the host
    takes [l2_lo of the rank's first tile, l2_hi of its last] and k_filter_step<BIG> reads the SAME per-tile tables: inside by construction.
  * on the fixed halo nobody knows the plan: k_filter_step compares its own [bb_min, bb_min + span - 1] with the rows it was given
    (first = max(win_tile0, 0), last = min(win_tile0 + win_tiles - 1, B - 1)), raises win_flag and clamps bb_min into [first, last]
    with span = 1, so the launch stays inside the halo buffer whatever it then computes; k_shard_window_check does the same comparison
    from the tables.  The flags are reduced over the ranks after the loop and the series is run again on the exact path.
The reading found the kernel's range inside the planned one in every case, no unclamped index and no loop that waits for data.

ssme_*_shard_stats report the widest reach only where the split level-2 planned the exchange (include/ssme_pf.h: 0 otherwise), so the
reported reach is held to the oracle-needed one on the split-l2 layout and to 0 elsewhere.  Times on an MI355X: tests/README.md."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import shard_edge_cases as sc
import test_expectations_gpu as teg
from test_liu_west_edges_gpu import same_bits

pytestmark = pytest.mark.gpu
sa = teg.sa
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(ROOT, "tests", "golden", "spy_returns.csv")
ERR_UNSUPPORTED = 3
EXIT_ERR_STATE = 5                             # the harness's exit status when a bootstrap rank returned SSME_ERR_STATE


@pytest.fixture(scope="module")
def harness():
    """tests/cpp/test_shard_threads and the mock RCCL, built once for the module."""
    from ssme_amd import build
    so = build.build()
    cpp = os.path.join(ROOT, "tests", "cpp")
    mock, exe = os.path.join(cpp, "libmock_rccl.so"), os.path.join(cpp, "test_shard_threads")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wno-unused-result", os.path.join(cpp, "mock_rccl.cpp"), "-o", mock])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", os.path.join(cpp, "test_shard_threads.cpp"), "-o", exe, "-Wl,--no-as-needed", mock,
                           "-Wl,--as-needed", so, "-Wl,-rpath," + cpp, "-Wl,-rpath," + os.path.dirname(so)])
    return exe


@pytest.fixture(scope="module")
def window_check_exe():
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "test_window_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function", "-Wno-unused-value",
                           "-Wno-unused-result", os.path.join(cpp, "test_window_check.hip"), "-o", exe])
    return exe


def test_window_check_kernel_decides_at_the_margin(window_check_exe, tmp_path):
    """k_shard_window_check launched alone on windows written by hand: a reach of margin - 1 and margin tiles stays, margin + 1 and
    margin + 2 leave, left and right, for every rank (the last one owning fewer tiles), from the [world][2] plan and from the per-tile
    tables; the recorded widest reach is the largest one given.  Through the drivers this decision is hidden behind k_filter_step's own."""
    cases = sc.window_check_file(str(tmp_path / "cases.txt"))
    assert any(sc.window_check_expect(c)[0] for c in cases) and not all(sc.window_check_expect(c)[0] for c in cases)
    p = subprocess.run([window_check_exe, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr)
    assert sc.window_check_verify(cases, p.stdout) == 2 * len(cases)


def _timeout(layout):
    return 180 if layout["name"] == "split-l2" else 60


def _read_dump(path):
    with open(path, "rb") as f:
        assert f.read(8) == b"SSMEDMP1"
        T, n, kind, complete = (int(v) for v in np.fromfile(f, dtype=np.int64, count=4))
        out = dict(T=T, n=n, kind=kind, complete=bool(complete))
        if complete:
            out["per"] = np.fromfile(f, dtype=np.float64, count=T)
            out["x"] = np.fromfile(f, dtype=np.float64, count=n)
            if kind == 0:
                out["cdf"] = np.fromfile(f, dtype=np.uint64, count=n)
            else:
                out["theta"] = np.fromfile(f, dtype=np.float64, count=4 * n).reshape(4, n)
            assert f.read(1) == b"" and out["per"].size == T and out["x"].size == n
    return out


def run_harness(exe, tmp_path, layout, T, model, rs, mode, sched=1, yscale="1", form=0, yset="-", zset="-", theta="-", rerun=0, ok=(0,)):
    """One harness process; a timeout is a hang (subprocess.TimeoutExpired fails the test, nothing is tried again)."""
    dump = str(tmp_path / "dump.bin")
    args = [exe, CSV, str(layout["world"]), str(layout["n"]), str(T), str(model), str(rs), str(mode), str(sc.SEED), "0.7", yscale, str(sched),
            str(form), dump, yset, zset, theta, str(rerun)]
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=_timeout(layout))
    assert p.returncode in ok, (p.returncode, p.stderr[-2000:], p.stdout[-2000:])
    lines = p.stdout.strip().splitlines()
    world = layout["world"]
    rows = lambda key: [l.split() for l in lines if l.startswith(key + " ")]
    ranks, stats, lays = rows("rank"), rows("stats"), rows("layout")
    assert len(ranks) == world and len(stats) == world and len(lays) == world and lines[-1].startswith("particle_mismatches")
    kv = {l.split()[0]: l.split()[1] for l in lines if l.split()[0] in ("ref", "ref_hex", "sum_mismatches", "compared_ranks", "cdf_mismatches",
                                                                       "theta_mismatches", "particle_mismatches",
                                                                       "per_step_mismatches_between_ranks", "per_step_mismatches_vs_unsharded")}
    res = dict(rc=p.returncode, paths=[int(r[5]) for r in ranks], exch=[int(r[7]) for r in ranks], any_flag=[int(r[9]) for r in ranks],
               own_flag=[int(r[11]) for r in ranks], reach=[(int(s[7]), int(s[9])) for s in stats],
               sums=[np.array([int(l[2], 16)], dtype=np.uint64).view(np.float64)[0] for l in rows("sum_hex")],
               ref=np.array([int(kv["ref_hex"], 16)], dtype=np.uint64).view(np.float64)[0], err=[int(l[2]) for l in rows("err_state")],
               layout=[tuple(int(l[k]) for k in (3, 5, 7, 9)) for l in lays], kv=kv, dump=_read_dump(dump))
    assert [int(s[3]) for s in stats] == res["any_flag"] and [int(s[5]) for s in stats] == res["own_flag"]
    # the layout rule restated in Python against ssme_*_shard_layout, rank by rank
    B, Bl, own, parts = sc.shares(layout["n"], world)
    assert res["layout"] == [(B, Bl, own[r], parts[r]) for r in range(world)], res["layout"]
    return res


def assert_one_decision(res):
    """Every rank reports the same path, the same reduced flag and the same return status; the reduced flag is the max of the own flags."""
    assert len(set(res["paths"])) == 1 and len(set(res["any_flag"])) == 1 and len(set(res["err"])) == 1, (res["paths"], res["any_flag"], res["err"])
    assert res["any_flag"][0] == max(res["own_flag"]), (res["any_flag"], res["own_flag"])


def assert_equals_unsharded(res, world, aux):
    """By bits, inside the harness: sums, per-step values, particles, integer cdf / theta planes of every rank."""
    assert int(res["kv"]["compared_ranks"]) == world and res["dump"]["complete"]
    for key in ("sum_mismatches", "per_step_mismatches_between_ranks", "per_step_mismatches_vs_unsharded", aux + "_mismatches", "particle_mismatches"):
        assert int(res["kv"][key]) == 0, (key, res["kv"][key])


def oracle_sum(lls):
    tot = 0.0
    for v in lls:
        tot = tot + v
    return tot


def assert_equals_oracle(res, run, T, name):
    lls = [run[t][0][0] for t in range(T)]
    d, so = res["dump"], run[T - 1][1][0]
    same_bits(d["per"], lls, name + ": per-step values")
    same_bits(res["sums"], [oracle_sum(lls)] * len(res["sums"]), name + ": the sum on every rank")
    same_bits([res["ref"]], [oracle_sum(lls)], name + ": the unsharded sum")
    same_bits(d["x"], so["x"], name + ": final particles")
    np.testing.assert_array_equal(d["cdf"], so["cdf"], err_msg=name + ": final integer cdf")


def path_log(name, layout, res, widest, must):
    print(f"SHARDPATH {name} needed_reach {widest} must_leave {list(must) if isinstance(must, tuple) else must} reported_reach {res['reach']} "
          f"path {res['paths'][0]} err_state {res['err'][0]} any_left_halo {res['any_flag'][0]} own_left_halo {res['own_flag']} exchanged {res['exch']}")


RUNS = sc.runs()


@pytest.mark.parametrize("item", RUNS, ids=sc.run_id)
def test_bootstrap_cpp_driver(harness, oracle, tmp_path, item):
    case, layout, rs, mode = item
    name = sc.run_id(item)
    n, T = sc.shape(case, layout)
    world = layout["world"]
    B, Bl, own, parts = sc.shares(n, world)
    run = sc.oracle_run(oracle, case, layout, rs)
    must = sc.must_leave(case, layout, rs)
    widest = sc.must_leave_from_oracle(oracle, case, layout, rs)[1] if rs != sc.IID else None
    yset, zset, theta = sc.overrides(case, T)
    res = run_harness(harness, tmp_path, layout, T, case["model"], rs, mode, sched=case["sched"], yset=yset, zset=zset, theta=theta,
                      ok=(0, EXIT_ERR_STATE) if mode == 1 else (0,))
    path_log(name, layout, res, widest, must)
    assert_one_decision(res)
    if mode != 2 and rs != sc.IID:
        # the fixed-halo pass: reported reach >= needed reach where the split level-2 plans (documented 0 elsewhere)
        for r in range(world):
            if layout["name"] == "split-l2":
                assert res["reach"][r][0] >= widest[r][0] and res["reach"][r][1] >= widest[r][1], (name, r, res["reach"], widest)
            else:
                assert res["reach"][r] == (0, 0)
    if mode == 1:
        assert res["paths"] == [1] * world
        if must:
            assert res["err"] == [1] * world and res["rc"] == EXIT_ERR_STATE, f"{name}: the oracle needs {must} outside the halo"
        assert (res["rc"] == EXIT_ERR_STATE) == (res["err"][0] == 1) == (res["any_flag"][0] == 1)
        if res["err"][0]:
            assert int(res["kv"]["compared_ranks"]) == 0
            return
    else:
        assert res["err"] == [0] * world
        if mode == 2 or rs == sc.IID or must:
            assert res["paths"] == [2] * world, f"{name}: path {res['paths']}, the oracle needs {must} outside the halo"
        if mode == 0 and rs != sc.IID:
            assert (res["paths"][0] == 2) == (res["any_flag"][0] == 1)
    if layout["name"] == "2xBl4" and rs != sc.IID and mode != 2:
        # reach = margin = the whole share: rank 0's rows are tiles [-4, 7] and rank 1's [0, 11], so every window of the 8 tiles lies inside
        # both halos -- the collapse's [0, 0] (systematic, stratified) and even the multinomial [0, 7].  The fixed halo MUST hold, whatever
        # the case; 2xBl5, one tile more per rank, must leave it (MUST_LEAVE).  The `>` of the margin comparison itself is pinned by
        # test_window_check_kernel_decides_at_the_margin.
        assert res["paths"] == [1] * world and res["any_flag"] == [0] * world and res["err"] == [0] * world, (name, res["paths"], res["own_flag"])
    if rs == sc.IID:
        # unsorted targets: every rank receives every tile it does not own, at every step that resamples
        assert res["exch"] == [(B - own[r]) * len(sc.resampled_steps(case, T)) for r in range(world)]
    if world == 1:
        assert res["exch"] == [0] and res["own_flag"] == [0]
    assert_equals_unsharded(res, world, "cdf")
    assert_equals_oracle(res, run, T, name)


def test_iid_resampler_rejects_the_fixed_halo_only_mode(harness, tmp_path):
    """Unsorted targets need every tile: mode 1 is SSME_ERR_UNSUPPORTED on every rank, before anything is launched."""
    layout = sc.LAYOUTS["4x2"]
    p = subprocess.run([harness, CSV, "4", str(layout["n"]), "4", "0", str(sc.IID), "1", str(sc.SEED)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=60)
    assert p.returncode == 3 and f"shard_run_series: status {ERR_UNSUPPORTED}" in p.stderr, (p.returncode, p.stderr)


BENIGN = dict(sc.CASES["nan-y"], name="benign", y_set={}, expect=dict(nan_steps=()))


@pytest.mark.parametrize("rs", [0, 1])
@pytest.mark.parametrize("lname", ["4x2", "2r-one-particle", "2xBl5"])
def test_handle_recovers_after_a_nan_series(harness, oracle, tmp_path, lname, rs):
    """ssme_pf_shard_run_series(NaN series) and then the benign series on the SAME handles (flags, statistics, the exact path's window
    buffers and the carried scalars of the first run behind them) equals fresh handles: the unsharded filter's bits and the oracle's."""
    layout, case = sc.LAYOUTS[lname], sc.CASES["nan-y"]
    n, T = sc.shape(case, layout)
    yset, zset, theta = sc.overrides(case, T)
    res = run_harness(harness, tmp_path, layout, T, 0, rs, 0, yset=yset, zset=zset, theta=theta, rerun=1)
    assert_one_decision(res)
    assert res["err"] == [0] * layout["world"]
    assert_equals_unsharded(res, layout["world"], "cdf")
    run = sc.oracle_run(oracle, BENIGN, layout, rs)
    assert np.isfinite([run[t][0][0] for t in range(T)]).all()
    assert_equals_oracle(res, run, T, f"benign after nan-y@{lname}-rs{rs}")


LW_RUNS = [(c, l, form) for l in sc.LW_LAYOUTS for c in sc.LW_CASES for form in (0, 1)]
_lw_id = lambda it: f"{it[0]}@{it[1]}-form{it[2]}" if isinstance(it, tuple) else str(it)


@pytest.mark.parametrize("item", LW_RUNS, ids=_lw_id)
def test_liu_west_cpp_driver(harness, oracle, tmp_path, item):
    """ssme_lw_shard_run_series has no exact path: either every rank ends with the unsharded Liu-West filter's bits (and the oracle's),
    or every rank returns SSME_ERR_STATE -- never a mixture -- and the latter is required where the oracle proves a window leaves."""
    cname, lname, form = item
    case, layout = sc.LW_CASES[cname], sc.LAYOUTS[lname]
    world, name = layout["world"], _lw_id(item)
    lst = lambda d: ",".join(f"{t}:{sc._fmt(v)}" for t, v in sorted(d.items())) or "-"
    res = run_harness(harness, tmp_path, layout, sc.LW_T, -1, int(round(sc.LW_DELTA * 1000)), 0, yscale=repr(case["scale"]), form=form,
                      yset=lst(case["y_set"]), zset=lst(case["z_set"]))
    must = sc.lw_must_leave(oracle, case, layout, form)
    path_log(name, layout, res, None, must)
    assert_one_decision(res)
    run = sc.lw_oracle_run(oracle, case, layout, form)
    lls = [run[t][0] for t in range(sc.LW_T)]
    same_bits([res["ref"]], [oracle_sum(lls)], name + ": the unsharded sum against the oracle")
    if must:
        assert res["err"] == [1] * world, f"{name}: the oracle proves a window outside the halo"
    if res["err"][0]:
        assert res["paths"] == [2] * world and res["any_flag"] == [1] * world and int(res["kv"]["compared_ranks"]) == 0
        return
    assert res["paths"] == [1] * world and res["any_flag"] == [0] * world
    assert_equals_unsharded(res, world, "theta")
    d, so = res["dump"], run[sc.LW_T - 1][1]
    same_bits(d["per"], lls, name + ": per-step values")
    same_bits(res["sums"], [oracle_sum(lls)] * world, name + ": the sum on every rank")
    same_bits(d["x"], so["x"], name + ": final particles")
    same_bits(d["theta"], so["theta"], name + ": final parameters")


@pytest.mark.parametrize("item", [(c, l, form) for c, l, form in LW_RUNS], ids=_lw_id)
def test_unsharded_liu_west_equals_oracle(sa, oracle, item):
    """The unsharded side of the comparison above against the oracle's Liu-West filter, built as test_liu_west_edges_gpu.py builds it, with
    the harness's fixed priors: per-step values, the sum, particles and parameters."""
    cname, lname, form = item
    case, layout = sc.LW_CASES[cname], sc.LAYOUTS[lname]
    run = sc.lw_oracle_run(oracle, case, layout, form)
    y, z = sc.lw_series(case)
    lo, hi = oracle.LW_PRIOR_LO, oracle.LW_PRIOR_HI
    cls = sa.svol_lw_2_par if form else sa.svol_lw_1_par
    g = cls(sc.LW_DELTA, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=layout["n"], seed=sc.SEED, transforms=tuple(oracle.LW_TRANSFORMS))
    tot = g.run_series(y, z)
    lls = [run[t][0] for t in range(sc.LW_T)]
    same_bits(g.per_step()[0], lls, _lw_id(item) + ": per_step()")
    same_bits(tot, [oracle_sum(lls)], _lw_id(item) + ": the sum")
    st, so = g.state(0), run[sc.LW_T - 1][1]
    same_bits(st["x"], so["x"], "particles")
    same_bits(st["theta"], so["theta"], "parameters")
    g.close()


# ---- the Python drivers (gloo rehearsal: every rank a process on the one GPU) ------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_workers(script, world, args_of, outs):
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", script), str(r), str(world), str(port), outs[r]] + args_of, env=env)
             for r in range(world)]
    deadline = time.monotonic() + 90                      # one deadline for the whole world, not one per rank
    try:
        for p in procs:
            assert p.wait(timeout=max(1.0, deadline - time.monotonic())) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [np.load(o) for o in outs]


def _window_routes(res, name, world, margin):
    """window_routes as every rank saved it: the same list on every rank (the fit decision is global), every entry one of the two routes.
    World 2: B - Bl = 2 = the margin, so no window can fail to fit -- every draw exchanges in place, and some rank received tiles."""
    per_rank = [[tuple(int(v) for v in row[:-1]) + (str(row[-1]),) for row in r["routes"]] for r in res]
    print(f"SHARDROUTE {name} world {world} routes {per_rank[0]} exchanged {[int(r['exchanged']) for r in res]}")
    assert all(p == per_rank[0] for p in per_rank), per_rank
    assert per_rank[0] and {e[-1] for e in per_rank[0]} <= {"in_place", "assembled"}, per_rank[0]
    if world == 2:
        B, Bl, own, parts = sc.shares(sc.py_layout(2)["n"], 2)
        assert B - Bl <= margin
        assert all(e[-1] == "in_place" for e in per_rank[0]), per_rank[0]
        assert sum(int(r["exchanged"]) for r in res) > 0
    return per_rank[0]


def _py_margin(layout):
    B, Bl, own, parts = sc.shares(layout["n"], layout["world"])
    margin = sc.py_margin(B, Bl, layout["world"])
    assert margin == 2 == sc.halo_margin(Bl, layout["world"])               # the two rules agree on this layout: the oracle's lists apply
    return margin


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cname", ["nan-y", "huge-y"])
def test_python_bootstrap_driver(oracle, tmp_path, cname, world):
    """ShardedParticleFilter.run_series (the host-planned loop: ssme_pf_shard_plan, the halo or the assembled window, ssme_pf_shard_step)
    over a collapsed cloud, Bl = 2: the oracle's bits on every rank, and the route of every draw (window_routes: (t, route)).  World 2
    must stay in place (_window_routes); at world 4 every step of shard_edge_cases.must_leave must be assembled on every rank: the
    oracle's needed reach exceeds the margin there, and the planned window contains the needed one."""
    case, layout = sc.CASES[cname], sc.py_layout(world)
    n, T = sc.shape(case, layout)
    yset, zset, theta = sc.overrides(case, T)
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(world)]
    res = _run_workers("shard_worker.py", world, [str(case["model"]), str(n), str(T), "0", str(sc.SEED), "1", yset, zset, theta], outs)
    run = sc.oracle_run(oracle, case, layout, 0)
    lls = [run[t][0][0] for t in range(T)]
    for r in res:
        same_bits(r["per_step"].reshape(-1), lls, f"{cname} world {world}: per_step()")
        same_bits([float(r["ll"])], [oracle_sum(lls)], "the sum")
    so = run[T - 1][1][0]
    same_bits(np.concatenate([r["x"] for r in res]), so["x"], "final particles")
    np.testing.assert_array_equal(np.concatenate([r["cdf"] for r in res]).astype(np.uint64), so["cdf"])
    np.testing.assert_array_equal(np.concatenate([r["anc"] for r in res]).astype(np.uint32), so["anc"])
    routes = _window_routes(res, cname, world, _py_margin(layout))
    assert [t for t, _ in routes] == sc.resampled_steps(case, T)             # one entry per draw that exchanged
    if world == 4:
        must = sc.must_leave(case, layout, 0)
        assert must == {"nan-y": ((3, 2), (3, 3)), "huge-y": ((3, 0), (3, 1))}[cname]
        for t in sorted({t for t, _ in must}):
            assert (t, "assembled") in routes, (t, routes)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cname", ["nan-y", "huge-y"])
def test_python_liu_west_driver(oracle, tmp_path, cname, world):
    """ShardedLiuWest.run_series -- the host-planned loop that run_series_native hands over to when the C++ driver returns
    SSME_ERR_STATE (that hand-over itself needs one GPU per rank) -- over a collapsed cloud: the oracle's bits on every rank, and the
    route of every draw (window_routes: (t, which, route)).  World 2 must stay in place (_window_routes); at world 4 the resampling draw
    (which = 0) of every step in shard_edge_cases.lw_must_leave_steps must be assembled on every rank.  That list does not cover the k draw
    (which = 1) nor the steps whose ancestors span several tiles (all of huge-y): those draws are held to rank agreement only."""
    case, layout = sc.LW_CASES[cname], sc.py_layout(world)
    lst = lambda d: ",".join(f"{t}:{sc._fmt(v)}" for t, v in sorted(d.items())) or "-"
    outs = [str(tmp_path / f"lw_rank{r}.npz") for r in range(world)]
    res = _run_workers("shard_worker_lw.py", world, [str(layout["n"]), str(sc.LW_T), str(sc.SEED), repr(sc.LW_DELTA), "0", "1", lst(case["y_set"]),
                                                       lst(case["z_set"]), repr(case["scale"])], outs)
    run = sc.lw_oracle_run(oracle, case, layout, 0)
    lls = [run[t][0] for t in range(sc.LW_T)]
    for r in res:
        same_bits(r["per_step"].reshape(-1), lls, f"{cname} world {world}: per_step()")
        same_bits([float(r["ll"])], [oracle_sum(lls)], "the sum")
    so = run[sc.LW_T - 1][1]
    same_bits(np.concatenate([r["x"] for r in res]), so["x"], "final particles")
    same_bits(np.concatenate([r["theta"] for r in res], axis=1), so["theta"], "final parameters")
    routes = _window_routes(res, "lw " + cname, world, _py_margin(layout))
    assert [(t, which) for t, which, _ in routes] == [(t, which) for t in range(1, sc.LW_T) for which in (0, 1)]   # form 0, rs 1: two draws per step
    if world == 4:
        for t in sc.lw_must_leave_steps(oracle, case, layout, 0):
            assert (t, 0, "assembled") in routes, (t, routes)
