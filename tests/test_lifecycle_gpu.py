"""Handle life cycles on the device: every hand-written scenario (H1 - H8) and every seeded walk of tests/lifecycle_cases.py on one
handle per (run, shape), H9 (create and destroy churn) on its own.  After EVERY op what the op returned is compared (step values,
log-likelihoods; NaN for NaN, -0 is not +0), after every state-changing or refused op loglik(), per_step() with T' <= T, state() of every
filter (x and the integer cdf, tile sums and maxima, m, S; Liu-West: x, theta) and one rotating reader -- bit for bit against the host
model's oracle values (lifecycle_cases.HandleModel / OracleMemo: oracle.Filter / oracle.LWFilter built fresh from the model's seed and
theta and fed the model's history), or, for the readers the oracle does not restate (expectations_multi, weights, sim_future_obs,
swarm_aggregate, log_mean_exp; Liu-West expectations, param_means, weights, sim_future_obs), against a FRESH device handle that
replays the same history through the step API with eager launches: their summation trees are fixed, so the bits must agree.  At the
end of each hand-written scenario those readers are also held once to the budgets of expect_ref.py.  A mismatch names the op index
and the ops before it.  Nothing here provokes a fault: every call is a valid one, or one the library refuses before it touches HIP.
test_lifecycle_cpu.py proves without a GPU that every scenario reaches the host path it is written for."""
import ctypes as C

import numpy as np
import pytest

import lifecycle_cases as L
import test_bootstrap_edges_gpu as teb
import test_expectations_gpu as teg
import test_liu_west_edges_gpu as tle
from test_liu_west_edges_gpu import same_bits

pytestmark = pytest.mark.gpu
sa = teg.sa
RUNS = L.all_runs()


@pytest.fixture(scope="module")
def memo(oracle):
    return L.OracleMemo(oracle)


class Device:
    """One handle of a shape, and the ops of lifecycle_cases.py as calls on it."""

    def __init__(self, sa, oracle, s, seed=L.SEED):
        from ssme_amd import _capi
        self.s, self.capi, self.lib, self.stream = s, _capi, _capi.lib(), None
        self.lw = s["kind"] == "lw"
        if self.lw:
            lo, hi = oracle.LW_PRIOR_LO, oracle.LW_PRIOR_HI
            self.h = (sa.svol_lw_2_par if s["form"] else sa.svol_lw_1_par)(s["delta"], lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=s["n"],
                                                                           n_filters=s["R"], seed=seed, transforms=tuple(oracle.LW_TRANSFORMS), rs=s["rs"])
            if s["split"] is not None:
                self.h.set_debug(False, split_level2=s["split"])
        else:
            self.h = sa.ParticleFilterBank(s["model"], s["n"], s["R"], seed, s["rs"], s["sched"], tile=s["tile"], dtype=_capi.F32 if s["f32"] else _capi.F64)
            assert (self.h.tile, self.h.n_tiles) == (s["tile"], s["B"])
            if s["split"] is not None:
                self.h.set_debug(False, False, split_level2=s["split"])

    def close(self):
        self.h.close()

    def _refused(self, what, t):
        capi, lib, h, one = self.capi, self.lib, self.h._h, np.zeros(max(self.s["R"], 9))
        if what == "series_T0":
            fn = lib.ssme_lw_run_series if self.lw else lib.ssme_pf_run_series
            assert fn(h, capi.dptr(one), None, 0, capi.dptr(one)) == capi.ERR_LENGTH
        elif what == "params_length":
            th = np.append(L.theta_arg(self.s, "one"), 0.5)
            assert lib.ssme_pf_set_params(h, capi.dptr(th), th.size, 1) == capi.ERR_INVALID_ARG
            th = np.tile(L.theta_arg(self.s, "one"), self.s["R"] + 1)
            assert lib.ssme_pf_set_params(h, capi.dptr(th), th.size // (self.s["R"] + 1), self.s["R"] + 1) == capi.ERR_INVALID_ARG
        elif what == "tuning":
            assert lib.ssme_pf_set_tuning(h, 384) == capi.ERR_INVALID_ARG
            if self.s["tile"] != 2048:
                assert lib.ssme_pf_set_tuning(h, 1024) == capi.ERR_UNSUPPORTED
        elif what == "five_functionals":
            fs = np.array([0, 1, 2, 3, 0], dtype=np.int32)
            rc = lib.ssme_pf_get_expectations_multi(h, fs.ctypes.data_as(C.POINTER(C.c_int32)), 5, capi.dptr(np.zeros(5 * self.s["R"])))
            assert rc == (capi.ERR_INVALID_ARG if t >= 1 else capi.ERR_STATE)
        elif what == "functional_id_8":
            fs = np.array([0, 8], dtype=np.int32)
            assert lib.ssme_lw_get_expectations(h, fs.ctypes.data_as(C.POINTER(C.c_int32)), 2, capi.dptr(np.zeros(2 * self.s["R"]))) == capi.ERR_INVALID_ARG
        else:
            raise ValueError(what)

    def do(self, op, t=0):
        """The call of a state-changing or refused op; returns what it returned."""
        k, s, h, capi = op[0], self.s, self.h, self.capi
        if k == "refused":
            return self._refused(op[1], t)
        if k == "set_params":
            return h.set_params(L.theta_arg(s, op[1]))
        if k in ("set_seed", "set_graph_mode", "set_small_series", "set_tuning"):
            return getattr(h, k)(op[1])
        if k in ("reset", "lw_reset"):
            return h.reset()
        if k in ("series", "lw_series"):
            y, z = L.obs(s, op[2], op[1])
            return h.run_series(y, z if op[3] else None)
        if k == "step":
            return np.array([h.step(y, z if op[3] else None) for y, z in (L.step_obs(s, op[2] + j) for j in range(op[1]))])
        if k == "step_queued":                    # logcondlike_out = NULL: the C ABI itself, the Python class always asks for the results
            for j in range(op[1]):
                y, z = L.step_obs(s, op[2] + j)
                yv, zv = np.array([y]), (np.array([z]) if op[3] else None)
                capi.check(self.lib.ssme_pf_step(h._h, capi.dptr(yv), capi.dptr(zv), None), h._h)
            return None
        if k == "lw_filter":
            out = []
            for j in range(op[1]):
                h.filter(*L.step_obs(s, op[2] + j))
                out.append(h._last.copy())
            return np.array(out)
        if k == "set_debug":
            return h.set_debug(op[1], op[2], split_level2=op[3])
        if k == "lw_set_debug":
            return h.set_debug(op[1], split_level2=op[2])
        if k == "set_stream":
            import torch
            if op[1]:
                self.stream = torch.cuda.Stream()
            capi.check(self.lib.ssme_pf_set_stream(h._h, C.c_void_p(self.stream.cuda_stream) if op[1] else None), h._h)
            return None
        raise ValueError(op)

    def per_step(self, Tp):
        out = np.empty((self.s["R"], Tp))
        fn = self.lib.ssme_lw_get_per_step if self.lw else self.lib.ssme_pf_get_per_step
        self.h._chk(fn(self.h._h, self.capi.dptr(out), Tp))
        return out

    def read(self, what, last_y=0.0):
        h, R = self.h, self.s["R"]
        if what == "loglik":
            if not self.lw:
                return h.loglik()
            out = np.empty(R)
            h._chk(self.lib.ssme_lw_get_loglik(h._h, self.capi.dptr(out)))
            return out
        if what == "state":
            return [h.state(r) if self.lw else h.state(r, logw=False) for r in range(R)]
        if what == "state_anc":
            return [h.state(r, ancestors=True, logw=False)["anc"] for r in range(R)]
        if what == "state_logw":
            return [h.state(r, logw=True)["logw"] for r in range(R)]
        if what == "state_idx":
            return [h.state(r, indices=True) for r in range(R)]
        if what == "expectations_multi":
            return h.expectations_multi([0, 1, 2, 3])
        if what == "expectations":
            return h.expectations(list(range(8)))
        if what == "param_means":
            return h.param_means()
        if what == "weights":
            return [h.weights(r) for r in range(R)]
        if what == "sim_future_obs":
            return h.sim_future_obs(2, last_y, states=True, start=True)
        if what == "swarm_aggregate":
            return h.swarm_aggregate([0, 1, 2, 3], num_threads=2)
        if what == "log_mean_exp":
            return h.log_mean_exp()
        raise ValueError(what)


def _flat(v):
    if isinstance(v, dict):
        return [a for k in sorted(v) if v[k] is not None for a in _flat(v[k])]
    if isinstance(v, (list, tuple)):
        return [a for x in v for a in _flat(x)]
    return [np.atleast_1d(np.asarray(v))]


def same(got, want, what):
    g, w = _flat(got), _flat(want)
    assert len(g) == len(w), what
    for i, (a, b) in enumerate(zip(g, w)):
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            same_bits(a, b, f"{what} [{i}]")
        else:
            np.testing.assert_array_equal(a, b, err_msg=f"{what} [{i}]")


_FRESH = {}


def fresh_read(sa, oracle, m, what):
    """`what` read from a fresh handle that replays the model's history through the step API, eager launches."""
    key = (m.key(), what)
    if key not in _FRESH:
        d = Device(sa, oracle, m.s, seed=m.seed)
        try:
            if not m.lw:
                d.h.set_graph_mode(False)
                d.h.set_params(m.theta)
            for y, z in m.hist:
                if m.lw:
                    d.h.filter(y, z)
                else:
                    d.h.step(y, z if m.s["model"] == L.LEV else None)
            _FRESH[key] = d.read(what, m.hist[-1][0])
        finally:
            d.close()
        if m.s["n"] > L.BIG_N:                   # nothing large is kept
            return _FRESH.pop(key)
    return _FRESH[key]


def check_reader(sa, oracle, memo, dev, m, what, arg=None):
    lw = m.lw
    if what == "loglik":
        want = m.round_out(L.running_sum(memo.of(m)["lls"])) if m.hist else np.zeros(m.s["R"])
        return same(dev.read("loglik"), want, "loglik()")
    if what == "per_step":
        T = len(m.series_rec[2])
        Tp = T if arg is None else arg
        return same(dev.per_step(Tp), memo.per_step(m)[:, :Tp], f"per_step({Tp}) of the last series, T = {T}")
    got = dev.read(what, m.hist[-1][0])
    st = memo.of(m)["states"]
    if what == "state":
        for r, (g, o) in enumerate(zip(got, st)):
            if lw:
                same_bits(g["x"], o["x"], f"state() r={r}: particles")
                same_bits(g["theta"], o["theta"], f"state() r={r}: parameters")
            else:
                teb.compare_state(g, o, f"state() r={r}", False, logw=False)
    elif what in ("state_anc", "state_logw", "state_idx"):
        expect = m.logw_expect if what == "state_logw" else m.anc_expect
        for r, g in enumerate(got):
            for k in (("kidx", "anc") if lw else (None,)):
                a = g if k is None else g[k]
                if expect == "zeros":
                    assert not np.asarray(a).any(), f"{what} r={r} {k}: a buffer allocated zeroed and not written since"
                elif expect == "oracle":
                    same(a, st[r]["logw" if what == "state_logw" else (k or "anc")], f"{what} r={r} {k}")
    else:
        same(got, fresh_read(sa, oracle, m, what), f"{what} against a fresh handle that replays the history")


def check_return(memo, m, op, got):
    k = op[0]
    if k in ("step", "lw_filter"):
        same(got, m.round_out(memo.of(m)["lls"][:, -op[1]:].T), "the values the steps returned")
    elif k in ("series", "lw_series"):
        same(got, m.round_out(L.running_sum(memo.of(m)["lls"])), "the sum run_series returned")


def after_op(sa, oracle, memo, dev, m, i):
    check_reader(sa, oracle, memo, dev, m, "loglik")
    if m.series_rec is not None:
        T = len(m.series_rec[2])
        check_reader(sa, oracle, memo, dev, m, "per_step", (T, 1, (T + 1) // 2)[i % 3])
    if m.t >= 1:
        check_reader(sa, oracle, memo, dev, m, "state")
        rot = L.LW_ROTATING if m.lw else L.ROTATING
        check_reader(sa, oracle, memo, dev, m, rot[i % len(rot)])


def final_budgets(oracle, memo, dev, m, name):
    """The readers the oracle does not restate, once against the budgets of expect_ref.py (fp64 boundary only)."""
    if m.t < 1 or m.s["f32"]:
        return
    for r, so in enumerate(memo.of(m)["states"]):
        if m.lw:
            tle.check_readouts(dev.h, oracle, m.s, r, so, f"{name} r={r}")
        else:
            teb.check_readouts(dev.h, oracle, so, m.s["tile"], r, f"{name} r={r}")


def run_ops(sa, oracle, memo, s, ops, name, dev=None, m=None, budgets=False):
    own = dev is None
    dev = Device(sa, oracle, s) if own else dev
    m = L.HandleModel(s) if m is None else m
    try:
        for i, op in enumerate(ops):
            try:
                assert m.legal(op)
                if op[0] == "read":
                    check_reader(sa, oracle, memo, dev, m, op[1], op[2] if len(op) > 2 else None)
                    continue
                got = dev.do(op, m.t)
                m.apply(op)
                check_return(memo, m, op, got)
                after_op(sa, oracle, memo, dev, m, i)
            except AssertionError as e:
                raise AssertionError(f"{name}: op {i} {op} after {ops[:i]}:\n{e}") from e
        if budgets:
            final_budgets(oracle, memo, dev, m, name)
    finally:
        if own:
            dev.close()
    return dev, m


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_any_call_order_equals_fresh_handles(sa, oracle, memo, run):
    rid, name, ops = run
    run_ops(sa, oracle, memo, L.SHAPES[name], ops, rid, budgets=rid.startswith("H"))


def test_h9_create_and_destroy_churn(sa, oracle, memo):
    """H9: 40 handles of four shapes, three alive at a time (the raise-only LDS grants and the allocator's reuse of freed buffers, as
    test_handle_coexistence_gpu.py, but against the model's values): each runs a series when created and is read again, and stepped,
    after two younger handles were created and run; then it is destroyed."""
    alive = []

    def retire():
        dev, m, s, i = alive.pop(0)
        run_ops(sa, oracle, memo, s, [("read", "state"), ("lw_filter", 1, 0) if m.lw else ("step", 1, 0, True if s["model"] == L.LEV else False)],
                f"H9 handle {i} ({s['name']}) when retired", dev, m)
        dev.close()

    try:
        for i, (name, seed, n_alive) in enumerate(L.churn_plan()):
            assert len(alive) == n_alive
            s = L.SHAPES[name]
            dev, m = Device(sa, oracle, s, seed=seed), L.HandleModel(s)
            m.seed = seed
            alive.append((dev, m, s, i))
            run_ops(sa, oracle, memo, s, L._start(s) + [L._ser(s, 5 + i % 2, i % 3)], f"H9 handle {i} ({name})", dev, m)
            if len(alive) == 3:
                retire()
        while alive:
            retire()
    finally:
        for dev, _, _, _ in alive:
            dev.close()
