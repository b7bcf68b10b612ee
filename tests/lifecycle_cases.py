"""Handle life cycles: any call order on ONE handle must give what fresh handles give (tests/test_lifecycle_gpu.py; checked without a
GPU by tests/test_lifecycle_cpu.py).  This file holds the vocabulary of calls (ops), the host model of a handle, the shapes, one
hand-written scenario per hazard (H1 - H9) and the seeded random walks.

An OP is a tuple, its first entry the name:
  state-changing, bootstrap     ("set_params", how)        how = "one" (one shared row), "rows" (R rows), "second" (another theta, one row)
                                ("set_seed", seed)  ("reset",)
                                ("series", T, s, z)        observations obs(s, T); z = True: their lag as covariates, False: z = None
                                ("step", k, i0, z)         k steps with observations step_obs(i0 ..), results returned
                                ("step_queued", k, i0, z)  the same with logcondlike_out = NULL: nothing returned, nothing waited for
                                ("set_graph_mode", on)  ("set_debug", ancestors, keep_logw, split)  ("set_tuning", threads)
                                ("set_small_series", on)  ("set_stream", on)   on = a caller's stream, off = back to NULL
  state-changing, Liu-West      ("lw_reset",)  ("lw_filter", k, i0)  ("lw_series", T, s, z)  ("lw_set_debug", on, split)
  readers                       ("read", what[, arg])      READERS / LW_READERS below
  refused calls                 ("refused", what)          REFUSED below; the handle must be exactly what it was

HandleModel tracks what a handle SHOULD be from the documented contract alone (include/ssme_pf.h): configuration, seed, theta rows,
debug flags, t, and the observations and covariates fed since the last reset (set_params, set_seed, reset and every run_series reset).
Expected values never come from the handle under test: OracleMemo feeds the model's history to oracle.Filter / oracle.LWFilter built
fresh from the model's (seed, theta), memoised on (shape, seed, theta, history).  Beside the contract the model restates the host
bookkeeping of csrc/pf_api.hip and csrc/handle_core.h that no result shows when it is right -- which run_series replays the captured
graph and which captures anew (the five key fields of ssme_pf_run_series plus "no drop since"), which call grows which buffer, which
step redraws the Gamma-table chunk -- as EVENTS, so that test_lifecycle_cpu.py can assert that every scenario reaches what it is for.

SHAPES are the smallest at which each route exists, taken from bs_edge_cases.routes() / lw_edge_cases by name where they have one."""
import os
import random

import numpy as np

import bs_edge_cases as bc
import lw_edge_cases as lc

ROOT = bc.ROOT
SVOL, LEV = bc.MODEL_SVOL, bc.MODEL_SVOL_LEVERAGE
SEED = bc.SEED
SERIES_T = (1, 2, 5, 6, 63, 64, 65, 130)
KEY_FIELDS = ("T", "has_z", "debug", "logw", "nt")          # g_T, g_has_z, g_debug, g_logw, g_nt of ssme_pf_run_series
CHUNK = 64                                                   # kStepGammaChunk
BIG_N = bc.BIG_N
TH = {SVOL: ((1.0, 0.95, 0.25), (0.8, 0.9, 0.3)), LEV: ((0.9, 0.0, 1.0, -0.1), (0.95, 0.1, 0.8, -0.3))}
PHI = {SVOL: 1, LEV: 0}                                      # index of phi: row r of "rows" has phi - 0.01 r

READERS = ("loglik", "per_step", "state", "state_anc", "state_logw", "expectations_multi", "weights", "sim_future_obs",
           "swarm_aggregate", "log_mean_exp")
ROTATING = ("expectations_multi", "weights", "sim_future_obs", "swarm_aggregate", "log_mean_exp")   # the oracle does not restate these
LW_READERS = ("loglik", "per_step", "state", "state_idx", "expectations", "param_means", "weights", "sim_future_obs")
LW_ROTATING = ("expectations", "param_means", "weights", "sim_future_obs")
REFUSED = ("series_T0", "params_length", "tuning", "five_functionals")
LW_REFUSED = ("series_T0", "functional_id_8")
BS_CLASSES = ("set_params_one", "set_params_rows", "set_params_second", "set_seed", "reset", "series_z", "series_noz", "step",
              "step_queued", "set_graph_mode", "set_debug", "set_tuning", "set_small_series", "set_stream")
LW_CLASSES = ("lw_reset", "lw_filter", "lw_series_z", "lw_series_noz", "lw_set_debug")


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
def _bs(name, model, n, tile, R, rs, sched=1, split=None, f32=False, tmax=130, walk_ops=25):
    tile = tile or bc.default_tile(n, R)
    return dict(name=name, kind="bs", model=model, n=n, tile=tile, B=-(-n // tile), R=R, rs=rs, sched=sched, split=split, f32=f32, tmax=tmax,
                walk_ops=walk_ops)


def _lw(n, R, form, rs, split):
    return dict(name=f"lw-{n}-form{form}-rs{rs}" + ("-split" if split else ""), kind="lw", n=n, tile=lc.TILE, B=lc.tiles(n), R=R, form=form,
                rs=rs, split=split, f32=False, tmax=130, walk_ops=25, delta=0.99)


def shapes():
    r = {x["name"]: x for x in bc.routes()}
    n5 = 4 * 2048 + 77                                       # five tiles of 2048, the last one ragged
    s = [
        _bs("small-100", SVOL, r["small-100"]["n"], 0, 3, 0),                                  # lane kernel
        _bs("pair-1500", LEV, 1500, 0, 2, 1),                                                   # pair kernel, systematic
        _bs("wl2-512", LEV, r["wl2-512"]["n"], r["wl2-512"]["tile"], 1, 0),
        _bs("tiles5-2048", LEV, n5, 2048, 2, 0),                                                # set_tuning has a choice here
        _bs("split-forced-5", SVOL, n5, 2048, 1, 1, split=r["split-forced-5"]["split"]),
        _bs("tables-5", SVOL, n5, 2048, 1, 0, split=r["tables-5"]["split"]),
        _bs("split-1025", SVOL, r["split-1025"]["n"], r["split-1025"]["tile"], 1, 0, tmax=6, walk_ops=8),
        _bs("sched3-mult", LEV, r["wl2-512"]["n"], 512, 2, 0, sched=3),
        _bs("sched3-sys", LEV, r["wl2-512"]["n"], 512, 1, 1, sched=3),
        _bs("f32-lev", LEV, r["wl2-512"]["n"], 512, 1, 0, f32=True),
    ]
    for n, R in ((300, 2), (3 * 2048 + 5, 1)):
        for form, rs, split in ((0, 1, None), (1, 3, None), (0, 3, True), (1, 1, True)):
            s.append(_lw(n, R, form, rs, split))
    return s


SHAPES = {s["name"]: s for s in shapes()}


def allowed_splits(s):
    """Level-2 policies set_debug may force on the shape: one-tile filters keep the default."""
    return (None,) if s["B"] == 1 else (None, True, False, "tables")


def allowed_nt(s):
    """ssme_pf_set_tuning: 512-particle tiles run 256 threads, 1024-particle tiles 512, 2048-particle tiles any of the three."""
    return {512: (256,), 1024: (512,)}.get(s["tile"], (256, 512, 1024))


# ---- observations ------------------------------------------------------------------------------------------------------------------
_SPY = None


def _spy():
    global _SPY
    if _SPY is None:
        _SPY = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    return _SPY


def _lw_base(seed, n):
    return np.random.default_rng(seed).normal(0.0, 0.02, n)


def obs(s, sidx, T):
    """Series number sidx (0, 1, 2): (y[T], lag z[T]).  The three differ from their first row on, so that a stale replay shows."""
    if s["kind"] == "lw":
        y = _lw_base(3 + sidx, 130)[:T].copy()
    else:
        y = _spy()[200 * sidx:200 * sidx + T].copy()
    return y, np.concatenate([[0.0], y[:-1]])


def step_obs(s, i):
    """Observation number i of the step API's own stream, and its lag."""
    if s["kind"] == "lw":
        v = _lw_base(99, 600)
        return float(v[i + 1]), float(v[i])
    return float(_spy()[1000 + i + 1]), float(_spy()[1000 + i])


def theta_arg(s, how):
    """What set_params is given: one row (1-D) or R rows."""
    th = np.asarray(TH[s["model"]][1 if how == "second" else 0], dtype=np.float64)
    if how != "rows":
        return th
    rows = np.repeat(th[None, :], s["R"], axis=0)
    rows[:, PHI[s["model"]]] -= 0.01 * np.arange(s["R"])
    return rows


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- the host model ----------------------------------------------------------------------------------------------------------------
class HandleModel:
    def __init__(self, shape):
        s = self.s = shape
        self.lw = s["kind"] == "lw"
        self.seed = SEED
        self.theta = None                       # [R, n_theta] as the filters see it (float-rounded on an F32 handle)
        self.t, self.hist, self.series_rec = 0, (), None
        self.n_steps = 0                        # observations of the step stream used so far
        self.anc = self.keep_logw = False
        self.graph, self.small, self.stream = True, True, False
        self.nt = 256 if s["tile"] == 512 else 512
        self.mult = self.lw or s["rs"] == 0     # Gamma tables: the multinomial resampler, and both draws of Liu-West
        self.ycap = self.tcap = 1
        self.gcap = 1 if self.mult else 0
        self.gamma_t0 = self.gamma_rows = 0
        self.cause = "first"                    # what emptied the Gamma-table chunk last
        self.gkey = None
        self.policy = (0, 0)
        self.policy = self._policy(s["split"])  # the shape's own policy is set right after creation
        self.anc_alloc, self.logw_alloc = False, (not self.lw and s["sched"] > 1)
        self.anc_expect, self.logw_expect = None, ("unknown" if self.logw_alloc else None)
        self.events = []

    # -- bookkeeping restated from pf_api.hip --------------------------------------------------------------------------------------
    def _policy(self, split):
        """(split_l2, l2_tables) as ssme_pf_set_debug / ssme_lw_set_debug decide them."""
        B = self.s["B"]
        want = 1 if (B > bc.MAX_TILES_PER_FILTER or split is True or split == "tables") else (0 if split is False else int(B > bc.SPLIT_ABOVE_TILES))
        return (want, int(split == "tables" and not self.lw))

    def lw_needed(self):
        return self.keep_logw or self.s.get("sched", 1) > 1

    def _drop(self, why):
        if self.gkey is not None:
            self.events.append("drop:" + why)
        self.gkey = None

    def series_path(self):
        s = self.s
        if self.lw:
            return "eager"
        if s["B"] == 1 and s["tile"] == 2048 and self.small:
            return "small"
        return "graph" if self.graph else "eager"

    def _grow_series(self, T):
        moved = False
        if T > self.ycap:
            self.ycap, moved = T, True
            self.events.append("regrow:ybuf")
        if T > self.tcap:
            self.tcap, moved = T, True
            self.events.append("regrow:per_step")
        if self.mult and T > self.gcap:
            self.gcap = T
            self.events.append("regrow:gamma")
            self._drop("gamma moved")
        if moved:
            self._drop("series buffers moved")

    def _reset(self, cause):
        self.t, self.hist = 0, ()
        self.gamma_rows, self.cause = 0, cause
        if self.anc_expect == "oracle":
            self.anc_expect = "unknown"
        if self.logw_expect == "oracle":
            self.logw_expect = "unknown"

    def _one_step(self, y, z, api):
        """The bookkeeping of one filter step at time index self.t; api: the step API (Gamma tables by chunks)."""
        t, s = self.t, self.s
        if api and self.mult:
            if self.gcap < CHUNK:
                self.gcap = CHUNK
                self.events.append("regrow:gamma")
                self._drop("gamma moved")
            if (not self.lw or t > 0) and (t < self.gamma_t0 or t >= self.gamma_t0 + self.gamma_rows):
                self.events.append("redraw:" + ("chunk-end" if self.gamma_rows and t == self.gamma_t0 + self.gamma_rows else self.cause))
                self.gamma_t0, self.gamma_rows = t, CHUNK
        self.hist += ((y, z),)
        self.t += 1
        resampled = t > 0 and t % s.get("sched", s.get("rs", 1)) == 0
        if self.anc:                            # indices are compared where the step drew them anew; elsewhere they are not part of the model
            self.anc_expect = "oracle" if (resampled and (not self.lw or s["rs"] == 1)) else "unknown"
        elif self.anc_expect == "oracle":
            self.anc_expect = "unknown"
        if not self.lw:
            if self.lw_needed():
                self.logw_expect = "oracle"
            elif self.logw_expect == "oracle":
                self.logw_expect = "unknown"

    def _inputs(self, y, z):
        return (float(_f32(y)), float(_f32(z))) if self.s["f32"] else (float(y), float(z))

    # -- the contract ----------------------------------------------------------------------------------------------------------------
    def legal(self, op):
        k = op[0]
        if k == "read":
            what = op[1]
            if what == "loglik":
                return True
            if what == "per_step":
                return self.series_rec is not None
            if what in ("state_anc", "state_idx"):
                return self.anc_alloc and self.t >= 1
            if what == "state_logw":
                return self.logw_alloc and self.lw_needed() and self.t >= 1
            return self.t >= 1
        if k == "refused":
            return True
        if self.lw:
            return True
        if k in ("step", "step_queued", "reset", "series"):
            return self.theta is not None
        if k == "set_tuning":
            return op[1] in allowed_nt(self.s)
        if k == "set_debug":
            return op[3] in allowed_splits(self.s)
        return True

    def apply(self, op):
        """Advance the model by one op; returns the events the op caused (also appended to self.events)."""
        assert self.legal(op), op
        n0, k, s = len(self.events), op[0], self.s
        if k in ("read", "refused"):
            pass
        elif k == "set_params":
            th = theta_arg(s, op[1])
            th = np.repeat(th[None, :], s["R"], axis=0) if th.ndim == 1 else th
            self.theta = _f32(th) if s["f32"] else th.copy()
            self._reset("set_params")
        elif k == "set_seed":
            self.seed = int(op[1])
            self._reset("set_seed")
        elif k in ("reset", "lw_reset"):
            self._reset("reset")
        elif k in ("series", "lw_series"):
            T, sidx, has_z = op[1], op[2], bool(op[3])
            assert 1 <= T <= s["tmax"]
            self._grow_series(T)
            self._reset("series")
            path = self.series_path()
            if path == "graph":
                key = dict(T=T, has_z=int(has_z), debug=int(self.anc), logw=int(self.lw_needed()), nt=self.nt)
                if self.gkey == key:
                    self.events.append("replay")
                else:
                    diff = [f for f in KEY_FIELDS if self.gkey is not None and self.gkey[f] != key[f]]
                    self.events.append("recapture:" + (",".join(diff) if diff else "no graph"))
                self.gkey = key
            self.events.append(f"series:{path}:{'odd' if T & 1 else 'even'}")
            y, z = obs(s, sidx, T)
            for t in range(T):
                self._one_step(*self._inputs(y[t], z[t] if has_z else 0.0), api=False)
            if path == "small":                 # the one-launch kernels keep neither ancestors nor log-weights
                self.anc_expect = "unknown" if self.anc_expect == "oracle" or self.anc else self.anc_expect
                self.logw_expect = "unknown" if self.logw_expect is not None else None
            self.series_rec = (self.seed, None if self.theta is None else self.theta.copy(), self.hist)
        elif k in ("step", "step_queued", "lw_filter"):
            n, i0 = op[1], op[2]
            has_z = True if self.lw else bool(op[3])
            for j in range(n):
                y, z = step_obs(s, i0 + j)
                self._one_step(*self._inputs(y, z if has_z else 0.0), api=True)
            self.n_steps = max(self.n_steps, i0 + n)
        elif k == "set_graph_mode":
            self.graph = bool(op[1])
        elif k == "set_small_series":
            self.small = bool(op[1])
        elif k == "set_tuning":
            self.nt = int(op[1])
        elif k == "set_stream":
            self.stream = bool(op[1])
            self._drop("set_stream")
        elif k in ("set_debug", "lw_set_debug"):
            anc, keep, split = (op[1], False, op[2]) if self.lw else op[1:4]
            if anc and not self.anc_alloc:
                self.anc_alloc, self.anc_expect = True, "zeros"
                self.events.append("alloc:anc")
            self.anc, self.keep_logw = bool(anc), bool(keep)
            pol = self._policy(split)
            if pol != self.policy:
                self._drop("set_debug policy")
            self.policy = pol
            if not self.lw and self.lw_needed() and not self.logw_alloc:
                self.logw_alloc, self.logw_expect = True, "zeros"
                self.events.append("alloc:logw")
        else:
            raise ValueError(op)
        return self.events[n0:]

    def key(self):
        """What the oracle's values depend on."""
        return (self.s["name"], self.seed, b"" if self.theta is None else self.theta.tobytes(), self.hist)

    def op_class(self, op):
        k = op[0]
        if k == "set_params":
            return "set_params_" + op[1]
        if k in ("series", "lw_series"):
            return k + ("_z" if op[3] else "_noz")
        return k

    def round_out(self, v):
        return _f32(v) if self.s["f32"] else np.asarray(v, dtype=np.float64)


def running_sum(lls):
    """[R, T] -> [R]: 0 + ll_0 + ll_1 + ... in that order, as every accounting kernel adds them."""
    out = np.zeros(lls.shape[0])
    for t in range(lls.shape[1]):
        out = out + lls[:, t]
    return out


class OracleMemo:
    """oracle.Filter / oracle.LWFilter runs of (shape, seed, theta, history), each computed once.  A history that extends the one
    last run for its (shape, seed, theta) continues that run."""

    def __init__(self, oracle):
        self.o, self.live, self.cache = oracle, {}, {}

    def _make(self, s, seed, theta):
        o = self.o
        if s["kind"] == "lw":
            return [o.LWFilter(s["n"], seed, rep=r, delta=s["delta"], form=s["form"], resamp_sched=s["rs"]) for r in range(s["R"])]
        return [o.Filter(s["model"], s["n"], theta[r], seed, rep=r, resampler=s["rs"], resamp_sched=s["sched"], tile=s["tile"]) for r in range(s["R"])]

    def run(self, s, seed, theta, hist, states=True):
        """dict(lls [R, len(hist)], states [R] or None for an empty history or where states = False)"""
        key = (s["name"], seed, b"" if theta is None else np.asarray(theta).tobytes(), hist)
        if key in self.cache and (not states or not hist or self.cache[key]["states"] is not None):
            return self.cache[key]
        big = s["n"] > BIG_N
        if big:                                  # at most one large run held, and the states of one large result
            self.live = {k: v for k, v in self.live.items() if k == key[:3]}
            for k, v in self.cache.items():
                if SHAPES[k[0]]["n"] > BIG_N:
                    v["states"] = None
        live = self.live.get(key[:3])
        if live is not None and not states and hist == live["hist"][:len(hist)]:         # a prefix of the run held: its values are there
            lls = np.array(live["lls"][:len(hist)], dtype=np.float64).reshape(len(hist), s["R"]).T.copy()
            return self.cache.setdefault(key, dict(lls=lls, states=None))
        if live is None or live["hist"] != hist[:len(live["hist"])]:
            live = self.live[key[:3]] = dict(fs=self._make(s, seed, theta), hist=(), lls=[])
        for y, z in hist[len(live["hist"]):]:
            live["lls"].append([f.step(y, z) for f in live["fs"]])
        live["hist"] = hist
        lls = np.array(live["lls"], dtype=np.float64).reshape(len(hist), s["R"]).T.copy()
        res = dict(lls=lls, states=[f.state() for f in live["fs"]] if hist and states else None)
        self.cache[key] = res
        return res

    def of(self, m):
        return self.run(m.s, m.seed, m.theta, m.hist)

    def per_step(self, m):
        seed, theta, hist = m.series_rec
        return m.round_out(self.run(m.s, seed, theta, hist, states=False)["lls"])


# ---- the hand-written scenarios: one per hazard ---------------------------------------------------------------------------------
def _is(s, **kw):
    return all(s.get(k) == v for k, v in kw.items())


def _start(s):
    return [] if s["kind"] == "lw" else [("set_params", "one")]


def _ser(s, T, sidx, z=True):
    return ("lw_series", T, sidx, z) if s["kind"] == "lw" else ("series", T, sidx, bool(z and s["model"] == LEV))


class _Steps:
    """Hands out consecutive observations of the step stream."""

    def __init__(self, s):
        self.s, self.i = s, 0

    def __call__(self, k, queued=False, z=True):
        i0, self.i = self.i, self.i + k
        if self.s["kind"] == "lw":
            return ("lw_filter", k, i0)
        return ("step_queued" if queued else "step", k, i0, bool(z and self.s["model"] == LEV))


def h1_graph_key(s):
    """Guards ssme_pf_run_series' replay condition (pf_api.hip: `if (!h->gexec || h->g_T != T || ...)`), the drops in ssme_pf_set_debug,
    ssme_pf_set_stream, ensure_gamma_capacity and ensure_series_capacity, and what must survive a replay: Tcap in the captured
    arguments, the key and model constants in place on the device, `h->cur = (T & 1)`."""
    if s["kind"] == "lw" or s["B"] == 1 or s["tmax"] < 130:
        return None
    lev = s["model"] == LEV
    o = _start(s) + [_ser(s, 6, 0), _ser(s, 130, 1), _ser(s, 6, 2), _ser(s, 6, 0)]                          # g_T; the larger T first grows
    if lev:
        o += [_ser(s, 6, 1, z=False), _ser(s, 6, 2, z=False), _ser(s, 6, 1)]                                  # g_has_z
    nts = [n for n in allowed_nt(s) if n != (256 if s["tile"] == 512 else 512)]
    for nt in nts[:1]:
        o += [("set_tuning", nt), _ser(s, 6, 2), _ser(s, 6, 0), ("set_tuning", 512), _ser(s, 6, 1)]             # g_nt
    sp = s["split"]
    o += [("set_debug", False, True, sp), _ser(s, 6, 2), _ser(s, 6, 0), ("read", "state_logw"),                 # g_logw
          ("set_debug", True, True, sp), _ser(s, 6, 1), _ser(s, 6, 0), ("read", "state_anc"),                   # g_debug
          ("set_debug", False, False, sp), _ser(s, 6, 2), ("set_seed", 11), _ser(s, 6, 2), ("set_params", "second"), _ser(s, 6, 2)]
    for pol in (True, "tables", False, None, sp):                                                             # the policy drops the graph
        o += [("set_debug", False, False, pol), _ser(s, 5, 0), _ser(s, 5, 1)]
    o += [("set_graph_mode", False), _ser(s, 5, 2), ("set_graph_mode", True), _ser(s, 5, 0), ("set_graph_mode", False), _ser(s, 6, 1),
          ("set_graph_mode", True)]
    o += [("set_stream", True), _ser(s, 6, 2), _ser(s, 6, 0), ("set_stream", False), _ser(s, 6, 1), _ser(s, 6, 2)]
    return o


def h2_regrowth(s):
    """Guards the separate growth of ybuf / zbuf (ycap), per_step (tcap, laid out [R][tcap]), the Gamma tables (gcap; the step APIs
    raise it to kStepGammaChunk on their own) and small_ms in ensure_series_capacity / ensure_gamma_capacity / lw_ensure_capacity /
    ensure_series_buffers, read_per_step's stride, and the late Mem::zeroed allocations of set_debug behind queued steps."""
    if s["tmax"] < 130:
        return None
    st, lw = _Steps(s), s["kind"] == "lw"
    o = _start(s) + [st(2)]                                                                                   # gcap -> 64 while tcap = 1
    if lw:
        o += [("lw_set_debug", True, s["split"]), ("read", "state_idx"), st(1), ("read", "state_idx")]
    else:
        o += [st(2, queued=True), ("set_debug", True, True, s["split"]), ("read", "state_anc"), ("read", "state_logw"), st(1),
              ("read", "state_anc"), ("read", "state_logw"), ("set_debug", False, False, s["split"])]
    o += [_ser(s, 5, 0), ("read", "per_step", 5), _ser(s, 65, 1), ("read", "per_step", 5), _ser(s, 130, 2), _ser(s, 6, 0), ("read", "per_step", 5),
          ("read", "per_step", 6), st(2)]
    return o


def h3_covariates(s):
    """Guards `a.z = has_z ? h->zbuf : nullptr` (enqueue_step), the zeroed zbuf of ensure_series_buffers and the hipMemsetAsync of zbuf
    in ssme_lw_run_series: a series without covariates after a longer one with them must equal z = 0."""
    if s["tmax"] < 130 or (s["kind"] == "bs" and s["model"] != LEV):
        return None
    st = _Steps(s)
    return _start(s) + [_ser(s, 130, 0), _ser(s, 6, 1, z=False), st(2, z=False), ("read", "state"), _ser(s, 6, 2), _ser(s, 5, 1, z=False), st(1)]


def h4_gamma(s):
    """Guards step_gamma_row (handle_core.h), `gamma_rows = 0` in do_reset / lw_reset, and that run_series leaves its own rows in the
    tables without claiming them: steps across t = 63 / 64 / 65, set_seed and reset in mid-chunk, steps continuing a series."""
    m = HandleModel(s)
    if not m.mult or s["tmax"] < 130:
        return None
    st, lw = _Steps(s), s["kind"] == "lw"
    # a new seed while t = 0 .. 2 still lies inside the chunk drawn for the old one: only gamma_rows = 0 makes the steps redraw
    o = _start(s) + ([st(3)] if lw else [st(3), ("set_seed", 14), st(3)]) + [st(60), st(3), st(1)]
    o += ([] if lw else [("set_seed", 12), st(2)]) + [("lw_reset",) if lw else ("reset",), st(2)]
    o += [_ser(s, 5, 0), st(2), _ser(s, 65, 1), st(2), st(62), st(2), _ser(s, 6, 2), st(1)]
    if not lw:
        o += [("set_params", "rows"), st(2)]
    return o


def h5_parity(s):
    """Guards the ping-pong parity: `h->cur = (T & 1)` after a replay, `h->cur ^= 1` per enqueued step, `h->cur = 1` after the one-launch
    kernels, the std::swap of xB / xr per queued Liu-West step: every reader and a further step must find the right half."""
    st = _Steps(s)
    if s["kind"] == "lw":
        return [st(3), ("read", "state"), ("lw_reset",), _ser(s, 5, 0), ("read", "state"), ("read", "expectations"), st(1), _ser(s, 6, 1),
                ("read", "sim_future_obs"), st(2), ("read", "weights"), _ser(s, 2, 2, z=False), st(1)]
    forms = [("small", [("set_small_series", True)])] if s["B"] == 1 else []
    forms += [("graph", [("set_small_series", False), ("set_graph_mode", True)]), ("eager", [("set_graph_mode", False)])]
    o = _start(s)
    for _, pre in forms:
        o += pre
        for T in (5, 6) if s["n"] <= BIG_N else (1, 2):           # the parities alone matter; the oracle dominates the large shape
            o += [_ser(s, T, T % 3), ("read", "state"), ("read", "expectations_multi"), ("read", "sim_future_obs"), st(1), ("read", "weights")]
    return o


def h6_queued(s):
    """Guards "every later call on the handle is ordered behind it" for ssme_pf_step with logcondlike_out = NULL: each reader, and
    set_seed, right behind steps that nobody waited for."""
    if s["kind"] == "lw":
        return None
    st, k = _Steps(s), (2 if s["n"] <= BIG_N else 1)          # the oracle's time on the large shape: one queued step each, T = 2
    o = _start(s) + [_ser(s, 6 if k == 2 else 2, 0)]
    for rd in ("loglik", "per_step", "state", "expectations_multi", "weights", "sim_future_obs", "swarm_aggregate", "log_mean_exp"):
        o += [st(k, queued=True), ("read", rd)]
    return o + [st(k, queued=True), ("set_seed", 13), st(1), st(1, queued=True), ("reset",), st(1)]


def h7_theta_rows(s):
    """Guards the row choice of ssme_pf_set_params (`n_rows == 1 ? 0 : r`) and the model constants that stay in place on the device
    under a captured graph."""
    if s["kind"] == "lw":
        return None
    st, T = _Steps(s), min(5, s["tmax"])
    return [("set_params", "one"), st(2), _ser(s, T, 0), ("set_params", "rows"), _ser(s, T, 0), st(2), ("set_params", "one"), _ser(s, T, 0),
            ("set_params", "second"), _ser(s, T, 0), st(1)]


def h8_refused(s):
    """Guards the argument checks that come before any HIP call (ssme_pf_run_series T < 1, ssme_pf_set_params length,
    ssme_pf_set_tuning, enqueue_expectations n > 4; ssme_lw_run_series, ssme_lw_get_expectations): a refused call between every
    pair of steps of a short series leaves the handle exactly what it was."""
    st, ref = _Steps(s), (LW_REFUSED if s["kind"] == "lw" else REFUSED)
    o = [("refused", ref[0])] + _start(s)
    for i in range(5):
        o += [st(1), ("refused", ref[i % len(ref)])]
    return o + [_ser(s, min(5, s["tmax"]), 0)] + [("refused", r) for r in ref] + [st(1)]


SCENARIOS = dict(H1=h1_graph_key, H2=h2_regrowth, H3=h3_covariates, H4=h4_gamma, H5=h5_parity, H6=h6_queued, H7=h7_theta_rows, H8=h8_refused)


def scenarios():
    """[(hazard, shape name, ops)] for every shape the hazard exists on."""
    out = []
    for h, fn in SCENARIOS.items():
        for s in SHAPES.values():
            ops = fn(s)
            if ops:
                out.append((h, s["name"], ops))
    return out


CHURN_SHAPES = ("small-100", "wl2-512", "lw-300-form0-rs1", "tiles5-2048")


def churn_plan(n=40, alive=3):
    """H9: [(shape name, seed, handles alive when this one is created)]: n handles of four shapes, `alive` at a time."""
    return [(CHURN_SHAPES[(i * 7 + i // 4) % 4], SEED + i % 5, min(i, alive - 1)) for i in range(n)]


# ---- seeded random walks ---------------------------------------------------------------------------------------------------------
def _instantiate(cls, m, rng):
    s = m.s
    Ts = [T for T in SERIES_T if T <= s["tmax"]]
    if cls.startswith("set_params_"):
        return ("set_params", cls[len("set_params_"):])
    if cls == "set_seed":
        return ("set_seed", 100 + rng.randrange(3))
    if cls in ("reset", "lw_reset"):
        return (cls,)
    if cls in ("series_z", "series_noz", "lw_series_z", "lw_series_noz"):
        T = rng.choice(Ts) if rng.random() < 0.5 else rng.choice(Ts[:4])
        return ("lw_series" if m.lw else "series", T, rng.randrange(3), cls.endswith("_z"))
    if cls in ("step", "step_queued"):
        return (cls, rng.choice((1, 2, 3)), m.n_steps, s["model"] == LEV and rng.random() < 0.7)
    if cls == "lw_filter":
        return (cls, rng.choice((1, 2, 3)), m.n_steps)
    if cls == "set_graph_mode":
        return (cls, not m.graph if rng.random() < 0.7 else m.graph)
    if cls == "set_small_series":
        return (cls, not m.small if rng.random() < 0.7 else m.small)
    if cls == "set_stream":
        return (cls, not m.stream)
    if cls == "set_tuning":
        return (cls, rng.choice(allowed_nt(s)))
    if cls == "set_debug":
        return (cls, rng.random() < 0.5, rng.random() < 0.5, rng.choice(allowed_splits(s)))
    if cls == "lw_set_debug":
        return (cls, rng.random() < 0.5, rng.choice((None, True)))
    raise ValueError(cls)


def _classes(s):
    if s["kind"] == "lw":
        return LW_CLASSES
    return tuple(c for c in BS_CLASSES if c != "series_z" or s["model"] == LEV)


def walk(s, seed, covered):
    """One walk of s["walk_ops"] ops.  covered: {(class, class): a reader stood between them at least once}, updated in place.  The
    next class is drawn from those the contract allows now (the model is asked), uncovered pairs first; the first instance of a pair,
    and one in three afterwards, gets a reader between the two."""
    rng = random.Random(f"{s['name']}/{seed}")
    m, ops, prev = HandleModel(s), [], None
    readers, refused = (LW_READERS, LW_REFUSED) if m.lw else (READERS, REFUSED)
    while len(ops) < s["walk_ops"]:
        cands = [c for c in _classes(s) if m.legal(_instantiate(c, m, random.Random(0)))]
        fresh = [c for c in cands if prev is not None and not covered.get((prev, c))]
        cls = rng.choice(fresh or cands)
        op = _instantiate(cls, m, rng)
        if not m.legal(op):
            continue
        if prev is not None:
            between = []
            if not covered.get((prev, cls)) or rng.random() < 0.34:
                rd = [r for r in readers if m.legal(("read", r))]
                between.append(("read", rng.choice(rd)))
            if rng.random() < 0.1:
                between.append(("refused", rng.choice(refused)))
            covered[(prev, cls)] = covered.get((prev, cls), False) or any(b[0] == "read" for b in between)
            ops += between
        ops.append(op)
        m.apply(op)
        prev = cls
    return ops


_WALKS = None


def walks(max_rounds=12):
    """[(shape name, seed, ops)] and the coverage map.  Rounds of one walk per shape (seeds 0, 1, ...) are added until every ordered
    pair of state-changing op classes stands adjacent in some walk of some shape with a reader between them -- bootstrap and
    Liu-West classes each among themselves -- and at least two rounds."""
    global _WALKS
    if _WALKS is None:
        cov = {"bs": {}, "lw": {}}
        out = []
        for seed in range(max_rounds):
            for s in SHAPES.values():
                out.append((s["name"], seed, walk(s, seed, cov[s["kind"]])))
            if seed >= 1 and not missing_pairs(cov):
                break
        _WALKS = (out, cov)
    return _WALKS


def missing_pairs(cov):
    need = [("bs", a, b) for a in BS_CLASSES for b in BS_CLASSES] + [("lw", a, b) for a in LW_CLASSES for b in LW_CLASSES]
    return [p for p in need if not cov[p[0]].get((p[1], p[2]))]


def all_runs():
    """Every op list that the GPU module runs: [(id, shape name, ops)]"""
    return [(f"{h}@{n}", n, ops) for h, n, ops in scenarios()] + [(f"walk{seed}@{n}", n, ops) for n, seed, ops in walks()[0]]


def trace(shape_name, ops):
    """[(op, events)] of a run through the model."""
    m = HandleModel(SHAPES[shape_name])
    return [(op, m.apply(op)) for op in ops]


def paths_report():
    """profiles/lifecycle_paths.txt: per scenario, the ops and the predicted replay / recapture / regrow / redraw events."""
    lines = ["# written by `python tests/lifecycle_cases.py`: the ops of every hand-written scenario and walk, and the events the host model",
             "# predicts for each (replay / recapture:<key fields that differ> / drop / regrow / alloc / redraw:<what emptied the chunk> / series:<form>:<parity>)"]
    for rid, name, ops in all_runs():
        tr = trace(name, ops)
        lines.append(f"\n{rid}  ({len(ops)} ops)")
        if rid.startswith("walk"):               # walks: the ops in one line each would fill the file; their events, counted
            count = {}
            for _, ev in tr:
                for e in ev:
                    e = e.split(":")[0] + (":" + e.split(":")[1] if e.startswith(("series", "redraw")) else "")
                    count[e] = count.get(e, 0) + 1
            lines.append("  classes: " + " ".join(HandleModel(SHAPES[name]).op_class(op) for op, _ in tr if op[0] not in ("read", "refused")))
            lines.append("  events:  " + " ".join(f"{k} x{v}" for k, v in sorted(count.items())))
            continue
        for i, (op, ev) in enumerate(tr):
            lines.append(f"  {i:3d} {' '.join(str(a) for a in op):44s} {' '.join(ev)}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    import sys
    sys.stdout.write(paths_report())
