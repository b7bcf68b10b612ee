"""Whole-series parity at the shapes the project is measured at (-m gpu): the device against the oracle's stored records
(tests/golden/long_series_golden.npz, made by tests/golden/make_golden_long.py), every per-step log conditional likelihood bit for bit,
the sum, and the final state by SHA-256 and a strided sample -- series API, a second pass on the same handle (graph replay) and the
step API.  The shapes cheap enough for a live oracle (the one-launch small-series kernel and the small rows of tests/long_parity.py)
run against it over all 3084 steps."""
import importlib.util
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

IDS = ["G1", "G2", "G3", "G4", "G5", "G6", "G7", "L1", "L2", "L3"]
STEP_API_IDS = ["G1", "G3", "G5", "L2"]

_spec = importlib.util.spec_from_file_location("make_golden_long", os.path.join(ROOT, "tests", "golden", "make_golden_long.py"))
mgl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgl)                      # sample_index / evidence: one definition for the records and for this module


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None        # the in-tree HIP library is what runs
    return ssme_amd


@pytest.fixture(scope="module")
def records():
    with np.load(os.path.join(ROOT, "tests", "golden", "long_series_golden.npz")) as f:
        rec = {k: f[k] for k in f.files}
    assert list(rec["ids"]) == IDS
    return rec


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cfg(rec, rid):
    """A record's configuration as plain Python values."""
    return {k[len(rid) + 1:]: (v.item() if v.ndim == 0 else v) for k, v in rec.items() if k.startswith(rid + "_")}


def _series(spy, T):
    return spy[:T], np.concatenate([[0.0], spy[:-1]])[:T]


def _make(sa, c):
    """The device filter of a record, created with the record's stored tile."""
    if c["kind"] == "pf":
        b = sa.ParticleFilterBank(int(c["model"]), int(c["n"]), int(c["filters"]), int(c["seed"]), int(c["resampler"]), int(c["sched"]),
                                  tile=int(c["tile"]))
        assert b.tile == int(c["tile"])
        b.set_params(c["theta"])
        return b
    lo, hi = c["prior_lo"], c["prior_hi"]
    cls = sa.svol_lw_2_par if int(c["form"]) == 1 else sa.svol_lw_1_par
    return cls(float(c["delta"]), lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=int(c["n"]), seed=int(c["seed"]),
               rs=int(c["m_rs"]))


def assert_per_step(dev, ref, what):
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert dev.shape == ref.shape, f"{what}: {dev.shape} values against {ref.shape}"
    bad = _bits(dev) != _bits(ref)
    if bad.any():
        t = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {dev.size} per-step values differ, first at step {t}: device {dev[t]!r} vs record {ref[t]!r}")


def assert_state(c, st, what):
    """Final-state evidence: x and cdf (bootstrap) or x, theta and the parameter means (Liu-West)."""
    names = ("x", "cdf") if c["kind"] == "pf" else ("x", "theta")
    for name in names:
        a = np.ascontiguousarray(st[name], dtype=np.uint64 if name == "cdf" else np.float64)
        sha, smp = mgl.evidence(a)
        ref = c["sample_" + name]
        view = (lambda v: np.ascontiguousarray(v).view(np.uint64))
        bad = view(smp) != view(ref)
        if bad.any():                                              # the sample says where; the hash below would only say that
            k = tuple(int(i) for i in np.argwhere(bad)[0])
            idx = int(mgl.sample_index(a.shape[-1])[k[-1]])
            raise AssertionError(f"{what}: final {name} differs in {int(bad.sum())} of {bad.size} sampled values, first at particle {idx}"
                                 f"{' plane ' + str(k[0]) if len(k) > 1 else ''}: device {smp[k]!r} vs record {ref[k]!r}")
        assert sha == str(c["sha_" + name]), f"{what}: final {name}: the strided sample agrees but the SHA-256 of all {a.size} values differs"
    if c["kind"] == "lw":
        tb = np.asarray(st["thetabar"], dtype=np.float64)
        assert np.array_equal(_bits(tb), _bits(c["thetabar"])), f"{what}: theta-bar {tb!r} vs record {c['thetabar']!r}"


def _state(c, f):
    return f.state(0, logw=False) if c["kind"] == "pf" else f.state(0)


def _lw_loglik(f):
    from ssme_amd import _capi
    out = np.empty(f.r)
    _capi.check(_capi.lib().ssme_lw_get_loglik(f._h, _capi.dptr(out)), f._h, last_error=_capi.lib().ssme_lw_last_error)
    return out


@pytest.mark.parametrize("rid", IDS)
def test_series_api_matches_record(sa, records, spy, rid):
    """run_series over the record's T: every per-step value, the sum, the final state; then the same series again on the same handle
    (after set_seed / reset: the captured graph is replayed, not captured) must give the same bits."""
    c = _cfg(records, rid)
    T = int(c["T"])
    y, z = _series(spy, T)
    f = _make(sa, c)
    try:
        for run in ("first pass", "second pass on the same handle"):
            ll = f.run_series(y, None if c["kind"] == "pf" else z)[0]
            assert_per_step(f.per_step()[0], c["per"], f"{rid} series API, {run}")
            assert float(ll) == float(c["ll"]), f"{rid} series API, {run}: sum {float(ll)!r} vs record {float(c['ll'])!r}"
            assert_state(c, _state(c, f), f"{rid} series API, {run}")
            if c["kind"] == "pf":
                f.set_seed(int(c["seed"]))
            else:
                f.reset()
    finally:
        f.close()


@pytest.mark.parametrize("rid", STEP_API_IDS)
def test_step_api_matches_record(sa, records, spy, rid):
    """The same series one observation at a time (ssme_pf_step / ssme_lw_step: T host round trips, T hand-overs of the
    cross-workgroup ticket per workgroup): every return value, the accumulated sum and the final state."""
    c = _cfg(records, rid)
    T = int(c["T"])
    y, z = _series(spy, T)
    f = _make(sa, c)
    try:
        got = np.empty(T)
        if c["kind"] == "pf":
            for t in range(T):
                got[t] = f.step(y[t])[0]
            ll = f.loglik()[0]
        else:
            for t in range(T):
                f.filter(y[t], z[t])
                got[t] = f.getLogCondLike()
            ll = _lw_loglik(f)[0]
        assert_per_step(got, c["per"], f"{rid} step API")
        assert float(ll) == float(c["ll"]), f"{rid} step API: sum {float(ll)!r} vs record {float(c['ll'])!r}"
        assert_state(c, _state(c, f), f"{rid} step API")
    finally:
        f.close()


# (model, N, filters, resampler, schedule): the rows of tests/long_parity.py cheap enough for a live oracle -- the one-launch
# small-series kernel (N <= 2048; several filters, schedule 3, leverage with systematic resampling) and the 4 x 2^14 leverage bank
LIVE = [(0, 100, 3, 0, 1), (0, 500, 3, 0, 1), (1, 500, 2, 1, 1), (0, 2000, 2, 0, 1), (0, 500, 2, 0, 3), (1, 16384, 4, 0, 1)]
LIVE_THETA = {0: [1.0, 0.95, 0.25], 1: [0.9, 0.0, 1.0, -0.1]}


@pytest.mark.parametrize("model,n,r,rs,sched", LIVE)
def test_whole_series_against_live_oracle(sa, oracle, spy, model, n, r, rs, sched):
    """All 3084 steps, every filter of the bank against its own oracle filter (one per thread), per-step values, sums and final state."""
    seed, th = 4242, LIVE_THETA[model]
    y, z = _series(spy, spy.size)
    z = z if model == 1 else None
    b = sa.ParticleFilterBank(model, n, r, seed, rs, sched)
    try:
        b.set_params(th)
        ll = b.run_series(y, z)
        per = b.per_step()
        tile = b.tile

        def ref(rep):
            o = oracle.Filter(model, n, th, seed, rep=rep, resampler=rs, resamp_sched=sched, tile=tile)
            llo, po = o.run_series(y, z)
            return llo, po, o.state()

        with ThreadPoolExecutor(min(r, 16)) as ex:
            refs = list(ex.map(ref, range(r)))
        for k in range(r):
            what = f"model {model} N {n} schedule {sched} filter {k}"
            assert_per_step(per[k], refs[k][1], what)
            assert float(ll[k]) == float(refs[k][0]), f"{what}: sum {float(ll[k])!r} vs oracle {float(refs[k][0])!r}"
            st = b.state(k, logw=False)
            assert np.array_equal(_bits(st["x"]), _bits(refs[k][2]["x"])), f"{what}: final particles differ"
            assert np.array_equal(st["cdf"], refs[k][2]["cdf"]), f"{what}: final integer cdf differs"
    finally:
        b.close()
