"""A recorded Liu-West series (ssme_lw_set_series_expectations / ssme_lw_get_series_expectations) against the step API, bit for bit.

Three handles per case, same configuration and seed:
  A  run_series on the series route (set_small_series(1); k_lw_series' recording instantiation where N <= 2048), recording
  B  run_series on the tiled route (set_small_series(0); k_lw_param_partials + k_lw_param_means queued behind every step), recording
  C  stepped with filter(), expectations(range(8)) and param_means() read after every step
Rows of A == rows of B == read-outs of C: all T x 8 x R values, every bit, NaN for NaN.  Then: recording changes nothing else that
any call returns, the life cycle of the switch and the buffer, a longer series and a bank.
The case list is tests/lw_series_expect_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import lw_edge_cases as lc
import lw_series_expect_cases as xc
import test_expectations_gpu as teg
from test_liu_west_edges_gpu import same_bits

pytestmark = pytest.mark.gpu
sa = teg.sa
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = list(range(xc.N_VALUES))


def make(sa, oracle, case, series, record, n=None, R=None, first=0):
    tr, lo, hi = lc.prior(case, oracle)
    cls = sa.svol_lw_2_par if case["form"] else sa.svol_lw_1_par
    g = cls(case["delta"], lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], nparts=case["n"] if n is None else n,
            n_filters=case["R"] if R is None else R, seed=lc.SEED, transforms=tuple(tr), rs=case["rs"], first_filter_id=first)
    g.set_debug(True)
    g.set_small_series(series)
    if record:
        g.record_series_expectations(True)
    return g


def stepped(g, y, z):
    """([T, 8, R] expectations(range(8)), [T, R, 4] param_means()) read after every filter() call."""
    rows, means = [], []
    for k in range(len(y)):
        g.filter(y[k], z[k])
        rows.append(g.expectations(IDS))
        means.append(g.param_means())
    return np.array(rows), np.array(means)


def expected_route(sa, n):
    """What lw_series_route decides for a recording handle with small series enabled: the whole-series kernel keeps one-tile
    filters (profiles/lw_series_expectations_timing.txt)."""
    return sa.ROUTE_LW_SERIES if n <= lc.TILE else sa.ROUTE_TILED


def three_handles(sa, oracle, case, y=None, z=None):
    if y is None:
        y, z = lc.series(case)
    T, R = len(y), case["R"]
    a, b, c = make(sa, oracle, case, True, True), make(sa, oracle, case, False, True), make(sa, oracle, case, True, False)
    assert a.series_route() == (expected_route(sa, case["n"]), 512)
    assert b.series_route() == (sa.ROUTE_TILED, 512)
    a.run_series(y, z)
    b.run_series(y, z)
    ra, rb = a.series_expectations(), b.series_expectations()
    want, want_means = stepped(c, y, z)
    assert ra.shape == rb.shape == want.shape == (T, xc.N_VALUES, R)
    same_bits(ra, rb, case["name"] + ": rows of the series route == rows of the tiled route")
    same_bits(ra, want, case["name"] + ": rows == expectations(range(8)) after every step")
    same_bits(a.series_param_means(), want_means, case["name"] + ": series_param_means() == param_means() after every step")
    same_bits(b.series_param_means(), want_means, case["name"] + ": series_param_means() of the tiled route")
    same_bits(ra[-1], a.expectations(IDS), case["name"] + ": the last row == expectations() after the series")
    for g in (a, b, c):
        g.close()
    return ra


@pytest.mark.parametrize("case", xc.size_cases(), ids=lambda c: c["name"])
def test_sizes(sa, oracle, case):
    rows = three_handles(sa, oracle, case)
    assert not np.isnan(rows).any()
    same_bits(rows[:, 3], np.full((case["T"], 1), 42.0), case["name"] + ": E[42]")


@pytest.mark.parametrize("case", xc.schedule_cases(), ids=lambda c: c["name"])
def test_schedules(sa, oracle, case):
    three_handles(sa, oracle, case)


@pytest.mark.parametrize("case", xc.degenerate_cases(), ids=lambda c: c["name"])
def test_degenerate_inputs(sa, oracle, case):
    rows = three_handles(sa, oracle, case)
    if case["base"] == "nan-y-R3":
        # y[2] = NaN reaches every filter's weights at step 2 and no other step: the draw that follows starts from log-weights 0 again
        nan = np.isnan(rows)
        assert nan[xc.NAN_Y_STEP].all(), rows[xc.NAN_Y_STEP]
        assert not np.delete(nan, xc.NAN_Y_STEP, axis=0).any()


@pytest.mark.parametrize("case", xc.tiled_only_cases(), ids=lambda c: c["name"])
def test_more_than_one_tile(sa, oracle, case):
    three_handles(sa, oracle, case)


def _same_state(a, b, R, T, what):
    same_bits(a.per_step(), b.per_step(), what + ": per_step()")
    same_bits(a.expectations(IDS), b.expectations(IDS), what + ": expectations()")
    same_bits(a.param_means(), b.param_means(), what + ": param_means()")
    for r in range(R):
        u, v = a.state(r, indices=True), b.state(r, indices=True)
        for k in ("x", "theta", "thetabar", "L"):
            same_bits(u[k], v[k], f"{what} r={r}: {k}")
        for k in ("anc", "kidx"):
            np.testing.assert_array_equal(u[k], v[k], err_msg=f"{what} r={r}: {k}")
        for p, q, k in zip(a.weights(r), b.weights(r), ("x", "untransformed theta", "w")):
            same_bits(p, q, f"{what} r={r}: weights() {k}")


@pytest.mark.parametrize("series", (True, False), ids=("series-route", "tiled-route"))
@pytest.mark.parametrize("case", xc.invisible_cases(), ids=lambda c: c["name"])
def test_recording_is_invisible(sa, oracle, case, series):
    """A recording run_series against a non-recording one on a fresh handle with the same seed."""
    y, z = lc.series(case)
    rec, plain = make(sa, oracle, case, series, True), make(sa, oracle, case, series, False)
    what = case["name"]
    same_bits(rec.run_series(y[:5], z[:5]), plain.run_series(y[:5], z[:5]), what + ": the returned sums")
    _same_state(rec, plain, case["R"], 5, what)
    rows = rec.series_expectations()
    for k in range(5, 8):
        rec.filter(y[k], z[k])
        plain.filter(y[k], z[k])
        same_bits(np.atleast_1d(rec.getLogCondLike()), np.atleast_1d(plain.getLogCondLike()), f"{what} t={k}: getLogCondLike()")
        u, v = rec.state(0, indices=True), plain.state(0, indices=True)
        for key in ("x", "theta", "thetabar", "L"):
            same_bits(u[key], v[key], f"{what} t={k}: {key}")
        for key in ("anc", "kidx"):
            np.testing.assert_array_equal(u[key], v[key], err_msg=f"{what} t={k}: {key}")
        same_bits(rec.expectations(IDS), plain.expectations(IDS), f"{what} t={k}: expectations()")
    same_bits(rec.series_expectations(), rows, what + ": the recorded rows after three filter() calls")
    fa = rec.sim_future_obs(4, y[7], states=True, start=True, prop=True)
    fb = plain.sim_future_obs(4, y[7], states=True, start=True, prop=True)
    same_bits(fa[0], fb[0], what + ": forecast observations")
    same_bits(fa[1], fb[1], what + ": forecast states")
    np.testing.assert_array_equal(fa[2], fb[2], err_msg=what + ": start draw")
    same_bits(fa[3][:, :14], fb[3][:, :14], what + ": forecast proposal")
    rec.close()
    plain.close()


def _get_status(sa, g, T, n=8):
    from ssme_amd import _capi
    ids = np.arange(n, dtype=np.int32)
    out = np.full((max(T, 1), n, g.r), -1.0)
    rc = _capi.lib().ssme_lw_get_series_expectations(g._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), n, _capi.dptr(out), T)
    return rc, out


@pytest.mark.parametrize("series", (True, False), ids=("series-route", "tiled-route"))
@pytest.mark.parametrize("form", (0, 1))
def test_life_cycle(sa, oracle, form, series):
    from ssme_amd import _capi
    case = lc._c("rec-life", n=300, T=6, form=form)
    y, z = lc.series(case)
    g = make(sa, oracle, case, series, False)
    assert _get_status(sa, g, 1)[0] == _capi.ERR_STATE                      # before any series
    with pytest.raises(_capi.SsmeError) as e:
        g.series_expectations()
    assert e.value.status == _capi.ERR_STATE
    g.run_series(y, z)
    assert _get_status(sa, g, 1)[0] == _capi.ERR_STATE                      # after a non-recording series
    g.record_series_expectations(True)
    assert _get_status(sa, g, 1)[0] == _capi.ERR_STATE                      # the switch alone records nothing
    g.reset()                                                               # the setting survives reset
    assert g.series_route() == ((expected_route(sa, case["n"]) if series else sa.ROUTE_TILED), 512)
    g.run_series(y, z)
    rows6 = g.series_expectations()
    fresh = make(sa, oracle, case, series, True)
    fresh.run_series(y, z)
    same_bits(rows6, fresh.series_expectations(), "recording switched on later == a handle that recorded from the start")
    rc, part = _get_status(sa, g, 3)                                        # fewer rows than recorded: the first three
    assert rc == _capi.OK
    same_bits(part, rows6[:3], "the first three rows")
    assert _get_status(sa, g, 7)[0] == _capi.ERR_INVALID_ARG                # T beyond the recorded series
    # a second recording series of another T returns the rows of the second series
    g.run_series(y[:4], z[:4])
    fresh.close()
    fresh = make(sa, oracle, case, series, True)
    fresh.run_series(y[:4], z[:4])
    rows4 = g.series_expectations()
    assert rows4.shape == (4, 8, 1)
    same_bits(rows4, fresh.series_expectations(), "second series of another T")
    same_bits(rows4, rows6[:4], "the same first four steps")
    assert _get_status(sa, g, 5)[0] == _capi.ERR_INVALID_ARG                # the buffer holds 6 rows, the last series recorded 4
    # filter() neither records nor clears
    g.filter(y[4], z[4])
    same_bits(g.series_expectations(), rows4, "the recorded rows after filter()")
    assert _get_status(sa, g, 5)[0] == _capi.ERR_INVALID_ARG
    # switching off and running again: nothing recorded
    g.record_series_expectations(False)
    rc, part = _get_status(sa, g, 4)
    assert rc == _capi.OK                                                   # the rows stay until the next run_series
    same_bits(part, rows4, "rows after switching off, before the next series")
    g.run_series(y, z)
    assert _get_status(sa, g, 1)[0] == _capi.ERR_STATE
    # refusals on a live handle
    assert _capi.lib().ssme_lw_set_series_expectations(g._h, 2) == _capi.ERR_INVALID_ARG
    assert _capi.lib().ssme_lw_set_series_expectations(g._h, -1) == _capi.ERR_INVALID_ARG
    g.record_series_expectations(True)
    g.run_series(y, z)
    ids = np.arange(8, dtype=np.int32)
    ip, out = ids.ctypes.data_as(C.POINTER(C.c_int32)), np.empty((6, 8, 1))
    L = _capi.lib()
    assert L.ssme_lw_get_series_expectations(g._h, ip, 8, None, 6) == _capi.ERR_INVALID_ARG
    assert L.ssme_lw_get_series_expectations(g._h, None, 8, _capi.dptr(out), 6) == _capi.ERR_INVALID_ARG
    assert L.ssme_lw_get_series_expectations(g._h, ip, 0, _capi.dptr(out), 6) == _capi.ERR_INVALID_ARG
    assert L.ssme_lw_get_series_expectations(g._h, ip, 9, _capi.dptr(out), 6) == _capi.ERR_INVALID_ARG
    assert L.ssme_lw_get_series_expectations(g._h, ip, 8, _capi.dptr(out), 0) == _capi.ERR_INVALID_ARG
    bad = np.array([0, 8], dtype=np.int32)
    assert L.ssme_lw_get_series_expectations(g._h, bad.ctypes.data_as(C.POINTER(C.c_int32)), 2, _capi.dptr(out), 6) == _capi.ERR_INVALID_ARG
    bad[1] = -1
    assert L.ssme_lw_get_series_expectations(g._h, bad.ctypes.data_as(C.POINTER(C.c_int32)), 2, _capi.dptr(out), 6) == _capi.ERR_INVALID_ARG
    same_bits(g.series_expectations(), rows6, "recording again after a non-recording series")
    # a permuted list with a repeat: chosen at read time
    same_bits(g.series_expectations((7, 0, 7, 3)), rows6[:, (7, 0, 7, 3)], "a permuted id list")
    g.close()
    fresh.close()


@pytest.mark.parametrize("form", (0, 1))
def test_route_of_a_recording_handle(sa, oracle, form):
    case = lc._c("rec-route", n=lc.TILE, T=2, form=form)
    g = make(sa, oracle, case, True, True)
    assert g.series_route() == (expected_route(sa, lc.TILE), 512)
    g.set_small_series(False)
    assert g.series_route() == (sa.ROUTE_TILED, 512)
    g.close()
    g = make(sa, oracle, case, True, True, n=lc.TILE + 1)
    assert g.series_route() == (sa.ROUTE_TILED, 512)
    g.close()


def _spy_rows(T):
    y = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))[:T]
    return y, np.concatenate([[0.0], y[:-1]])


@pytest.mark.parametrize("form", (0, 1))
def test_a_longer_series(sa, oracle, form):
    case = lc._c("rec-long", n=xc.LONG_N, T=xc.LONG_T, form=form)
    y, z = _spy_rows(xc.LONG_T)
    rows = three_handles(sa, oracle, case, y, z)
    assert not np.isnan(rows).any()


@pytest.mark.parametrize("form", (0, 1))
def test_a_bank(sa, oracle, form):
    case = lc._c("rec-bank", n=xc.BANK_N, T=xc.BANK_T, R=xc.BANK_R, form=form)
    y, z = _spy_rows(xc.BANK_T)
    a, b = make(sa, oracle, case, True, True), make(sa, oracle, case, False, True)
    a.run_series(y, z)
    b.run_series(y, z)
    rows = a.series_expectations()
    assert rows.shape == (xc.BANK_T, 8, xc.BANK_R)
    same_bits(rows, b.series_expectations(), "bank: rows of the series route == rows of the tiled route")
    means = a.series_param_means()
    for r in xc.BANK_STEPPED:
        c = make(sa, oracle, case, True, False, R=1, first=r)
        want, want_means = stepped(c, y, z)
        same_bits(rows[:, :, r:r + 1], want, f"bank: filter {r} == its stepped twin")
        same_bits(means[:, r:r + 1], want_means, f"bank: parameter means of filter {r}")
        c.close()
    assert len({rows[:, :, r].tobytes() for r in range(xc.BANK_R)}) == xc.BANK_R           # no filter wrote another's rows
    a.close()
    b.close()
