"""Runs a library whose user model declares functionals of its own (SSME_PF_LIB: a header of tests/series_expect_cases.USER_LIBS) in a
process of its own and pickles what tests/test_series_expectations_gpu.py compares: recorded trajectories (ssme_pf_set_series_expectations)
and, for each, what a fresh handle stepped with step() returns after every step.
    python tests/series_expect_worker.py LIB OUT.pkl"""
import ctypes as C
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssme_amd as sa  # noqa: E402
from ssme_amd import _capi  # noqa: E402
import series_expect_cases as sc  # noqa: E402
import user_edge_cases as uc  # noqa: E402

lib, out = sys.argv[1], sys.argv[2]
L = _capi.lib()
U = sc.MODEL_USER0
if lib == sc.NO_H_LIB["lib"]:
    # a user model WITHOUT functionals: user != 0 is unsupported on its own handles, and leaves the handle's setting alone
    assert L.ssme_pf_user_model_n_h() == 0
    bank = sc.make_bank(sa, U, 500, np.asarray(sc.NO_H_LIB["theta"], dtype=np.float64))
    ids = (C.c_int32 * 1)(2)
    st = {"user-with-n_h-0": L.ssme_pf_set_series_expectations(bank._h, ids, 1, 1),
          "user-only-with-n_h-0": L.ssme_pf_set_series_expectations(bank._h, None, 0, 1),
          "builtins-with-n_h-0": L.ssme_pf_set_series_expectations(bank._h, ids, 1, 0)}
    y = sc.spy()[:sc.USER_T].copy()
    bank.run_series(y)
    buf = np.zeros(sc.USER_T * 2)
    st["get-builtins"] = L.ssme_pf_get_series_expectations(bank._h, _capi.dptr(buf), sc.USER_T)
    st["get-user"] = L.ssme_pf_get_series_user_expectations(bank._h, _capi.dptr(buf), 1)
    bank.close()
    with open(out, "wb") as f:
        pickle.dump({"status": st}, f)
    sys.exit(0)
s = sc.USER_LIBS[lib]
assert L.ssme_pf_user_model_n_h() == s["n_h"]
th = np.asarray(s["theta"], dtype=np.float64)
res = {}

y, z = sc.user_series(lib)
for n in sc.USER_SIZES:
    for rs, sched in ((0, 1), (1, 3)):
        bank = sc.make_bank(sa, U, n, th, rs, sched)
        bank.record_series_expectations(sc.ALL4, True)
        route = bank.series_route()
        _, traj, utraj = sc.recorded(bank, y, z, sc.ALL4, True)
        bank.close()
        ref, uref = sc.stepped(sa, U, n, th, y, z, sc.ALL4, True, rs=rs, sched=sched)
        res[("rows", n, rs, sched)] = dict(route=route, traj=traj, utraj=utraj, ref=ref, uref=uref)
    bank = sc.make_bank(sa, U, n, th)
    res[("user-only", n)] = sc.recorded(bank, y, z, (), True)[2]
    bank.set_small_series(False)
    res[("tiled", n)] = sc.recorded(bank, y, z, (), True)[2]
    bank.close()

# graph replay on the tiled route: a second series of the same T with other observations and covariates, then one without covariates
n = 2049
y2, z2 = sc.user_series(lib, shift=40)
bank = sc.make_bank(sa, U, n, th)
_, _, first_u = sc.recorded(bank, y, z, sc.ALL4, True)
_, second_b, second_u = sc.recorded(bank, y2, z2, sc.ALL4, True)
_, _, noz_u = sc.recorded(bank, y2, None, sc.ALL4, True)
bank.close()
ref, uref = sc.stepped(sa, U, n, th, y2, z2, sc.ALL4, True)
_, uref_noz = sc.stepped(sa, U, n, th, y2, None, sc.ALL4, True)
res["replay"] = dict(first_u=first_u, second_b=second_b, second_u=second_u, noz_u=noz_u, ref=ref, uref=uref, uref_noz=uref_noz)

# a bad theta row between two healthy ones (user_edge_cases.HEADERS: derive() sets `bad`, log g = -inf, every weight zero)
if s["edge"]:
    rows = np.asarray((s["theta"][0], uc.HEADERS[s["edge"]]["bad"], s["theta"][1]), dtype=np.float64)
    for n in sc.BAD_ROW_SIZES:
        bank = sc.make_bank(sa, U, n, rows)
        _, traj, utraj = sc.recorded(bank, y, z, sc.ALL4, True)
        bank.close()
        ref, uref = sc.stepped(sa, U, n, rows, y, z, sc.ALL4, True)
        res[("bad-row", n)] = dict(traj=traj, utraj=utraj, ref=ref, uref=uref)

# statuses that need a user-model library
st = {}
sv = sc.make_bank(sa, sc.MODEL_SVOL, 500, sc.TH_SVOL3)
st["user-on-builtin-model"] = L.ssme_pf_set_series_expectations(sv._h, None, 0, 1)
sv.close()
bank = sc.make_bank(sa, U, 500, th)
bank.record_series_expectations((0,), False)
bank.run_series(y, z)
buf = np.zeros(sc.USER_T * s["n_h"] * len(th))
st["user-get-without-user"] = L.ssme_pf_get_series_user_expectations(bank._h, _capi.dptr(buf), 1)
bank.close()
res["status"] = st

with open(out, "wb") as f:
    pickle.dump(res, f)
