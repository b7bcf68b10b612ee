"""Runs marginal smoothing on a library with a user model that declares its transition density (SSME_PF_LIB) in a process of its own
and pickles the outcome for tests/test_marginal_gpu.py: the parity checks of tests/marginal_cases.py at N in {65, 513}, resamp_sched 1
and 3, every filter of a handle of two with different theta rows.
    python tests/marginal_worker.py OUT.pkl HEADER        HEADER: svol_student_t_f | svol_two_factor_f | svol_reg_cov_f
With HEADER = no_logf (a library whose header declares none): the status codes of the calls."""
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
from oracle import oracle as O  # noqa: E402
import backward_cases as bc  # noqa: E402
import backward_ref as br  # noqa: E402
import marginal_cases as mc  # noqa: E402
import series_expect_cases as sc  # noqa: E402
import user_cov_ref as ucr  # noqa: E402
import user_edge_cases as uc  # noqa: E402

out, header = sys.argv[1], sys.argv[2]
T = 6
res = {}
if header == "no_logf":
    assert not sa.filters.user_model_has_logf()
    th = np.asarray(uc.TH_ST, dtype=np.float64)
    y = sc.spy()[:T].copy()
    bank = bc.recorded(sa, sc.MODEL_USER0, th, 65, 0, True, 1, y, None)
    buf = np.zeros(bank.r * T)
    ids = (C.c_int32 * 1)(0)
    b = C.c_uint64()
    res["weights"] = _capi.lib().ssme_pf_download_smoothing_weights(bank._h, 0, 0, None, _capi.dptr(np.zeros(65)))
    res["means"] = _capi.lib().ssme_pf_get_marginal_smoothed_expectations(bank._h, ids, 1, _capi.dptr(buf), T)
    res["bytes"] = _capi.lib().ssme_pf_marginal_smoothing_bytes(bank._h, T, C.byref(b))
    res["genealogy"] = _capi.lib().ssme_pf_sample_trajectories(bank._h, 1, None, _capi.dptr(buf), None, T)
    res["unsupported"] = _capi.ERR_UNSUPPORTED
    bank.close()
else:
    assert sa.filters.user_model_has_logf()
    spec = {"svol_student_t_f": (uc.TH_ST, 1, 0, br.logf_student_t_f), "svol_two_factor_f": (uc.TH_2F, 2, 0, br.logf_two_factor_f),
            "svol_reg_cov_f": (uc.TH_REG, 1, 3, br.logf_reg_cov_f)}[header]
    th = np.asarray(spec[0], dtype=np.float64)
    dy, K, logf = spec[1], spec[2], spec[3]
    y = np.stack([sc.spy()[100 * d:100 * d + T] for d in range(dy)], axis=1).copy()
    if dy == 1:
        y = y[:, 0].copy()
    z = ucr.covariates(K, T) if K else None
    zs = None if z is None else [z[t] for t in range(T)]
    for n, tile, small in ((65, 0, True), (513, 0, True), (513, 512, True)):
        for sched in (1, 3):
            name = f"{header} N={n} tile={tile} sched={sched}"
            hist = bc.twin_history(sa, sc.MODEL_USER0, th, n, tile, sched, y, z)
            bank = bc.recorded(sa, sc.MODEL_USER0, th, n, tile, small, sched, y, z)
            degenerate, worst = mc.check_rows(O, bank, hist, lambda f: logf(O, th[f]), sched, name, zs=zs)
            mc.check_means(bank, T, name)
            x, w = bank.smoothing_weights(0, 0)
            res[name] = dict(route=bank.series_route(), degenerate=degenerate, worst=worst, dx=np.atleast_2d(x).shape[0],
                             carrying=int(np.count_nonzero(w > 0.0)))
            bank.close()
with open(out, "wb") as f:
    pickle.dump(res, f)
