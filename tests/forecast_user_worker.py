"""Runs the user-model library (SSME_PF_LIB: tests/models/svol_student_t.h compiled in) in its own process -- a process binds ONE
libssme_pf.so -- and writes the two status codes tests/test_forecast_gpu.py expects: ssme_pf_sim_future_obs on a SSME_MODEL_USER0
handle (user models declare no observation draw) and on a built-in model's handle of the same library.
    python tests/forecast_user_worker.py OUT.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssme_amd  # noqa: E402
from ssme_amd import _capi  # noqa: E402

L = _capi.lib()
assert L.ssme_pf_user_model_n_theta() == 4
codes = []
for model, th in ((ssme_amd.MODEL_USER0, [1.1, 0.95, 0.25, 7.0]), (ssme_amd.MODEL_SVOL, [1.1, 0.95, 0.25])):
    bank = ssme_amd.ParticleFilterBank(model, 300, 1, 3)
    bank.set_params(th)
    bank.step(0.01)
    y = np.empty((1, 2, 300))
    codes.append(L.ssme_pf_sim_future_obs(bank._h, 2, None, _capi.dptr(y), None, None))
    bank.close()
with open(sys.argv[1], "w") as f:
    f.write(" ".join(str(c) for c in codes))
