"""Runs the library built with tests/models/lin_gauss_4d_h.h (dim_x = dim_y = 4, n_h = 16: the documented maxima) in its own process.
    python tests/user_4d_worker.py OUT.npz N TILE T NSEEDS
Reads y4.npy ([T_long, 4]) beside OUT: a debug run over its first T rows (state, ancestors, per-step values, the sixteen
expectations), then NSEEDS replicate filters over the whole series for the Kalman anchor."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ssme_amd  # noqa: E402
from ssme_amd import _capi  # noqa: E402

out, n, tile, T, nseeds = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
L = _capi.lib()
dx, dy = C.c_int32(), C.c_int32()
assert L.ssme_pf_user_model_dims(C.byref(dx), C.byref(dy)) == 0 and (dx.value, dy.value) == (4, 4)
assert L.ssme_pf_user_model_n_h() == 16 and L.ssme_pf_user_model_n_theta() == 6
y = np.load(os.path.join(os.path.dirname(out), "y4.npy"))
th = [0.9, 0.5, 0.7, 0.4, 1.1, 0.25]              # phi, sigma, tau_1..4
z = 0.5 + 0.25 * np.arange(T)
bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, n, 1, 5, 0, 1, tile=tile)
bank.set_debug(True, True)
bank.set_params(th)
ll = bank.run_series(y[:T], z)
st = bank.state(0, ancestors=True)
per = bank.per_step()
ue = bank.user_expectations()
bank.close()
bank = ssme_amd.ParticleFilterBank(ssme_amd.MODEL_USER0, n, nseeds, 6, 0, 1, tile=tile)
bank.set_params(th)
lls = bank.run_series(y)
bank.close()
np.savez(out, ll=ll, per=per, x=st["x"], logw=st["logw"], cdf=st["cdf"], anc=st["anc"], A=st["A"], mb=st["mb"], m=np.array([st["m"]]), ue=ue, lls=lls, z=z)
