"""Runs the smoothing calls on a library with a vector user model (SSME_PF_LIB: tests/models/svol_two_factor.h, dim_x = dim_y = 2) in a
process of its own and pickles what tests/test_smoothing_gpu.py compares: for every shape the device's trajectories of all final
particles (both state planes) with their lineage indices, and the host genealogy of a handle stepped with step() (tests/smooth_ref.py).
    python tests/smooth_worker.py OUT.pkl"""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssme_amd as sa  # noqa: E402
import series_expect_cases as sc  # noqa: E402
import smooth_ref as sr  # noqa: E402
import user_edge_cases as uc  # noqa: E402

out = sys.argv[1]
T = 7
th = np.asarray(uc.HEADERS["svol_two_factor"]["theta"], dtype=np.float64)
y = np.stack([sc.spy()[100 * d:100 * d + T] for d in range(2)], axis=1).copy()
assert sa.ParticleFilterBank(sc.MODEL_USER0, 8, 1)._dims() == (2, 2)
res = {}
for name, n, tile, small in (("lane-500", 500, 0, True), ("pair-1030", 1030, 0, True), ("tiled-1027-t512", 1027, 512, True)):
    for sched in (1, 3):
        ref_bank = sc.make_bank(sa, sc.MODEL_USER0, n, th, 0, sched, tile)
        hist = sr.stepped_history(ref_bank, y)
        ref_bank.close()
        want_x, want_idx = sr.reference(hist, sched)
        bank = sc.make_bank(sa, sc.MODEL_USER0, n, th, 0, sched, tile)
        bank.set_small_series(small)
        bank.record_series_history()
        ll = bank.run_series(y)
        term = np.tile(np.arange(n, dtype=np.uint32), (bank.r, 1))
        x, idx = bank.sample_trajectories(n, terminal=term, indices=True)
        res[f"{name}-sched{sched}"] = dict(route=bank.series_route(), want_route=sc.expected_route(n, tile, small), ll=ll,
                                           x=x, idx=idx, want_x=want_x, want_idx=want_idx, bytes=bank.series_history_bytes(T),
                                           npad=bank.tile * bank.n_tiles)
        bank.close()
with open(out, "wb") as f:
    pickle.dump(res, f)
