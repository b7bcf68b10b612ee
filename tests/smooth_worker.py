"""Runs the smoothing calls on a library with a vector user model (SSME_PF_LIB) in a process of its own and pickles what
tests/test_smoothing_gpu.py and tests/test_smoothing_edges_gpu.py compare.  Modes (second argument; default "lineages"):
  lineages   tests/models/svol_two_factor.h (dim_x = dim_y = 2): for every shape the device's trajectories of all final particles (both
             state planes) with their lineage indices, and the host genealogy of a handle stepped with step() (tests/smooth_ref.py);
  smoothed   the same library: also smoothed_expectations, expectations_multi and the stepped handle's final states;
  dx3        tests/models/lin_gauss_3d.h (dim_x = 3, dim_y = 1): lineages, all three planes;
  user_h     tests/models/svol_two_factor_h.h (7 functionals of its own) on the tiled route: series_user_expectations with the history
             on and off, and the lineages of the recording run.
    python tests/smooth_worker.py OUT.pkl [MODE]"""
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
mode = sys.argv[2] if len(sys.argv) > 2 else "lineages"
T = 7
header = {"lineages": "svol_two_factor", "smoothed": "svol_two_factor", "dx3": "lin_gauss_3d", "user_h": "svol_two_factor"}[mode]
dx, dy = uc.HEADERS[header]["dx"], uc.HEADERS[header]["dy"]
th = np.asarray(uc.HEADERS[header]["theta"], dtype=np.float64)
y = np.stack([sc.spy()[100 * d:100 * d + T] for d in range(dy)], axis=1).copy()
if dy == 1:
    y = y[:, 0].copy()
assert sa.ParticleFilterBank(sc.MODEL_USER0, 8, 1)._dims() == (dx, dy)
SHAPES = (("lane-500", 500, 0, True), ("pair-1030", 1030, 0, True), ("tiled-1027-t512", 1027, 512, True))
res = {}


def lineages_of(bank, n):
    term = np.tile(np.arange(n, dtype=np.uint32), (bank.r, 1))
    return bank.sample_trajectories(n, terminal=term, indices=True)


if mode == "user_h":
    from ssme_amd import _capi
    assert _capi.lib().ssme_pf_user_model_n_h() == 7
    z = 0.37 + 0.5 * np.arange(T)
    name, n, tile, small = SHAPES[2]
    for sched in (1, 3):
        ref_bank = sc.make_bank(sa, sc.MODEL_USER0, n, th, 0, sched, tile)
        hist = sr.stepped_history(ref_bank, y, z)
        ref_bank.close()
        want_x, want_idx = sr.reference(hist, sched)
        got = {}
        for on in (False, True):
            bank = sc.make_bank(sa, sc.MODEL_USER0, n, th, 0, sched, tile)
            bank.set_small_series(small)
            bank.record_series_expectations(sc.ALL4, True)
            bank.record_series_history(on)
            got["ll_on" if on else "ll_off"] = bank.run_series(y, z)
            got["on" if on else "off"] = bank.series_user_expectations()
            if on:
                got["route"] = bank.series_route()
                got["x"], got["idx"] = lineages_of(bank, n)
            bank.close()
        res[f"{name}-sched{sched}"] = dict(got, want_x=want_x, want_idx=want_idx)
else:
    for name, n, tile, small in SHAPES:
        for sched in (1, 3):
            ref_bank = sc.make_bank(sa, sc.MODEL_USER0, n, th, 0, sched, tile)
            hist = sr.stepped_history(ref_bank, y)
            ref_bank.close()
            want_x, want_idx = sr.reference(hist, sched)
            bank = sc.make_bank(sa, sc.MODEL_USER0, n, th, 0, sched, tile)
            bank.set_small_series(small)
            bank.record_series_history()
            ll = bank.run_series(y)
            x, idx = lineages_of(bank, n)
            r = dict(route=bank.series_route(), want_route=sc.expected_route(n, tile, small), ll=ll, x=x, idx=idx, want_x=want_x,
                     want_idx=want_idx, bytes=bank.series_history_bytes(T), npad=bank.tile * bank.n_tiles)
            if mode == "smoothed":
                r.update(sm=bank.smoothed_expectations(sc.ALL4), em=bank.expectations_multi(sc.ALL4), final=hist["final"], n=n, tile=bank.tile,
                         n_tiles=bank.n_tiles)
            res[f"{name}-sched{sched}"] = r
            bank.close()
with open(out, "wb") as f:
    pickle.dump(res, f)
