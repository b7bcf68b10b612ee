"""Generates tests/golden/ref_thread_pool_lme.npz: log-mean-exp values computed BY THE REFERENCE's own thread_pool.h
(thread_pool<>::work, thread_pool.h:189-215,263-268) through oracle/_ref, so that the tests that pin the oracle's, the
host code's and the device's log-mean-exp against the reference run without the reference being present.

Contents:
    kat_want                the reference's own KAT input (10 000 values of 3.0, test_thread_pool.cpp:39-46)
    cases_n, cases_scale    the case grid of test_log_mean_exp_pinned_by_reference_thread_pool
    cases_v                 every case's input values, concatenated in grid order
    cases_want              the reference's log-mean-exp of each case
    bank_ll, bank_want      R = 16 SVOL filters (N = 3000, seed 8, theta (1, .95, .25), first 200 rows of spy_returns.csv,
                            kernel-matched oracle = the device's bits) and the reference's log-mean-exp of them
                            (test_device_log_mean_exp_against_reference_thread_pool)

Needs the reference's include/ssme/thread_pool.h; run from the repo root:
    python tests/golden/make_golden_ref_lme.py [REFERENCE_ROOT]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

NS = (1, 2, 7, 100, 1000)
SCALES = (1e-3, 1.0, 50.0, 700.0)
BANK = dict(n=3000, r=16, seed=8, theta=[1.0, 0.95, 0.25], T=200)


def main():
    if len(sys.argv) > 1:
        O.build_ref(sys.argv[1])
    O.build()
    if O.build_ref() is None:
        sys.exit("oracle/_ref could not be built: the reference's thread_pool.h is needed")
    out = {"kat_want": np.array([O.ref_log_mean_exp(np.full(10000, 3.0))])}
    rng = np.random.default_rng(5)
    ns, scales, vs, wants = [], [], [], []
    for n in NS:
        for scale in SCALES:
            v = -4700.0 + scale * rng.standard_normal(n)
            ns.append(n)
            scales.append(scale)
            vs.append(v)
            wants.append(O.ref_log_mean_exp(v))
    out.update(cases_n=np.array(ns, dtype=np.int64), cases_scale=np.array(scales), cases_v=np.concatenate(vs),
               cases_want=np.array(wants))
    y = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))[:BANK["T"]]
    tile = O.default_tile(BANK["n"], BANK["r"])
    ll = np.array([O.Filter(O.MODEL_SVOL, BANK["n"], BANK["theta"], BANK["seed"], rep=r, tile=tile).run_series(y)[0]
                   for r in range(BANK["r"])])
    out.update(bank_ll=ll, bank_want=np.array([O.ref_log_mean_exp(ll)]))
    path = os.path.join(ROOT, "tests", "golden", "ref_thread_pool_lme.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
