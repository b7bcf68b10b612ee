"""Generates tests/golden/long_series_golden.npz: whole-series records of the CPU oracle in kernel-matched (Philox) mode at the
shapes the project is measured at, which no pytest case can afford to recompute (about an hour of one CPU core in all).

Each record keeps its configuration, every per-step log conditional likelihood, their sum as the oracle accumulates it, and
evidence of the final state after step T: SHA-256 of the bytes of x and cdf (Liu-West: x and theta), a strided sample of 1024
values of each, and for Liu-West the parameter means.  Whole states are not stored.

Run from the repo root (records run in parallel processes, longest first; each prints its wall time):
    python tests/golden/make_golden_long.py [--jobs K] [--only G4,L3]
"""
import argparse
import hashlib
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor, as_completed

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "long_series_golden.npz")

SVOL_THETA = [1.0, 0.95, 0.25]
LW_LO, LW_HI = (0.8, -0.1, 0.01, -0.5), (0.99, 0.1, 0.1, -0.01)        # priors of tests/long_parity.py (phi, mu, sigma, rho)
N_SAMPLE = 1024

# id -> configuration.  kind "pf": oracle.Filter (model 0 = SVOL); kind "lw": oracle.LWFilter.  cost: rough core-minutes (ordering only).
RECORDS = {
    "G1": dict(kind="pf", n=1 << 20, seed=20260101, resampler=0, sched=1, tile=2048, T=3084, cost=9.0),     # the headline pass
    "G2": dict(kind="pf", n=1 << 20, seed=4242, resampler=1, sched=1, tile=2048, T=3084, cost=9.0),         # systematic, 512 tiles
    "G3": dict(kind="pf", n=1 << 18, seed=4242, resampler=0, sched=1, tile=None, T=3084, cost=2.0),         # default tile: 1024
    "G4": dict(kind="pf", n=300000, seed=4242, resampler=2, sched=1, tile=512, T=1000, cost=1.0),           # ragged N, small tiles
    "G5": dict(kind="pf", n=1 << 18, seed=4242, resampler=0, sched=3, tile=2048, T=3084, cost=2.0),         # carried log-weights
    "G6": dict(kind="pf", n=1 << 21, seed=4242, resampler=0, sched=1, tile=2048, T=1024, cost=6.0),         # 1024 tiles: split level-2
    "G7": dict(kind="pf", n=2200 * 2048 + 1, seed=4242, resampler=0, sched=1, tile=2048, T=512, cost=6.5),  # > 2048 tiles, ragged
    "L1": dict(kind="lw", n=1 << 20, seed=77, form=0, delta=0.99, m_rs=1, T=1024, cost=10.0),               # Liu-West benchmark shape
    "L2": dict(kind="lw", n=1 << 18, seed=77, form=1, delta=0.99, m_rs=2, T=3084, cost=7.5),                # SISR form with a schedule
    "L3": dict(kind="lw", n=1300 * 2048 + 11, seed=77, form=0, delta=0.95, m_rs=1, T=256, cost=6.5),        # split level-2, ragged
}

# Sums recorded by GPU builds of earlier rounds (profiles/r03_full_pass_vs_oracle.txt, profiles/r03_long_parity.txt).  A generated sum
# that differs means the arithmetic specification moved since: find the commit, do not accept the new value.
CROSS_CHECK = {"G1": -4097.376005593798, "G3": -4097.165936157169, "G4": -1685.9138876866527}


def sample_index(n):
    """The strided sample: N_SAMPLE indices spread evenly over [0, n)."""
    return (np.arange(N_SAMPLE, dtype=np.int64) * int(n)) // N_SAMPLE


def evidence(a):
    """(SHA-256 hex digest of the array's bytes in C order, strided sample along the last axis)."""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest(), np.ascontiguousarray(a[..., sample_index(a.shape[-1])])


def series():
    y = np.loadtxt(os.path.join(ROOT, "tests", "golden", "spy_returns.csv"))
    return y, np.concatenate([[0.0], y[:-1]])


def make_filter(cfg):
    """The oracle object of a record's configuration (cfg: RECORDS entry, or the same keys read back from the .npz)."""
    from oracle import oracle as O
    if cfg["kind"] == "pf":
        return O.Filter(O.MODEL_SVOL, int(cfg["n"]), cfg.get("theta", SVOL_THETA), int(cfg["seed"]), resampler=int(cfg["resampler"]),
                        resamp_sched=int(cfg["sched"]), tile=None if cfg["tile"] is None else int(cfg["tile"]))
    return O.LWFilter(int(cfg["n"]), int(cfg["seed"]), delta=float(cfg["delta"]), lo=cfg.get("prior_lo", LW_LO), hi=cfg.get("prior_hi", LW_HI),
                      form=int(cfg["form"]), resamp_sched=int(cfg["m_rs"]))


def run_oracle(cfg, T):
    """(filter, sum, per-step) of the oracle over the first T observations."""
    y, z = series()
    f = make_filter(cfg)
    if cfg["kind"] == "pf":
        ll, per = f.run_series(y[:T])
    else:
        per = np.array([f.step(y[t], z[t]) for t in range(T)])
        ll = f.loglik
    return f, float(ll), per


def make_record(rid):
    cfg = RECORDS[rid]
    t0 = time.time()
    f, ll, per = run_oracle(cfg, cfg["T"])
    st = f.state()
    out = {"kind": np.array(cfg["kind"]), "n": np.array(cfg["n"], dtype=np.int64), "filters": np.array(1, dtype=np.int64),
           "seed": np.array(cfg["seed"], dtype=np.uint64), "T": np.array(cfg["T"], dtype=np.int64), "per": per, "ll": np.array(ll)}
    if cfg["kind"] == "pf":
        out.update(model=np.array(0, dtype=np.int64), theta=np.array(SVOL_THETA), resampler=np.array(cfg["resampler"], dtype=np.int64),
                   sched=np.array(cfg["sched"], dtype=np.int64), tile=np.array(f.tile, dtype=np.int64))
        names = ("x", "cdf")
    else:
        out.update(model=np.array(1, dtype=np.int64), delta=np.array(cfg["delta"]), form=np.array(cfg["form"], dtype=np.int64),
                   m_rs=np.array(cfg["m_rs"], dtype=np.int64), tile=np.array(2048, dtype=np.int64),
                   prior_lo=np.array(LW_LO), prior_hi=np.array(LW_HI), thetabar=st["thetabar"])
        names = ("x", "theta")
    for name in names:
        sha, smp = evidence(st[name])
        out["sha_" + name] = np.array(sha)
        out["sample_" + name] = smp
    return rid, {f"{rid}_{k}": v for k, v in out.items()}, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", default="", help="comma-separated record ids: regenerate these, keep the others from the existing file")
    a = ap.parse_args()
    from oracle import oracle as O
    O.build()                                            # once, before the workers race for it
    ids = [s for s in a.only.split(",") if s] or list(RECORDS)
    done = {}
    t0 = time.time()
    with ProcessPoolExecutor(a.jobs) as ex:
        futs = [ex.submit(make_record, rid) for rid in sorted(ids, key=lambda r: -RECORDS[r]["cost"])]
        for fu in as_completed(futs):
            rid, rec, dt = fu.result()
            done[rid] = rec
            print(f"{rid}: sum {float(rec[rid + '_ll'])!r}  [{dt:.0f} s]", flush=True)
    bad = [r for r in ids if r in CROSS_CHECK and float(done[r][r + "_ll"]) != CROSS_CHECK[r]]
    out = {}
    if a.only and os.path.exists(OUT):
        with np.load(OUT) as old:
            out.update({k: old[k] for k in old.files})
    for rid in RECORDS:                                  # fixed order, whichever record finished first
        if rid in done:
            out.update(done[rid])
    out["ids"] = np.array([r for r in RECORDS if r + "_ll" in out])
    np.savez_compressed(OUT, **out)
    print(f"wrote {len(out)} arrays, {os.path.getsize(OUT)} bytes  [{time.time() - t0:.0f} s]")
    if bad:
        sys.exit(f"cross-check FAILED for {bad}: sums differ from the recorded device values in profiles/")
    print("cross-check sums equal the recorded device values:", [r for r in ids if r in CROSS_CHECK])


if __name__ == "__main__":
    main()
