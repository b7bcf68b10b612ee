"""The cases of tests/smooth_kernel_cases.py are what they claim, shown without a device: every shape edge the smoothing kernels branch
on is present, the out-of-range ancestors sit on paths that are read, the poisoned rows are unread under the reference, the
coalescing cases coalesce, the exactness premise of the integer check holds, and the numpy reference reproduces a lineage table
written out by hand."""
import numpy as np

import smooth_kernel_cases as kc
import smooth_ref as sr


def test_every_shape_edge_is_present():
    cs = kc.cases()
    assert 40 <= len(cs) <= 70
    for tile in kc.TILES:
        mine = [c for c in cs if c["tile"] == tile]
        assert {c["N"] for c in mine} >= set(kc.shape_ns(tile)), tile
        assert any(c["Bs"] > c["B"] for c in mine) and any(c["Bs"] > kc.lib_bs(c["B"]) for c in mine), tile
        assert {c["R"] for c in mine} >= {1, 3}, tile
        assert {c["states"] for c in mine if c["B"] == 3} >= {"code", "dyadic", "normal"}, tile
        assert {c["gen"] for c in mine} >= set(kc.GENEALOGIES), tile
        assert any(c["oor"] for c in mine) and any(c["dead"] for c in mine), tile
        assert {c["tmax"] for c in mine} >= {"equal", "spread", "zero-tile", "nan"}, tile
    assert {c["T"] for c in cs} >= {1, 2, 7, 33}
    assert {c["dx"] for c in cs} == {1, 2, 3, 4}
    assert {c["dx"] for c in cs if c["states"] == "code" and c["B"] > 1 and c["R"] > 1} >= {2, 3, 4}     # every plane stride, decodable
    assert any(c["dx"] > 1 and c["B"] == 3 for c in cs if c["states"] in ("dyadic", "code"))       # the sweep's dx stride, several tiles
    for s in ("1", "2", "3", "T", "T+1"):
        assert any(c["sched"] == {"1": 1, "2": 2, "3": 3, "T": c["T"], "T+1": c["T"] + 1}[s] and c["T"] > 1 for c in cs), s
    ks = {("N" if c["K"] == c["N"] else c["K"]) for c in cs}
    assert ks >= {1, 255, 1023, 1024, 1025, "N"}
    assert any(c["K"] == c["N"] and c["N"] > 1024 for c in cs)                   # a second grid block of k_sm_trajectories
    assert any(np.isnan(list(c["dead"].values())).any() for c in cs if c["dead"])
    assert any(0.0 in c["dead"].values() for c in cs)
    for c in cs:
        if c["tmax"] == "zero-tile":      # tile 0 has weight, and its scale is exactly zero
            assert (c["tsum"][:, 0] > 0).all() and (np.exp(c["mb"][:, 0] - c["mb"].max(axis=1)) == 0.0).all() and c["B"] >= 2
        if c["tmax"] == "nan":
            assert np.isnan(c["mb"][c["R"] - 1]).any() and np.isfinite(c["mb"][:c["R"] - 1]).all() and c["R"] > 1
        assert c["B"] == kc.n_tiles(c["N"], c["tile"]) and c["npad"] == c["B"] * c["tile"] and c["Bs"] >= c["B"]
        assert 0 < len(c["dead"]) < c["R"] or not c["dead"]                       # a dead filter always has live neighbours
        assert (c["q"] >= 0).all() and (c["q"] < 1 << 16).all() and (c["term"] < c["N"]).all()


def test_state_codes_decode():
    for c in kc.cases():
        if c["states"] != "code":
            continue
        T, dx, R, N = c["x"].shape
        for t, d, r, j in ((0, 0, 0, 0), (T - 1, dx - 1, R - 1, N - 1), (T // 2, dx - 1, 0, N // 2)):
            assert kc.decode(c["x"][t, d, r, j], dx, R, c["npad"]) == (t, d, r, j), c["name"]
        assert len(np.unique(c["x"])) == c["x"].size, c["name"]
        assert np.abs(c["x"]).max() < 8.0                                          # exp(x / 2) stays finite


def test_out_of_range_entries_are_on_paths_that_are_read():
    seen = set()
    for c in kc.cases():
        if not c["oor"]:
            assert (c["anc"] < c["N"]).all() and (c["anc"] >= 0).all(), c["name"]
            continue
        hit_sweep = hit_traj = 0
        for t in range(1, c["T"]):
            if not sr.resampled(t, c["sched"]):
                continue
            for r in range(c["R"]):
                bad = np.flatnonzero(c["anc"][t, r] >= c["N"])
                seen.update(int(v) if v < c["N"] + 1 or v == kc.U32MAX else "npad-1" for v in c["anc"][t, r, bad])
                hit_sweep += np.isin(c["B_ref"][r, t], bad).sum()
                hit_traj += np.isin(c["idx_ref"][r, :, t], bad).sum()
        assert hit_sweep > 0 and hit_traj > 0, c["name"]
        assert (c["B_ref"] < c["N"]).all() and (c["idx_ref"] < c["N"]).all()
        assert (c["B_ref"] == c["N"] - 1).any(), c["name"]                         # clamped, as the header says
    assert kc.U32MAX in seen and "npad-1" in seen and len(seen) >= 3


def test_poisoned_rows_are_unread_under_the_reference():
    """Replacing every row sm_resampled calls unread by garbage leaves the reference unchanged; a case's two variants differ exactly
    in the places no kernel may look at."""
    for c in kc.cases():
        rows = kc.unread_rows(c)
        assert 0 in rows
        d = dict(c)
        d["anc"] = c["anc"].copy()
        d["anc"][rows] = kc.U32MAX
        ref = kc.reference(d)
        for k in ("B_ref", "idx_ref", "xg"):
            np.testing.assert_array_equal(ref[k], c[k], err_msg=c["name"])
        a, b = kc.variant(c, True), kc.variant(c, False)
        N = c["N"]
        for k in ("hx", "cdf", "xg"):
            np.testing.assert_array_equal(a[k][..., :N], b[k][..., :N])
            assert np.isnan(a[k][..., N:]).all() and (b[k][..., N:] == 0).all()
        read = [t for t in range(c["T"]) if t not in rows]
        np.testing.assert_array_equal(a["hanc"][read][..., :N], b["hanc"][read][..., :N])
        assert (a["hanc"][rows] == kc.U32MAX).all() and (b["hanc"][rows] == 0).all()
        assert (a["hanc"][..., N:] == kc.U32MAX).all() and (b["hanc"][..., N:] == 0).all()
        assert np.isnan(a["tmax"][:, c["B"]:]).all() and np.isnan(a["tsum"][:, c["B"]:]).all()


def test_coalescing_cases_coalesce():
    n = 0
    for c in kc.cases():
        if c["gen"] != "coalesce" or c["coalesce_at"] == 0:
            continue
        n += 1
        for r in range(c["R"]):
            assert len(np.unique(c["B_ref"][r, 0])) == 1, c["name"]
            assert len(np.unique(c["B_ref"][r, c["T"] - 1])) == c["N"]
            if c["coalesce_at"] > 1 and c["sched"] == 1:
                assert len(np.unique(c["B_ref"][r, c["coalesce_at"]])) > 1, c["name"]
    assert n >= 3


def test_exactness_premise_of_the_integer_check():
    n = 0
    for c in kc.cases():
        if c["states"] != "dyadic":
            continue
        n += 1
        assert kc.exactness_margin(c) < 2 ** 53, c["name"]
        assert np.abs(c["x"]).max() <= 16.0 and np.array_equal(np.rint(c["x"] * 4), c["x"] * 4), c["name"]
        p = kc.exact_parts(c)
        cols = [i for i, f in enumerate(c["fids"]) if f != 2]
        assert cols and np.isfinite(p[..., cols]).all()
        # the same numbers by a float sum in another order: exact either way
        t, r = c["T"] - 1, c["R"] - 1
        sl = slice(0, min(c["N"], c["tile"]))
        assert p[t, r, 0, 0] == float(np.sum((c["xg"][t, r, sl] * c["q"][r, sl])[::-1]))
    assert n >= 9


def test_hand_written_lineage():
    """N = 5, T = 4, resamp_sched = 2: only step 2 resamples; rows 1 and 3 hold values that must not be read; entry 4 of row 2 is 7,
    out of range, and is clamped to 4."""
    c = dict(N=5, R=1, T=4, sched=2, K=5, dx=1, anc=kc.HAND_ANC.astype(np.int64), term=np.arange(5, dtype=np.uint32)[None, :],
             x=(10.0 * np.arange(4)[:, None] + np.arange(5)[None, :]).reshape(4, 1, 1, 5), S=np.array([1.0]))
    ref = kc.reference(c)
    np.testing.assert_array_equal(ref["B_ref"][0], kc.HAND_B)
    np.testing.assert_array_equal(ref["idx_ref"][0], kc.HAND_B.T)
    np.testing.assert_array_equal(ref["x_ref"][0, :, :, 0], [[3, 13, 20, 30], [3, 13, 21, 31], [0, 10, 22, 32], [1, 11, 23, 33], [4, 14, 24, 34]])
    np.testing.assert_array_equal(ref["xg"][:, 0, :], ref["x_ref"][0, :, :, 0].T)
    c["S"] = np.array([0.0])
    dead = kc.reference(c)
    assert np.isnan(dead["x_ref"]).all()
    np.testing.assert_array_equal(dead["idx_ref"], ref["idx_ref"])


def test_file_round_trip(tmp_path):
    """write_cases' layout is the one the program documents: header, sizes and order."""
    import struct
    cs = kc.cases()[:2]
    p = str(tmp_path / "cases.bin")
    kc.write_cases(p, cs)
    raw = open(p, "rb").read()
    assert raw[:8] == b"SSMESMK1" and struct.unpack("<q", raw[8:16])[0] == 4
    c = cs[0]
    hd = struct.unpack("<16i", raw[16:80])
    assert hd[:10] == (c["N"], c["tile"], c["B"], c["Bs"], c["R"], c["T"], c["sched"], c["dx"], c["K"], len(c["fids"]))
    per = lambda c: 64 + 8 * c["T"] * c["dx"] * c["R"] * c["npad"] + 4 * c["T"] * c["R"] * c["npad"] + 8 * c["R"] * c["npad"] + \
        16 * c["R"] * c["Bs"] + 8 * c["R"] + 4 * c["R"] * c["K"] + 8 * c["T"] * c["R"] * c["npad"]
    assert len(raw) == 16 + 2 * sum(per(c) for c in cs)
