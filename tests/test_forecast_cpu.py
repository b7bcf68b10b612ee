"""The forecast's reference (tests/forecast_ref.py) against independent statements of the start draw, and the argument checks of the
two entry points -- no device.

  * one tile: the fixed point of the level-2 is the tile's own (rshift = 41 for Npad = 2048), so A' = A, ratio = 1 and the draw is
    np.searchsorted of ceil(u A) on the exact integer cdf;
  * several tiles of different maxima, many zero weights: every drawn index carries weight (q > 0), and no tile whose rescaled
    sum underflowed to zero is ever chosen;
  * over the 2^40 midpoint grid of u the number of grid points that choose tile b is A'_b 2^40 / S up to the two grid points at
    its borders: found by bisection over the grid index (the choice is monotone in u) and compared with T analytically;
  * ssme_pf_sim_future_obs / ssme_lw_sim_future_obs return SSME_ERR_INVALID_ARG for a NULL handle, a NULL y_out and num_steps
    outside 1 .. 65535 before they touch the handle or HIP.
"""
import ctypes as C

import numpy as np

import forecast_ref as fr

SEED = 0x1234567887654321


def _uniforms(oracle, n, t0=4, rep=5):
    w = fr.philox_rows(oracle, np.arange(n), t0, rep, fr.STREAM_START, SEED)
    return fr.u01_mid40(w[:, 0], w[:, 1])


def _synthetic(rng, n, tile, zero_frac=0.5):
    """Tile-local integer cdf, tile sums and tile maxima of n particles with many zero weights."""
    q = rng.integers(1, 2 ** 41, size=n, dtype=np.int64)
    q[rng.random(n) < zero_frac] = 0
    starts = np.arange(0, n, tile)
    for s in starts:                                   # every tile's maximum weight is 2^41 (log-weight = the tile maximum)
        q[s + rng.integers(0, min(tile, n - s))] = 2 ** 41
    cdf = np.concatenate([np.cumsum(q[s:s + tile]) for s in starts])
    return q, cdf.astype(np.uint64), np.add.reduceat(q, starts).astype(np.uint64)


def test_u01_mid40_is_the_device_formula(oracle):
    """2 - bits(1.0 | w0 << 20 | (w1 >> 24) << 12 | 0x800) of csrc/ssme_math.h, restated with integers."""
    rng = np.random.default_rng(0)
    w0, w1 = rng.integers(0, 2 ** 32, 1000, dtype=np.uint64), rng.integers(0, 2 ** 32, 1000, dtype=np.uint64)
    w0[:2], w1[:2] = (0, 2 ** 32 - 1), (0, 2 ** 32 - 1)
    man = (w0 << np.uint64(20)) | ((w1 >> np.uint64(24)) << np.uint64(12)) | np.uint64(0x800)
    want = 2.0 - (man | np.uint64(0x3ff0000000000000)).view(np.float64)
    got = fr.u01_mid40(w0, w1)
    assert np.array_equal(got, want) and got.min() > 0.0 and got.max() < 1.0


def test_one_tile_draw_is_searchsorted_on_the_integer_cdf(oracle):
    rng = np.random.default_rng(1)
    for n in (1, 2, 500, 2048):
        q, cdf, A = _synthetic(rng, n, 2048)
        Ap, T, S, ratio = fr.level2(oracle, A, np.array([-3.25]), 41)
        assert int(Ap[0]) == int(A[0]) and ratio[0] == 1.0 and S == float(A[0])
        u = _uniforms(oracle, n)
        got = fr.start_from_uniforms(u, cdf, T, S, ratio, n, 2048)
        want = np.minimum(np.searchsorted(cdf.astype(np.int64), np.ceil(u * float(A[0])).astype(np.int64), side="left"), n - 1)
        assert np.array_equal(got, want)
        assert (q[got] > 0).all()


def test_several_tiles_draw_only_weighted_particles(oracle):
    rng = np.random.default_rng(2)
    tile, n = 512, 3 * 512 + 7
    q, cdf, A = _synthetic(rng, n, tile)
    mb = np.array([-1.0, -30.5, -0.25, -800.0])        # the last tile's scale underflows: A' = 0
    rshift = 52 - 11                                   # Npad = 2048
    Ap, T, S, ratio = fr.level2(oracle, A, mb, rshift)
    assert Ap[3] == 0 and (Ap[:3] > 0).all() and len(set(Ap[:3].tolist())) == 3
    u = _uniforms(oracle, 4 * n)
    anc = fr.start_from_uniforms(u, cdf, T, S, ratio, n, tile)
    assert (q[anc] > 0).all()
    assert (anc // tile < 3).all() and set((anc // tile).tolist()) == {0, 2}       # tile 1 weighs e^-30: not among 6000 draws
    # the reference's start_draw on the same state agrees with the pieces above
    st = dict(cdf=cdf, A=A, mb=mb, rshift=rshift)
    got, alive = fr.start_draw(oracle, st, n, tile, SEED, 5, 4)
    assert alive and np.array_equal(got, anc[:n])


def test_tile_frequencies_over_the_grid(oracle):
    rng = np.random.default_rng(3)
    tile, n = 512, 5 * 512
    _, _, A = _synthetic(rng, n, tile)
    mb = np.array([-2.0, -0.5, -7.0, -0.125, -40.0])
    Ap, T, S, _ = fr.level2(oracle, A, mb, 52 - 12)

    def tile_of(k):                                    # grid index k -> tile, exactly as the draw computes it
        u = 1.0 - (float(k) * 2.0 + 1.0) * 2.0 ** -41
        return int(fr.tile_of_target(T, np.ceil(np.array([u * S])))[0])

    # u decreases with k, so the chosen tile is nonincreasing in k: first_k[b] = the smallest k that chooses a tile <= b
    counts = []
    upper = 2 ** 40
    for b in range(T.size - 1, -1, -1):
        lo, hi = 0, upper                              # smallest k in [0, upper] with tile_of(k) < b  (upper if none)
        while lo < hi:
            mid = (lo + hi) // 2
            if tile_of(mid) < b:
                hi = mid
            else:
                lo = mid + 1
        counts.append((b, lo))
    first_below = dict(counts)                         # k from which on the tile is < b
    for b in range(T.size):
        nxt = first_below[b + 1] if b + 1 < T.size else 0
        cnt = first_below[b] - nxt                     # grid points that choose tile b
        assert abs(cnt - float(Ap[b]) * 2.0 ** 40 / S) <= 2.0, (b, cnt)
    assert first_below[0] == 2 ** 40


def test_dead_filter_has_no_draw(oracle):
    st = dict(cdf=np.zeros(7, dtype=np.uint64), A=np.zeros(1, dtype=np.uint64), mb=np.array([-np.inf]), rshift=41, x=np.arange(7.0))
    start, x, y = fr.forecast_bs(oracle, fr.MODEL_SVOL, [1.0, 0.9, 0.2], st, 7, 2048, SEED, 0, 3, 2)
    assert not start.any() and np.isnan(x).all() and np.isnan(y).all()


def test_arguments_are_validated_before_the_handle_is_touched():
    from ssme_amd import _capi
    L = _capi.lib()
    y = np.zeros(8)
    fake = C.create_string_buffer(1 << 16)             # zero bytes: never read when an argument is invalid
    hfake = C.cast(fake, C.c_void_p)
    lo = np.zeros(1)
    for fn, tail in ((L.ssme_pf_sim_future_obs, (None, None)), (L.ssme_lw_sim_future_obs, (None, None, None))):
        assert fn(None, 1, _capi.dptr(lo), _capi.dptr(y), *tail) == _capi.ERR_INVALID_ARG
        assert fn(hfake, 1, _capi.dptr(lo), None, *tail) == _capi.ERR_INVALID_ARG
        for bad in (0, -1, 65536, 2 ** 31 - 1):
            assert fn(hfake, bad, _capi.dptr(lo), _capi.dptr(y), *tail) == _capi.ERR_INVALID_ARG
    assert L.ssme_lw_sim_future_obs(hfake, 1, None, _capi.dptr(y), None, None, None) == _capi.ERR_INVALID_ARG      # last_obs is required
