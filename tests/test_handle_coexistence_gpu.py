"""Handles of different sizes alive in one process (-m gpu).  The dynamic-LDS ceiling of a kernel is state of the (kernel, device) pair
that every handle shares (grant_lds, csrc/handle_core.h): creating and running a handle that needs less must not take away what a
handle that needs more was granted.  The pairs below launch the SAME instantiations with different LDS sizes; the handle that needs more
is run, the smaller one is created and run, and the first must then repeat its own results bit for bit.  No oracle: a handle is
compared with itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048
THETA = [1.0, 0.95, 0.25]                   # SVOL: beta, phi, sigma
N_BIG = 1024 * TILE + 1                     # 1025 tiles: in-kernel level-2 of 81920 bytes of LDS, the smallest shape above 64 KiB
N_SMALL = 129 * TILE                        # 129 tiles: the same WL2 = false instantiations (more than 128 tiles), 53248 bytes
LW_N_BIG = 1024 * TILE                      # 1024 tiles: the largest in-kernel shape of the Liu-West stages, 65536 bytes
LW_N_SMALL = 2049                           # 2 tiles
SEED = 7


@pytest.fixture(scope="module")
def sa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ssme_amd
    from ssme_amd import _capi
    assert _capi.lib() is not None        # the in-tree HIP library is what runs
    return ssme_amd


@pytest.fixture(scope="module")
def y3(spy):
    return spy[:3]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bank(sa, n, device=0):
    b = sa.ParticleFilterBank(sa.MODEL_SVOL, n, 1, seed=SEED, tile=TILE, device=device)
    b.set_debug(False, False, split_level2=False)       # the in-kernel level-2: the one whose LDS grows with the tile count
    b.set_params(THETA)
    return b


def _run(f, y):
    """(loglik, per_step) of one series, as bits."""
    ll = f.run_series(y)
    return _bits(ll), _bits(f.per_step())


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _bootstrap_pair(sa, y3, small_device):
    big = _bank(sa, N_BIG)
    assert (big.tile, big.n_tiles) == (TILE, 1025)
    first_big = _run(big, y3)
    assert np.all(np.isfinite(first_big[1].view(np.float64)))
    small = _bank(sa, N_SMALL, device=small_device)
    assert (small.tile, small.n_tiles) == (TILE, 129)
    small.set_graph_mode(False)
    first_small = _run(small, y3)
    assert np.all(np.isfinite(first_small[1].view(np.float64)))
    small.set_graph_mode(True)
    assert _same(_run(small, y3), first_small)
    big.set_seed(SEED)
    assert _same(_run(big, y3), first_big)
    assert _same(_run(small, y3), first_small)
    small.close()
    big.close()


def test_bootstrap_small_handle_does_not_lower_big_handles_grant(sa, y3):
    _bootstrap_pair(sa, y3, small_device=0)


def test_bootstrap_handles_on_two_devices(sa, y3):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    _bootstrap_pair(sa, y3, small_device=1)


def test_liu_west_small_handle_does_not_lower_big_handles_grant(sa, y3):
    def make(n):
        return sa.svol_lw_1_par(0.99, 0.8, 0.99, -0.1, 0.1, 0.01, 0.1, -0.5, -0.01, nparts=n, seed=SEED)
    big = make(LW_N_BIG)
    first_big = _run(big, y3)
    assert np.all(np.isfinite(first_big[1].view(np.float64)))
    small = make(LW_N_SMALL)
    assert np.all(np.isfinite(small.run_series(y3)))
    assert _same(_run(big, y3), first_big)
    small.close()
    big.close()
