"""Cases and host reference of tests/cpp/test_smooth_kernels.hip: k_sm_trajectories, k_sm_sweep and k_sm_final (ssme_amd/csrc/smooth.h)
launched alone on histories written by hand.  No device code here; tests/test_smooth_kernel_cases_cpu.py shows the cases are what they
claim, tests/test_smooth_kernels_gpu.py runs the program once and compares.

The reference is smooth_ref.genealogy with the clamp the header of smooth.h promises restated (every ancestor index is min(a, N - 1)
before it is used) plus plain numpy sums.

States come in three kinds:
  code     x_t[d][r][j] = ((((t dx + d) R + r) Npad + j) 2^-20: exact doubles that decode to (t, d, r, j), so a wrong row, plane or filter
           stride shows as a decodable wrong value (decode());
  dyadic   multiples of 1/4 with |x| <= 16.  With integer weights below 2^16 every product x q, x^2 q, 42 q and every partial sum of up
           to 2048 of them is an exact double whatever the order, so the sweep's tile numerators of the functionals 0, 1, 3 must equal
           the integer reference bit for bit (exact_parts(); exactness_margin() is the premise);
  normal   standard normal draws: the sweep is compared tree for tree with k_expect_partials on the host's gather (all four functionals).
Every case is written twice (variant()): with NaN / 0xFFFFFFFF and with zeros in every place the kernels must not look at -- the columns
[N, Npad) of every buffer, the tiles [B, Bs) of the tile sums and maxima, and every row of hanc that sm_resampled says no draw wrote."""
import functools
import struct

import numpy as np

import smooth_ref as sr

ALL4 = (0, 1, 2, 3)
U32MAX = 0xFFFFFFFF
TILES = (512, 1024, 2048)
GENEALOGIES = ("identity", "zero", "last", "reverse", "shift", "random", "coalesce")
CODE_SCALE = 2.0 ** -20


def shape_ns(tile):
    return (1, 2, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile - 5)


def n_tiles(n, tile):
    return (n + tile - 1) // tile


def lib_bs(b):
    return (b + 1) & ~1               # the handles' stride of the per-tile tables (handle_core.h)


def code(t, d, r, j, dx, R, npad):
    return ((((t * dx + d) * R + r) * npad + j)) * CODE_SCALE


def decode(x, dx, R, npad):
    c = int(round(float(x) / CODE_SCALE))
    c, j = divmod(c, npad)
    c, r = divmod(c, R)
    t, d = divmod(c, dx)
    return t, d, r, j


def _ancestors(kind, N, tile, T, R, rng, coalesce_at):
    """[T, R, N] int64; row 0 is filled like every other row (the kernels never read it)."""
    j = np.arange(N, dtype=np.int64)
    a = np.empty((T, R, N), dtype=np.int64)
    for t in range(T):
        for r in range(R):
            if kind == "identity":
                a[t, r] = j
            elif kind == "zero":
                a[t, r] = 0
            elif kind == "last":
                a[t, r] = N - 1
            elif kind == "reverse":
                a[t, r] = N - 1 - j
            elif kind == "shift":
                a[t, r] = (j + tile + 1) % N
            elif kind in ("random", "coalesce"):
                a[t, r] = rng.integers(0, N, N)
            else:
                raise ValueError(kind)
            if kind == "coalesce" and t == coalesce_at:
                a[t, r] = (7 * r + N // 3) % N
    return a


def make_case(name, tile, N, R=1, T=7, sched=1, dx=1, K=None, gen="random", states="code", tmax="equal", bs_extra=0, oor=False,
              dead=None, fids=ALL4, seed=0):
    """One case: inputs (valid parts only) and the reference.  dead: {filter: S value} for filters without weight."""
    rng = np.random.default_rng(1000003 * seed + 7919 * N + tile + 31 * T + sched)
    B = n_tiles(N, tile)
    Bs = lib_bs(B) + bs_extra
    npad = B * tile
    K = N if K is None else K
    assert 1 <= K <= N and T >= 1 and sched >= 1
    coalesce_at = max([t for t in range(1, T) if sr.resampled(t, sched)], default=0)      # the last step that resamples, if any does
    anc = _ancestors(gen, N, tile, T, R, rng, coalesce_at)
    term = rng.integers(0, N, (R, K))
    term[:, 0] = N - 1
    if K > 1:
        term[:, 1] = 0
    if K > 2:
        term[:, 2] = N // 2
    oor_at = []
    if oor:
        bad = (N, npad - 1, U32MAX)
        for t in range(1, T):
            if not sr.resampled(t, sched):
                continue
            for r in range(R):
                # on the last row that resampled the lineages still sit where they started or were sent; rows before it get entries too
                pos = sorted({0, N - 1, N // 2, int(term[r, 0]), int(rng.integers(0, N))})
                for i, p in enumerate(pos):
                    anc[t, r, p] = bad[(i + t + r) % 3]
                    oor_at.append((t, r, p))
    if states == "code":
        t_, d_, r_, j_ = np.meshgrid(np.arange(T), np.arange(dx), np.arange(R), np.arange(N), indexing="ij")
        x = code(t_, d_, r_, j_, dx, R, npad).astype(np.float64)
    elif states == "dyadic":
        x = rng.integers(-64, 65, (T, dx, R, N)).astype(np.float64) / 4.0
    elif states == "normal":
        x = rng.standard_normal((T, dx, R, N))
    else:
        raise ValueError(states)
    q = rng.integers(0, 1 << 16, (R, N)).astype(np.int64)
    q[:, rng.integers(0, N, max(1, N // 8))] = 0                                   # particles without weight
    q[:, 0] = 1 + q[:, 0] % 65535                                                  # every filter keeps some weight (N = 1 too)
    if N > 3:
        q[:, 1] = (1 << 16) - 1
    tix = np.arange(N) // tile
    cdf = np.empty((R, N))
    tsum = np.zeros((R, B))
    for b in range(B):
        m = tix == b
        cdf[:, m] = np.cumsum(q[:, m], axis=1)
        tsum[:, b] = q[:, m].sum(axis=1)
    if tmax == "equal":
        mb = np.zeros((R, B))
    elif tmax == "spread":
        mb = -3.0 * rng.random((R, B))
    elif tmax == "zero-tile":                       # tile 0's scale e^(m_0 - m) underflows to exactly zero (the exp clamps at -746)
        assert B >= 2
        mb = -0.5 * rng.random((R, B))
        mb[:, 0] = mb[:, 1:].max(axis=1) - 800.0
    elif tmax == "nan":                             # the last filter's maximum is NaN: its row is NaN, the others are untouched
        mb = -3.0 * rng.random((R, B))
        mb[R - 1, B - 1] = np.nan
    else:
        raise ValueError(tmax)
    S = tsum.sum(axis=1).astype(np.float64)
    S[S <= 0] = 1.0
    for r, v in (dead or {}).items():
        S[r] = v
    c = dict(name=name, tile=tile, N=N, R=R, T=T, sched=sched, dx=dx, K=K, B=B, Bs=Bs, npad=npad, gen=gen, states=states, tmax=tmax,
             fids=tuple(fids), oor=bool(oor), oor_at=oor_at, dead=dict(dead or {}), coalesce_at=coalesce_at,
             anc=anc, term=term.astype(np.uint32), x=x, q=q, cdf=cdf, tsum=tsum, mb=mb, S=S)
    c.update(reference(c))
    return c


def lineage(c):
    """B [R, T, N]: smooth_ref.genealogy on the clamped ancestors."""
    N = c["N"]
    out = []
    for r in range(c["R"]):
        ancs = [np.minimum(c["anc"][t, r], N - 1) for t in range(c["T"])]
        out.append(sr.genealogy(ancs, c["sched"], n=N))
    return np.stack(out)


def reference(c):
    R, T, N, K, dx = c["R"], c["T"], c["N"], c["K"], c["dx"]
    Bl = lineage(c)
    idx = np.empty((R, K, T), dtype=np.uint32)
    xo = np.empty((R, K, T, dx))
    xg = np.empty((T, R, N))
    for r in range(R):
        for t in range(T):
            bk = Bl[r, t][c["term"][r].astype(np.int64)]
            idx[r, :, t] = bk
            xo[r, :, t, :] = c["x"][t, :, r, :][:, bk].T
            xg[t, r] = c["x"][t, 0, r, Bl[r, t]]
        if not (c["S"][r] > 0.0):
            xo[r] = np.nan
    return dict(B_ref=Bl, idx_ref=idx, x_ref=xo, xg=xg)


def exact_parts(c):
    """dyadic cases: part[t, r, b, f] for the functionals 0, 1, 3 (NaN in the column of any other), from integers."""
    assert c["states"] == "dyadic"
    T, R, B, tile, N = c["T"], c["R"], c["B"], c["tile"], c["N"]
    out = np.full((T, R, B, 4), np.nan)
    xi = np.rint(c["xg"] * 4).astype(np.int64)
    assert np.array_equal(xi / 4.0, c["xg"])
    for b in range(B):
        sl = slice(b * tile, min(N, (b + 1) * tile))
        for col, f in enumerate(c["fids"]):
            if f == 0:
                out[:, :, b, col] = (xi[:, :, sl] * c["q"][None, :, sl]).sum(axis=2) / 4.0
            elif f == 1:
                out[:, :, b, col] = (xi[:, :, sl] ** 2 * c["q"][None, :, sl]).sum(axis=2) / 16.0
            elif f == 3:
                out[:, :, b, col] = 42.0 * c["q"][None, :, sl].sum(axis=2)
    for col in range(len(c["fids"]), 4):
        out[:, :, :, col] = 0.0                     # columns beyond fs.n: the kernel's zero-initialised numerators
    return out


def exactness_margin(c):
    """The largest sum of |terms| of any tile and functional in units of its last place (1/16): every partial sum is an integer below
    this, so below 2^53 all of them are exact doubles in any order."""
    assert c["states"] == "dyadic"
    xi = np.abs(np.rint(c["xg"] * 4).astype(np.int64))
    worst = 0
    for b in range(c["B"]):
        sl = slice(b * c["tile"], min(c["N"], (b + 1) * c["tile"]))
        qq = c["q"][None, :, sl]
        worst = max(worst, int((xi[:, :, sl] ** 2 * qq).sum(axis=2).max()), int(4 * (xi[:, :, sl] * qq).sum(axis=2).max()),
                    int(16 * 42 * qq.sum(axis=2).max()))
    return worst


def exact_out(c):
    """dyadic cases with equal tile maxima (every scale is e^0 = 1): out[t, i, r] = one correctly rounded division of exact sums."""
    assert c["states"] == "dyadic" and c["tmax"] == "equal"
    p = exact_parts(c)
    den = c["tsum"].sum(axis=1)
    out = np.full((c["T"], len(c["fids"]), c["R"]), np.nan)
    for i, f in enumerate(c["fids"]):
        if f != 2:
            out[:, i, :] = p[:, :, :, i].sum(axis=2) / den[None, :]
    return out


def unread_rows(c):
    return [t for t in range(c["T"]) if not sr.resampled(t, c["sched"])]


def variant(c, poison):
    """The buffers as the program gets them.  poison: NaN / 0xFFFFFFFF where the kernels must not look, else zeros there."""
    T, R, N, dx, npad, B, Bs = c["T"], c["R"], c["N"], c["dx"], c["npad"], c["B"], c["Bs"]
    fd, fu = (np.nan, U32MAX) if poison else (0.0, 0)
    hx = np.full((T, dx, R, npad), fd)
    hx[..., :N] = c["x"]
    hanc = np.full((T, R, npad), fu, dtype=np.uint32)
    hanc[..., :N] = (c["anc"] & U32MAX).astype(np.uint32)
    for t in unread_rows(c):
        hanc[t] = fu
    cdf = np.full((R, npad), fd)
    cdf[:, :N] = c["cdf"]
    xg = np.full((T, R, npad), fd)
    xg[..., :N] = c["xg"]
    tsum = np.full((R, Bs), fd)
    tsum[:, :B] = c["tsum"]
    tmax = np.full((R, Bs), fd)
    tmax[:, :B] = c["mb"]
    return dict(hx=hx, hanc=hanc, cdf=cdf, tsum=tsum, tmax=tmax, S=c["S"], term=c["term"], xg=xg)


def sizes(c):
    """Element counts of the program's outputs, in file order."""
    R, K, T, dx, Bs, nf = c["R"], c["K"], c["T"], c["dx"], c["Bs"], len(c["fids"])
    return dict(x=R * K * T * dx, idx=R * K * T, part=T * R * Bs * 4, out=T * nf * R, apart=T * R * Bs * 4, aout=T * nf * R)


def write_cases(path, cs):
    """Every case twice: record 2 i with the poison, record 2 i + 1 with zeros."""
    with open(path, "wb") as f:
        f.write(b"SSMESMK1")
        f.write(struct.pack("<q", 2 * len(cs)))
        for c in cs:
            ids = list(c["fids"]) + [0] * (4 - len(c["fids"]))
            for poison in (True, False):
                v = variant(c, poison)
                f.write(struct.pack("<16i", c["N"], c["tile"], c["B"], c["Bs"], c["R"], c["T"], c["sched"], c["dx"], c["K"], len(c["fids"]),
                                    *ids, 0, 0))
                for k, dt in (("hx", "<f8"), ("hanc", "<u4"), ("cdf", "<f8"), ("tsum", "<f8"), ("tmax", "<f8"), ("S", "<f8"), ("term", "<u4"),
                              ("xg", "<f8")):
                    f.write(np.ascontiguousarray(v[k], dtype=dt).tobytes())


def read_outputs(path, cs):
    """[(poisoned outputs, zeroed outputs)] per case; refuses a file that is short, long or out of order."""
    res = []
    with open(path, "rb") as f:
        assert f.read(8) == b"SSMESMO1"
        assert struct.unpack("<q", f.read(8))[0] == 2 * len(cs)
        for i, c in enumerate(cs):
            pair = []
            for v in range(2):
                assert struct.unpack("<q", f.read(8))[0] == 2 * i + v
                o = {}
                for k, n in sizes(c).items():
                    o[k] = np.fromfile(f, dtype="<u4" if k == "idx" else "<f8", count=n)
                    assert o[k].size == n, (c["name"], k)
                R, K, T, dx, Bs, nf = c["R"], c["K"], c["T"], c["dx"], c["Bs"], len(c["fids"])
                o["x"] = o["x"].reshape(R, K, T, dx)
                o["idx"] = o["idx"].reshape(R, K, T)
                o["part"] = o["part"].reshape(T, R, Bs, 4)
                o["apart"] = o["apart"].reshape(T, R, Bs, 4)
                o["out"] = o["out"].reshape(T, nf, R)
                o["aout"] = o["aout"].reshape(T, nf, R)
                pair.append(o)
            res.append(tuple(pair))
        assert f.read(1) == b""
    return res


@functools.lru_cache(maxsize=None)
def cases():
    """The covering list (built once, never modified).  The sweep over (tile, N) carries the other axes round robin; the named cases
    after it pin what a round robin cannot promise."""
    cs = []
    Ts, kinds = (7, 2, 1, 33, 7), ("code", "dyadic", "normal")
    i = 0
    for tile in TILES:
        for N in shape_ns(tile):
            T = Ts[i % len(Ts)]
            sched = (1, 2, 3, T, T + 1)[(i // 2) % 5]
            dx = 1 + i % 4
            R = (3, 1)[i % 2] if N * dx * T <= 60000 else 1
            ks = [k for k in (1, 255, 1023, 1024, 1025) if k <= N] + [N]
            cs.append(make_case(f"sweep-t{tile}-n{N}", tile, N, R=R, T=T, sched=max(1, sched), dx=dx, K=ks[i % len(ks)],
                                gen=GENEALOGIES[i % len(GENEALOGIES)], states=kinds[i % 3], tmax=("equal", "spread")[(i // 3) % 2], seed=i))
            i += 1
    for tile in TILES:
        big = 3 * tile - 5
        # every genealogy and every state kind at three tiles with a ragged last one, R = 3: the exact check and the codes at each NPL
        cs.append(make_case(f"exact-shift-t{tile}", tile, big, R=3, T=7, sched=1, dx=2, K=1025, gen="shift", states="dyadic", seed=100))
        cs.append(make_case(f"exact-random-t{tile}", tile, big, R=3, T=7, sched=2, dx=1, K=big, gen="random", states="dyadic",
                            bs_extra=2, seed=101))
        cs.append(make_case(f"code-shift-t{tile}", tile, big, R=3, T=7, sched=1, dx=3, K=1024, gen="shift", states="code", seed=102))
        cs.append(make_case(f"code-reverse-t{tile}", tile, tile + 1, R=3, T=7, sched=3, dx=4, K=min(1023, tile + 1), gen="reverse", states="code", seed=103))
        # out-of-range ancestors on paths that are read
        cs.append(make_case(f"oor-t{tile}", tile, big, R=3, T=7, sched=1, dx=2, K=1025, gen="random", states="code", oor=True, seed=104))
        cs.append(make_case(f"oor-small-t{tile}", tile, 257, R=1, T=7, sched=2, dx=1, K=255, gen="identity", states="dyadic", oor=True,
                            bs_extra=1, seed=105))
        # lineages that coalesce; a zero tile scale; a NaN maximum; filters without weight beside live ones
        cs.append(make_case(f"coalesce-t{tile}", tile, big, R=3, T=7, sched=1, dx=1, K=255, gen="coalesce", states="normal", tmax="spread",
                            seed=106))
        cs.append(make_case(f"zero-tile-t{tile}", tile, big, R=3, T=2, sched=1, dx=1, K=1, gen="random", states="normal", tmax="zero-tile",
                            seed=107))
        cs.append(make_case(f"nan-max-t{tile}", tile, tile + 1, R=3, T=7, sched=1, dx=1, K=255, gen="random", states="dyadic", tmax="nan",
                            seed=108))
        cs.append(make_case(f"dead-t{tile}", tile, tile + 1, R=3, T=7, sched=1, dx=2, K=tile + 1, gen="random", states="code",
                            dead={1: 0.0}, seed=109))
    cs.append(make_case("dead-nan-S", 512, 1027, R=3, T=7, sched=3, dx=4, K=1027, gen="random", states="code", dead={0: np.nan, 2: 0.0},
                        seed=110))
    cs.append(make_case("long-33-t512", 512, 1531, R=1, T=33, sched=1, dx=1, K=1025, gen="random", states="dyadic", seed=111))
    cs.append(make_case("long-33-t2048", 2048, 2049, R=1, T=33, sched=2, dx=2, K=1024, gen="shift", states="normal", tmax="spread", seed=112))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return tuple(cs)


# the lineage table of test_hand_written_lineage (tests/test_smooth_kernel_cases_cpu.py): N = 5, T = 4, resamp_sched = 2.  Step 2 is the only
# one that resamples; row 1 and row 3 hold values that would change the table if they were read; entry 4 of row 2 is out of range.
HAND_ANC = np.array([[[9, 9, 9, 9, 9]], [[4, 4, 4, 4, 4]], [[3, 3, 0, 1, 7]], [[0, 0, 0, 0, 0]]])
HAND_B = np.array([[3, 3, 0, 1, 4], [3, 3, 0, 1, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]])
