"""The packed batched kernel's power iteration (csrc/pcx_batched.hip: the iterated matrix squared in
MFMA operand registers, its triangle sharing the covariance's LDS) and its LDS layout.

* bit for bit against the C oracle (oracle/pcx_oracle_batched.c) on every output, `pi_iters` and
  `flags` included, at the shapes that place the 16-wide tile edges (E = 15 / 16 / 17, 31 / 32),
  the k-step edges (E = 1 .. 5, 20 / 21) and the layout edges (N = 1, 2, 7, 63, 64): 256 rounds each;
* hand-made rounds that take the side branches, each checked on the ORACLE's own flags / step
  counts first: a zero covariance (flags & 1), a non-finite one (flags & 2), and a nearly
  repeated leading eigenvalue that keeps the loop running into the in-loop squarings;
* (CPU) the LDS one round asks for: 50 x 20 PCA in eight 1,280-byte units, no packed shape above
  what the layout with an LDS-resident squared matrix asked for.
"""
import numpy as np
import pytest

B = 256
PI_PRESQUARE, PI_POLISH, PI_SQUARE_EVERY = 3, 2, 32  # csrc/pcx_batched.hip, oracle/pcx_oracle_batched.c
# the loop ran past PI_SQUARE_EVERY steps, so it squared once more: it >= 33, sqn >= 4
ITERS_IN_LOOP_SQUARING = PI_SQUARE_EVERY + 1 + PI_POLISH + PI_PRESQUARE + 1

SHAPES = [(50, E) for E in (1, 2, 3, 4, 5, 15, 16, 17, 20, 21, 31, 32)] + \
         [(N, E) for E in (20, 32) for N in (1, 2, 7, 63, 64)]
SIDE_SHAPES = [(50, 20), (50, 16), (50, 17), (50, 4), (64, 32), (7, 20), (63, 32)]


def _np(outs):
    return {k: v.cpu().numpy() for k, v in outs.items() if not k.startswith("_")}


def _assert_bitexact(g, c, what):
    assert {"flags", "pi_iters", "scores", "adj_first_loadings", "smooth_rep"} <= set(g) <= set(c)
    for k, v in g.items():
        same = (v == c[k]) | (np.isnan(v) & np.isnan(c[k])) if v.dtype.kind == "f" else (v == c[k])
        assert np.all(same), (what, k, int(np.size(same) - np.count_nonzero(same)))


def _dyadic_reputation(nb, N):
    """Raw weights whose normalised values and every partial sum are exact (multiples of 2^-k)."""
    p = 1
    while p < N:
        p *= 2
    raw = np.ones((nb, N))
    raw[:, 0] = p - (N - 1)
    return raw


def side_rounds(N, E, seed=11, nb=B):
    """nb hand-made rounds of one shape (32 identical-reporter, 32 overflowing-bounds, the rest
    degenerate-eigenvalue): inputs and the round indices of each kind."""
    rng = np.random.default_rng(seed)
    n_id, n_wide = 32, 32
    n_deg = nb - n_id - n_wide
    assert n_deg >= 2
    sc = np.zeros((nb, E), bool)
    lo, hi = np.ones((nb, E)), 2.0 * np.ones((nb, E))
    R = np.empty((nb, N, E))
    rep = np.empty((nb, N))
    # every reporter files the same row: each centred report is exactly zero
    ident = np.arange(0, n_id)
    R[ident] = np.repeat(rng.integers(1, 3, (n_id, 1, E)).astype(np.float64), N, axis=1)
    rep[ident] = _dyadic_reputation(n_id, N)
    # one scaled event whose bounds are so wide that hi - lo overflows: its rescaled reports, and
    # with them the covariance, are not finite
    wide = np.arange(n_id, n_id + n_wide)
    R[wide] = rng.integers(1, 3, (n_wide, N, E)).astype(np.float64)
    j = E // 2
    sc[wide, j], lo[wide, j], hi[wide, j] = True, -1e308, 1e308
    R[wide, :, j] = rng.uniform(-1e307, 1e307, (n_wide, N))
    rep[wide] = rng.integers(1, 100, (n_wide, N))
    # two pairs of identical columns, the pairs' patterns orthogonal: the covariance has two
    # leading eigenvalues that differ only through the reputations' imbalance
    degen = np.arange(n_id + n_wide, nb)
    i = np.arange(N)
    R[degen] = 1.0
    R[degen, :, 0] = R[degen, :, 1] = 1.0 + (i % 2)
    R[degen, :, E - 2] = R[degen, :, E - 1] = 1.0 + ((i // 2) % 2)
    rep[degen] = rng.integers(1, 100, (n_deg, N))
    rep[degen[n_deg // 2:]] = 50.0 + rng.integers(0, 2, (n_deg - n_deg // 2, N))
    return R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi), dict(ident=ident, wide=wide, degen=degen)


def check_side_branches(c, kinds, nb=B):
    """The oracle itself took the branches the nb rounds were made for."""
    assert len(c["flags"]) == nb == sum(len(v) for v in kinds.values())
    assert np.all(c["flags"][kinds["ident"]] & 1), "identical reporters: zero covariance expected"
    assert np.all(c["pi_iters"][kinds["ident"]] == 0)
    assert np.all(c["flags"][kinds["wide"]] & 2), "overflowing bounds: non-finite covariance expected"
    assert np.all(c["pi_iters"][kinds["wide"]] == 0)
    it = c["pi_iters"][kinds["degen"]]
    assert np.all(c["flags"][kinds["degen"]] & 3 == 0)
    assert np.count_nonzero(it >= ITERS_IN_LOOP_SQUARING) >= 8, "too few rounds reach the in-loop squarings"
    assert np.count_nonzero((it > 0) & (it < ITERS_IN_LOOP_SQUARING)) >= 1  # and some stop before them


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_pca_bitexact_at_tile_and_layout_edges(gpu_lib, shape):
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched

    N, E = shape
    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=1000 + 64 * N + E)
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    c = OC.batched(R, **kw, threads=8)
    if N > 2 and E > 1:
        assert np.count_nonzero(c["pi_iters"] > PI_PRESQUARE + PI_POLISH) > B // 2  # the iteration ran
    _assert_bitexact(g, c, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SIDE_SHAPES, ids=["%dx%d" % s for s in SIDE_SHAPES])
def test_side_branches_bitexact(gpu_lib, shape):
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd.batched import consensus_batched

    R, kw, kinds = side_rounds(*shape)
    c = OC.batched(R, **kw, threads=8)
    check_side_branches(c, kinds)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    _assert_bitexact(g, c, shape)


def test_side_batch_64x32_reaches_the_iteration_cap():
    """The packed kernel's PI_MAXIT exit is compared by test_side_branches_bitexact[64x32]; this shows
    that the batch reaches it: the SPEC stops some degenerate-eigenvalue rounds at the cap (24 of 256)."""
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd._abi import FLAG_PI_MAXIT

    R, kw, kinds = side_rounds(64, 32)
    c = OC.batched(R, **kw, threads=8)
    capped = np.flatnonzero(c["flags"] & FLAG_PI_MAXIT)
    assert len(capped) >= 1 and set(capped) <= set(kinds["degen"]), capped


def _lds_bytes_lds_resident_m(N, E):
    """LDS bytes of a packed round when the squared matrix M had an LDS region of its own (the
    layout before M moved into registers): F | C = max(triangle, n1 n2 smooth adj old) |
    M = max(triangle, median scratch + totals) | miss."""
    c50 = (N, E) == (50, 20)
    ES, NR = (E, 50) if c50 else (E | 1, 64)
    nr, ne, tri = (N + 1) & ~1, (E + 1) & ~1, E * (E + 1) // 2
    cert = (N | 1) if ES & 1 else N
    f = max(N * ES, E * cert)
    med_scr = NR + ((NR + 7) // 8 * 8 + 8) + (NR + 1) // 2
    c = max(tri, 3 * nr + 2 * ne)
    m = max(tri, med_scr + ne, 2 * ne)
    return 8 * (f + c + m + ne)


def test_packed_lds_fits_eight_units():
    from pyconsensus_amd import _lib

    h = _lib.lib()
    PCA, ABSOLUTE, COKURTOSIS = 0, 1, 4  # the packed algorithms
    assert _lds_bytes_lds_resident_m(50, 20) == 11520
    assert 0 < h.pcx_batched_lds_bytes(50, 20, PCA) <= 8 * 1280
    for alg in (PCA, ABSOLUTE, COKURTOSIS):
        for N in range(1, 65):
            for E in range(1, 33):
                got = h.pcx_batched_lds_bytes(N, E, alg)
                assert 0 < got <= _lds_bytes_lds_resident_m(N, E), (alg, N, E, got)
    assert h.pcx_batched_lds_bytes(65, 20, PCA) == -1 and h.pcx_batched_lds_bytes(50, 33, PCA) == -1
