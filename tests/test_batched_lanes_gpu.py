"""The batched kernel's live-lane forms (csrc/pcx_batched.hip: the power iteration's convergence
test by ballot, tree_sum / wave_max over the event rows only, wave_pw_sum_prefix over the lanes
l < N and l < E, rank_avg3's three rankings on three lane groups), bit for bit against the C oracle
(oracle/pcx_oracle_batched.c) on every output, `branch`, `flags` and `pi_iters` included.  32 rounds
per case.

Shapes (synthetic.rounds): 50 x 20 on both compiled instantiations (PCA packed, big-five); N = 50
with E in {1, 2, 15, 16, 17, 21, 22, 32} (one / two event rows, 3 E <= 64 and past it: E = 21 ranks on
lanes 0 .. 62, E = 22 takes the three separate rankings); E = 20 with N in {1, 7, 8, 9, 15, 16, 17, 63,
64} (the pairwise sum's n < 8 branch, T = 1, 2, 8 and tails of 0 .. 7).

Crafted rounds, at E = 20 (compiled kernel) and E = 21 (dynamic kernel) where the rankings are meant.
Each batch was run through the C oracle on the CPU first (test_crafted_rounds_take_their_paths does
it again, with no GPU); the oracle rejects none, so none was dropped or replaced:

* ties: two pairs of event columns duplicated, so `old`, `nv1` and `nv2` hold equal entries and the
  average ranks are half-integers; the oracle takes branch 1 or 2 (the rank rule decides) in most
  rounds;
* nan: one scaled event whose bounds overflow hi - lo: the covariance is not finite (flags & 2),
  every score is NaN and with them `nv1`, `nv2` and their ranks: the rank rule's difference is NaN,
  neither zero nor negative, and the oracle reports branch 2;
* first_step: every reporter files the same row but for one event column, which carries all the
  variance: the start vector is the eigenvector and the loop stops on its first step (pi_iters =
  3 squarings + 1 step + 2 polish steps = 6);
* squaring: two pairs of identical columns with orthogonal patterns (two nearly equal leading
  eigenvalues): the loop runs past 32 steps into an in-loop squaring (pi_iters >= 40) in at least
  eight of the 32 rounds, and stops before it in others (seed fixed after a search on the CPU);
* tiny: unscaled reports of magnitude 1e-160.  The oracle's path, recorded from the CPU run.  Rounds
  0 .. 15 have no missing report: the covariance is tiny but neither zero nor non-finite (flags 0),
  the start vector's squares underflow to zero, its norm is 0 and the iterate is NaN from the start;
  every difference |y - x| is NaN, the SPEC's maximum skips them all (d = 0) and the loop stops on
  its first step (pi_iters = 6) with NaN loadings, scores and rankings (branch 2) -- the NaN edge of
  the convergence test.  Rounds 16 .. 31 keep their missing cells: the fills (1, 1.5 or 2) stand
  beside 1e-160 reports, the covariance is of order one and the iteration runs as usual (finite
  loadings, pi_iters > 6).
"""
import numpy as np
import pytest

B = 32
PI_PRESQUARE, PI_POLISH, PI_SQUARE_EVERY = 3, 2, 32  # csrc/pcx_batched.hip, oracle/pcx_oracle_batched.c
ITERS_FIRST_STEP = PI_PRESQUARE + 1 + PI_POLISH
ITERS_IN_LOOP_SQUARING = PI_SQUARE_EVERY + 1 + PI_POLISH + PI_PRESQUARE + 1

SHAPES = [(50, 20, "PCA"), (50, 20, "big-five")] + \
         [(50, E, "PCA") for E in (1, 2, 15, 16, 17, 21, 22, 32)] + \
         [(N, 20, "PCA") for N in (1, 7, 8, 9, 15, 16, 17, 63, 64)]
CRAFTED = [(kind, E) for kind in ("ties", "nan") for E in (20, 21)] + \
          [("first_step", 20), ("squaring", 20), ("tiny", 20)]
MUST = ("branch", "flags", "pi_iters", "scores", "adj_first_loadings", "smooth_rep", "this_rep", "outcomes_raw",
        "outcomes_final", "certainty", "consensus_reward", "reporter_bonus", "author_bonus", "participation",
        "avg_certainty", "original", "filled")


def _np(outs):
    return {k: v.cpu().numpy() for k, v in outs.items() if not k.startswith("_")}


def _assert_bitexact(g, c, what):
    assert set(MUST) <= set(g) <= set(c), (what, set(MUST) - set(g), set(g) - set(c))
    for k, v in g.items():
        same = (v == c[k]) | (np.isnan(v) & np.isnan(c[k])) if v.dtype.kind == "f" else (v == c[k])
        assert np.all(same), (what, k, int(np.size(same) - np.count_nonzero(same)))


def crafted_rounds(kind, E, N=50):
    """(reports, keyword arguments) of one crafted batch of B rounds."""
    from pyconsensus_amd import synthetic

    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=4100 + 64 * N + E)
    sc, lo, hi = sc.copy(), lo.copy(), hi.copy()
    rng = np.random.default_rng(77 + E)
    i = np.arange(N)
    if kind == "ties":  # columns 1 = 0 and E - 1 = E - 2, bounds included
        for dst, src in ((1, 0), (E - 1, E - 2)):
            R[:, :, dst] = R[:, :, src]
            sc[:, dst], lo[:, dst], hi[:, dst] = sc[:, src], lo[:, src], hi[:, src]
    elif kind == "nan":
        j = E // 2
        sc[:, j], lo[:, j], hi[:, j] = True, -1e308, 1e308
        R[:, :, j] = rng.uniform(-1e307, 1e307, (B, N))
    elif kind == "first_step":
        sc[:] = False
        lo[:], hi[:] = 1.0, 2.0
        R[:] = np.repeat(rng.integers(1, 3, (B, 1, E)).astype(np.float64), N, axis=1)
        R[:, :, E // 3] = rng.integers(1, 3, (B, N))
        R[:, 0, E // 3], R[:, 1, E // 3] = 1.0, 2.0  # (the column varies in every round)
    elif kind == "squaring":
        sc[:] = False
        lo[:], hi[:] = 1.0, 2.0
        R[:] = 1.0
        R[:, :, 0] = R[:, :, 1] = 1.0 + (i % 2)
        R[:, :, E - 2] = R[:, :, E - 1] = 1.0 + ((i // 2) % 2)
        rep = rng.integers(1, 100, (B, N)).astype(np.float64)
        rep[B // 2:] = 50.0 + rng.integers(0, 2, (B - B // 2, N))
    elif kind == "tiny":
        sc[:] = False
        lo[:], hi[:] = 1.0, 2.0
        R = np.where(np.isnan(R), np.nan, 1e-160 * rng.uniform(0.5, 2.0, R.shape))
        full = 1e-160 * rng.uniform(0.5, 2.0, R[:B // 2].shape)
        R[:B // 2] = full  # no missing report in the first half
    else:
        raise ValueError(kind)
    return R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi)


def check_crafted_path(kind, c):
    """The oracle itself took the path the batch was made for."""
    fl, it, br = c["flags"], c["pi_iters"], c["branch"]
    if kind == "ties":
        assert np.all(fl & 3 == 0)
        assert np.count_nonzero((br == 1) | (br == 2)) >= B // 2, br  # the rank rule decided
    elif kind == "nan":
        assert np.all(fl & 2) and np.all(it == 0)
        assert np.all(np.isnan(c["scores"]))
        assert np.all(br == 2), br  # the rank rule's difference is NaN: not 0 (branches 3, 4), not < 0
    elif kind == "first_step":
        assert np.all(fl == 0) and np.all(it == ITERS_FIRST_STEP), (fl, it)
    elif kind == "squaring":
        assert np.all(fl & 3 == 0)
        assert np.count_nonzero(it >= ITERS_IN_LOOP_SQUARING) >= 8, it
        assert np.count_nonzero((it > 0) & (it < ITERS_IN_LOOP_SQUARING)) >= 1, it
    elif kind == "tiny":
        h = B // 2
        assert np.all(fl == 0), fl
        assert np.all(it[:h] == ITERS_FIRST_STEP) and np.all(np.isnan(c["adj_first_loadings"][:h])), it
        assert np.all(np.isnan(c["scores"][:h])) and np.all(br[:h] == 2), br
        assert np.all(it[h:] > ITERS_FIRST_STEP) and not np.any(np.isnan(c["adj_first_loadings"][h:])), it


@pytest.mark.parametrize("case", CRAFTED, ids=["%s_E%d" % c for c in CRAFTED])
def test_crafted_rounds_take_their_paths(case):
    from oracle import pcx_oracle_c as OC

    kind, E = case
    R, kw = crafted_rounds(kind, E)
    check_crafted_path(kind, OC.batched(R, **kw, threads=4))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_%s" % s for s in SHAPES])
def test_shapes_bitexact_vs_c_oracle(gpu_lib, shape):
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched

    N, E, alg = shape
    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=9000 + 64 * N + E)
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    if alg != "PCA":
        kw.update(algorithm=alg, max_components=5, variance_threshold=0.75)
    c = OC.batched(R, **kw, threads=4)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    _assert_bitexact(g, c, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CRAFTED, ids=["%s_E%d" % c for c in CRAFTED])
def test_crafted_bitexact_vs_c_oracle(gpu_lib, case):
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd.batched import consensus_batched

    kind, E = case
    R, kw = crafted_rounds(kind, E)
    c = OC.batched(R, **kw, threads=4)
    check_crafted_path(kind, c)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    _assert_bitexact(g, c, case)
