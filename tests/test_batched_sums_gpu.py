"""The batched kernel's pairwise sums with the accumulator chains in lanes 0..7 (csrc/pcx_batched.hip:
wave_pw_sum_lds, its paired form, wave_pw_sum_dpp) and the fill-group sums of every scaled column in one
pass over three lane groups (csrc/pcx_batched_round.inc), bit for bit against the C oracle
(oracle/pcx_oracle_batched.c) on every output, `branch`, `flags` and `pi_iters` included.  32 rounds per
case.

Pairwise edges (synthetic.rounds): E = 20 with N in {7, 8, 9, 15, 16, 17, 23, 24, 25, 47, 48, 49, 50, 55,
56, 57, 63, 64} and N = 50 with E in {7, 8, 9, 15, 16, 17, 20, 21, 23, 24, 25, 31, 32}: T = 1 .. 8 full
rounds of eight, tails of 0 .. 7, the n < 8 branch, the register form of the column sums (E < 24) and the
permuted one past it; 50 x 20 on both compiled instantiations, the rest on the dynamic kernels.

Crafted rounds.  Each batch was run through the C oracle on the CPU first
(test_crafted_rounds_take_their_paths does it again, with no GPU):

* identical: every reporter files the same complete row, under dyadic reputation shares (the weighted
  mean is exact).  The covariance is zero (flags & 1), every score is 0, both score sets are all zero and
  both of normalize()'s re-sum branches run, and the reputation update's after them (this_rep = 1 / N);
* negzero: caller-supplied scores (cokurtosis).  Rounds 0 .. 15: every score is -0.0 (both sets are all
  zero again); rounds 16 .. 31: -0.0 among negative scores, so the larger extreme is -0.0;
* tiny: unscaled reports of magnitude 1e-160 (test_batched_lanes_gpu's recipe): subnormal partial sums.

Fill-group batches, at E = 20 (compiled kernel: lane groups) and E = 22 (dynamic kernel: the loop):

* no_scaled: no scaled column;
* all_scaled: every column scaled (bounds 0, 1: the rescale is exact), a tenth of the reports missing;
  the outcome median equals the fill in nearly every column;
* scaled_full: the synthetic rounds with every missing report of a scaled column filed: scaled columns
  with no missing row;
* fill_zero: column 0 scaled, rows 32 .. 49 missing, the other reports -0.5 and 0.5 in equal number
  under equal dyadic weights: the interpolation median is the mean of the two, a fill of exactly 0.0;
* nan_value: one scaled column whose bounds overflow hi - lo: every report of it rescales to 0.0, which
  counts as missing, the fill is NaN and so is every value of the column;
* neg_rep: one negative reputation, large enough that the reporter's smooth_rep is negative too;
* dominant: reporter 0's reputation share runs from 0.40 to 0.60 over the rounds, so its share of
  smooth_rep lies just under half in some rounds and just over in others (the dominant-weight exit:
  the outcome median is then reporter 0's own value);
* eighths: every column scaled with reports on the grid 1/8 .. 8/8: tie groups of about six rows.
"""
import numpy as np
import pytest

B = 32
N0 = 50
PW_SHAPES = [(50, 20, "PCA"), (50, 20, "big-five")] + \
            [(N, 20, "PCA") for N in (7, 8, 9, 15, 16, 17, 23, 24, 25, 47, 48, 49, 55, 56, 57, 63, 64)] + \
            [(50, E, "PCA") for E in (7, 8, 9, 15, 16, 17, 21, 23, 24, 25, 31, 32)]
PW_CRAFTED = ["identical", "negzero", "tiny"]
FG_KINDS = ["no_scaled", "all_scaled", "scaled_full", "fill_zero", "nan_value", "neg_rep", "dominant", "eighths"]
FG_CRAFTED = [(kind, E) for kind in FG_KINDS for E in (20, 22)]
CRAFTED = [(kind, 20) for kind in PW_CRAFTED] + FG_CRAFTED
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


def crafted_rounds(kind, E, N=N0):
    """(reports, keyword arguments) of one crafted batch of B rounds."""
    from pyconsensus_amd import synthetic

    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=5200 + 64 * N + E)
    sc, lo, hi = sc.copy(), lo.copy(), hi.copy()
    rng = np.random.default_rng(131 + E)
    kw = {}
    if kind == "identical":
        sc[:] = False
        lo[:], hi[:] = 1.0, 2.0
        R = np.repeat(rng.integers(1, 3, (B, 1, E)).astype(np.float64), N, axis=1)
        # 36 ones and 14 twos, total 64: every share is dyadic, every sum of them exact in any order, so
        # the weighted mean is the common report exactly and the covariance is exactly zero
        rep = rng.permuted(np.repeat(np.where(np.arange(N) < 36, 1.0, 2.0)[None, :], B, axis=0), axis=1)
    elif kind == "negzero":
        aux = -rng.uniform(0.5, 2.0, (B, N))
        aux[:, ::3] = -0.0
        aux[:B // 2] = -0.0
        kw.update(algorithm="cokurtosis", aux_scores=aux)
    elif kind == "tiny":
        sc[:] = False
        lo[:], hi[:] = 1.0, 2.0
        R = np.where(np.isnan(R), np.nan, 1e-160 * rng.uniform(0.5, 2.0, R.shape))
        R[:B // 2] = 1e-160 * rng.uniform(0.5, 2.0, R[:B // 2].shape)
    elif kind == "no_scaled":
        binary = rng.integers(1, 3, R.shape).astype(np.float64)
        R = np.where(sc[:, None, :] & ~np.isnan(R), binary, R)
        sc[:] = False
        lo[:], hi[:] = 1.0, 2.0
    elif kind in ("all_scaled", "eighths"):
        sc[:] = True
        lo[:], hi[:] = 0.0, 1.0
        if kind == "all_scaled":
            V = rng.uniform(0.001, 1.0, R.shape)
        else:
            V = rng.integers(1, 9, R.shape) / 8.0
        R = np.where(np.isnan(R), np.nan, V)
    elif kind == "scaled_full":
        sc[:, 0] = True  # (every round has one)
        lo[:, 0], hi[:, 0] = 0.0, 1.0
        R[:, :, 0] = rng.uniform(0.001, 1.0, (B, N))
        V = lo[:, None, :] + (hi - lo)[:, None, :] * rng.uniform(0.1, 1.0, R.shape)
        R = np.where(sc[:, None, :] & np.isnan(R), V, R)
    elif kind == "fill_zero":
        sc[:, 0] = True
        lo[:, 0], hi[:, 0] = 0.0, 1.0
        # reputations 36 ones and 14 twos (total 64: dyadic shares); rows 0 .. 31 present, sixteen of each
        # sign, each of weight (1 / 64) / (32 / 64) = 1 / 32 exactly: the running sum meets half exactly
        R[:, :, 0] = np.where(np.arange(N) % 2 == 0, -0.5, 0.5)
        R[:, 32:, 0] = np.nan
        rep = np.repeat(np.where(np.arange(N) < 36, 1.0, 2.0)[None, :], B, axis=0)
    elif kind == "nan_value":
        j = E // 2
        sc[:, j], lo[:, j], hi[:, j] = True, -1e308, 1e308
        R[:, :, j] = rng.uniform(-1e307, 1e307, (B, N))
    elif kind == "neg_rep":
        sc[:, 0] = True
        lo[:, 0], hi[:, 0] = 0.0, 1.0
        R[:, :, 0] = np.where(rng.random((B, N)) < 0.1, np.nan, rng.uniform(0.001, 1.0, (B, N)))
        rep = rep.copy()
        rep[np.arange(B), rng.integers(0, N, B)] = -60.0
    elif kind == "dominant":
        sc[:, 0] = True
        lo[:, 0], hi[:, 0] = 0.0, 1.0
        R[:, :, 0] = rng.uniform(0.001, 1.0, (B, N))
        R[:, 1::7, 0] = np.nan
        rep = rep.copy()
        s = np.linspace(0.40, 0.60, B)
        rep[:, 0] = rep[:, 1:].sum(axis=1) * s / (1.0 - s)
    else:
        raise ValueError(kind)
    kw.update(reputation=rep, scaled=sc, lo=lo, hi=hi)
    return R, kw


def _fills(c, kw):
    """(b, j, fill, outcomes_raw) of every scaled column with a missing row: the fill read from the column's
    first missing row of `filled`, as the kernel reads it."""
    miss = np.isnan(c["original"]) | (c["original"] == 0.0)
    out = []
    for b, j in zip(*np.nonzero(kw["scaled"] & miss.any(axis=1))):
        i = int(np.argmax(miss[b, :, j]))
        out.append((b, j, c["filled"][b, i, j], c["outcomes_raw"][b, j]))
    return out


def check_crafted_path(kind, c, kw):
    """The oracle itself took the path the batch was made for."""
    fl, br, sm = c["flags"], c["branch"], c["smooth_rep"]
    sc = kw["scaled"]
    miss = np.isnan(c["original"]) | (c["original"] == 0.0)
    fills = _fills(c, kw)
    if kind == "identical":
        assert np.all(fl & 1) and np.all(c["scores"] == 0.0), fl
        assert np.all((br == 3) | (br == 4)), br  # equal rankings: the rank rule's difference is 0
        # every nonconformity is 0: normalize() adds 1 and sums again, this_rep is 1 / N
        assert np.all(c["this_rep"] == 1.0 / c["this_rep"].shape[1])
    elif kind == "negzero":
        s = c["scores"]
        assert np.all(np.signbit(s[:B // 2]) & (s[:B // 2] == 0.0))
        assert np.all(np.any(np.signbit(s[B // 2:]) & (s[B // 2:] == 0.0), axis=1))
        assert np.all(s[B // 2:].max(axis=1) == 0.0) and np.all(s[B // 2:].min(axis=1) < 0.0)
    elif kind == "tiny":
        assert np.all(fl == 0), fl
        assert np.all(np.isnan(c["scores"][:B // 2])) and np.all(br[:B // 2] == 2), br
        assert not np.any(np.isnan(c["adj_first_loadings"][B // 2:]))
    elif kind == "no_scaled":
        assert not sc.any() and not fills
    elif kind in ("all_scaled", "eighths"):
        assert sc.all() and len(fills) >= B * sc.shape[1] * 9 // 10
        same = sum(1 for _, _, g, r in fills if g == r)
        assert same >= len(fills) * 3 // 4, (same, len(fills))  # the outcome median is the fill
        if kind == "eighths":
            assert np.all(np.isin(c["outcomes_raw"] * 16.0, np.arange(1, 17)))  # a grid value or a mean of two
    elif kind == "scaled_full":
        assert np.all(sc.sum(axis=1) >= 1) and not fills
        assert not miss[np.broadcast_to(sc[:, None, :], miss.shape)].any()
    elif kind == "fill_zero":
        zero = [(b, j) for b, j, g, _ in fills if j == 0 and g == 0.0]
        assert len(zero) == B, len(zero)
        assert np.all(c["filled"][:, 32:, 0] == 0.0)
    elif kind == "nan_value":
        j = sc.shape[1] // 2
        assert np.all(np.isnan(c["filled"][:, :, j])) and np.all(np.isnan(c["outcomes_raw"][:, j]))
    elif kind == "neg_rep":
        assert np.all(sm.min(axis=1) < 0.0), sm.min(axis=1)
        assert all(any(bb == b for bb, _, _, _ in fills) for b in range(B))
    elif kind == "dominant":
        share = sm[:, 0] / sm.sum(axis=1)
        assert np.count_nonzero((share > 0.47) & (share < 0.5)) >= 3, share
        assert np.count_nonzero((share > 0.5) & (share < 0.53)) >= 3, share
        over = share > 0.5 + 1e-9
        assert np.all(c["outcomes_raw"][over, 0] == c["filled"][over, 0, 0])  # reporter 0's own value
        assert np.all(~np.isnan(c["original"][:, 0, 0]) & np.isnan(c["original"][:, 1, 0]))


@pytest.mark.parametrize("case", CRAFTED, ids=["%s_E%d" % c for c in CRAFTED])
def test_crafted_rounds_take_their_paths(case):
    from oracle import pcx_oracle_c as OC

    kind, E = case
    R, kw = crafted_rounds(kind, E)
    check_crafted_path(kind, OC.batched(R, **kw, threads=4), kw)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PW_SHAPES, ids=["%dx%d_%s" % s for s in PW_SHAPES])
def test_pairwise_edges_bitexact_vs_c_oracle(gpu_lib, shape):
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched

    N, E, alg = shape
    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=9300 + 64 * N + E)
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
    check_crafted_path(kind, c, kw)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    _assert_bitexact(g, c, case)
