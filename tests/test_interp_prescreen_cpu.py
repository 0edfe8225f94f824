"""The prescreen of the batched kernel's interpolation medians, on the CPU: the batches of
interp_prescreen_cases.py through the C oracle and the numpy restatement of the prescreen.  No GPU."""
import numpy as np
import pytest

import interp_prescreen_cases as IC

DECIDED = ("plain", "ties", "signed")
REFUSED = ("collision", "near_half", "exact_half")
MIN_ROUNDS = 8  # of the 32


@pytest.mark.parametrize("shape", IC.SHAPES, ids=["%dx%d" % s for s in IC.SHAPES])
@pytest.mark.parametrize("kind", IC.KINDS)
def test_decided_medians_are_the_oracles(kind, shape):
    """Every median the restatement decides at half the margin (so every one the kernel can decide) is
    the oracle's fill of that column, bit for bit."""
    _, kw, c = IC.batch(kind, *shape)
    sc = np.asarray(kw["scaled"]).astype(bool)
    has, d, v = IC.restate(c, sc, 0.5)
    orig, filled = c["original"], c["filled"]
    for b, j in zip(*np.nonzero(d)):
        miss = np.isnan(orig[b, :, j]) | (orig[b, :, j] == 0.0)
        got = filled[b, miss, j]
        assert np.all(got.view(np.uint64) == np.float64(v[b, j]).view(np.uint64)), (kind, shape, b, j, v[b, j], got[0])
    _, d2, _ = IC.restate(c, sc, 2.0)
    assert np.all(d2 <= d) and np.all(d <= has)  # a wider margin decides no more


@pytest.mark.parametrize("kind", DECIDED + REFUSED)
def test_each_kind_takes_its_path(kind):
    """At 50 x 20 (the seeds were chosen on the CPU for this to hold, see the cases module): decided at
    twice the margin, or refused at half of it, in column 0 for the crafted kinds."""
    _, kw, c = IC.batch(kind, 50, 20)
    sc = np.asarray(kw["scaled"]).astype(bool)
    has, d2, _ = IC.restate(c, sc, 2.0)
    _, dh, _ = IC.restate(c, sc, 0.5)
    if kind in IC.CRAFTED or kind == "exact_half":
        has, d2, dh = has[:, :1], d2[:, :1], dh[:, :1]
    rounds = np.count_nonzero(d2.any(axis=1)) if kind in DECIDED else np.count_nonzero((has & ~dh).any(axis=1))
    print(kind, "rounds on the path:", rounds, "bounds:", IC.counter_bounds(kind))
    assert rounds >= MIN_ROUNDS, (kind, rounds)
    if kind in ("collision", "near_half"):  # every median of column 0, and no other column's business
        assert not dh[:, 0].any() and has[:, 0].all()


def test_plain_is_mostly_decided():
    lower, upper, total = IC.counter_bounds("plain")
    print("plain: decided at twice the margin", lower, "at half", upper, "of", total)
    assert total > 0 and lower >= 0.9 * total


def test_near_half_sits_inside_the_margin():
    """Column 0 of near_half: the crossing row's below-sum is T / 2 - 1 of T = 2^21 + 2 in the
    reputations as given, 2^-21 T from half, and the oracle's median is that row's value."""
    R, kw, c = IC.batch("near_half", 50, 20)
    for b in range(IC.B):
        x, w = R[b, :, 0], kw["reputation"][b]
        p = ~np.isnan(x)
        assert float(w[p].sum()) == 2.0 ** 21 + 2 and float(w[p & (x < 0.5)].sum()) == 2.0 ** 20
        assert float(w[x == 0.5].sum()) == 2.0
        assert np.all(c["filled"][b, ~p, 0] == 0.5)


def test_collision_shares_the_key():
    R, _, c = IC.batch("collision", 50, 20)
    a, a2 = np.float64(0.5), np.float64(0.5 * (1.0 + 2.0 ** -30))
    assert a != a2 and IC.key_hi32(np.array([a]))[0] == IC.key_hi32(np.array([a2]))[0]
    for b in range(IC.B):
        x = R[b, :, 0]
        assert np.count_nonzero(x == a) == 1 and np.count_nonzero(x == a2) == 1
        assert np.all(c["filled"][b, np.isnan(x), 0] == a2)  # the second of the pair is the median
