"""The fill-group test of the batched kernel's outcome medians, on the CPU: the crafted batches of
median_shortcut_cases.py through the C oracle and the numpy restatement of the test.  No GPU."""
import numpy as np
import pytest

import median_shortcut_cases as MC

DECIDES = ("plain", "ties")  # at least one median decided at 16 times the margin
REFUSES = ("exact_half", "far_fill", "no_missing", "dominant", "negative", "all_missing_column")  # refused at none
MIN_ROUNDS = 8  # of the 32


@pytest.mark.parametrize("kind", DECIDES + REFUSES)
def test_each_batch_takes_its_path(kind):
    """At 50 x 20 (the seeds were chosen on the CPU for this to hold, see the cases module)."""
    _, kw, c = MC.batch(kind, 50, 20)
    sc = kw["scaled"].astype(bool)
    assert np.all(sc.any(axis=1))  # every round has an outcome median
    if kind in DECIDES:
        d16, _ = MC.restate(c, sc, 16.0)
        rounds = np.count_nonzero(d16.any(axis=1))
    else:
        d0, _ = MC.restate(c, sc, 0.0)
        rounds = np.count_nonzero((sc & ~d0).any(axis=1))
    print(kind, "rounds on the path:", rounds, "bounds:", MC.counter_bounds(kind))
    assert rounds >= MIN_ROUNDS, (kind, rounds)


def test_exact_half_is_a_mean_of_two_values():
    """Column 0 of exact_half: the oracle's outcome median is neither the fill nor a report, but the
    mean of the fill and the report above it, and the weight below the fill is exactly half."""
    _, kw, c = MC.batch("exact_half", 50, 20)
    for b in range(MC.B):
        x, w = c["filled"][b, :, 0], c["smooth_rep"][b]
        miss = np.isnan(c["original"][b, :, 0])
        g = x[miss][0]
        assert np.all(w[miss] == 0.0) and float(np.sum(w[x < g])) == 0.5 and float(np.sum(w)) == 1.0
        above = np.min(x[x > g])
        assert c["outcomes_raw"][b, 0] == (g + above) / 2.0 and g < c["outcomes_raw"][b, 0] < above


@pytest.mark.parametrize("shape", MC.SHAPES, ids=["%dx%d" % s for s in MC.SHAPES])
@pytest.mark.parametrize("kind", MC.KINDS)
def test_decided_medians_are_the_oracles(kind, shape):
    """Wherever the restated test decides (at the kernel's margin, and at 16 times it), the oracle's
    outcomes_raw is the fill bit for bit."""
    _, kw, c = MC.batch(kind, *shape)
    sc = kw["scaled"].astype(bool)
    for scale in (1.0, 16.0):
        d, g = MC.restate(c, sc, scale)
        assert np.array_equal(c["outcomes_raw"][d].view(np.uint64), g[d].view(np.uint64)), (kind, shape, scale)
    d1, _ = MC.restate(c, sc, 1.0)
    d16, _ = MC.restate(c, sc, 16.0)
    d0, _ = MC.restate(c, sc, 0.0)
    assert np.all(d16 <= d1) and np.all(d1 <= d0)  # a wider margin decides no more
