"""The fast test of the batched kernel's binary guesses, on the CPU: the batches of guess_sums_cases.py
through the Python oracle's interpolation and the numpy restatement of the fast test, with row-order sums
and with the kernel's row-split order.  No GPU."""
import numpy as np
import pytest

import guess_sums_cases as GC

IDS = ["%dx%d" % s for s in GC.SHAPES]


def _reference_fill(R, kw, b):
    """The Python oracle's filled reports of round b."""
    from oracle.pcx_oracle import OracleCPU
    from pyconsensus_amd import synthetic

    rep = kw["reputation"]
    o = OracleCPU(R[b], synthetic.bounds_list(kw["scaled"][b], kw["lo"][b], kw["hi"][b]),
                  None if rep is None else rep[b], catch_tolerance=GC.CATCH_TOL)
    with np.errstate(all="ignore"):
        return np.asarray(o.interpolate(o.reports))


@pytest.mark.parametrize("shape", GC.SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", GC.KINDS)
def test_fast_columns_are_the_references(kind, shape):
    """Every binary column the restatement decides at half the margin (so every one the kernel can
    decide), from row-order sums or from the row-split ones, holds the reference's guess in its missing
    rows; and a wider margin decides no more."""
    R, kw = GC.build(kind, *shape)
    fills = {}
    for split in (False, True):
        has, fast, value = GC.restate(R, kw, 0.5, split=split)
        _, fast2, _ = GC.restate(R, kw, 2.0, split=split)
        assert np.all(fast2 <= fast) and np.all(fast <= has)
        for b, j in zip(*np.nonzero(fast)):
            if b not in fills:
                fills[b] = _reference_fill(R, kw, b)
            miss = np.isnan(R[b, :, j]) | (R[b, :, j] == 0.0)
            assert np.all(fills[b][miss, j] == value[b, j]), (kind, shape, split, b, j, value[b, j], fills[b][miss, j])


def test_plain_replay_share():
    """2,048 rounds of the bench generator: of the binary columns with a missing report the fast test
    leaves 4 of 30,418 to the replay, from row-order sums and from the row-split ones alike, far under
    the 1 % the replay may cost."""
    from pyconsensus_amd import synthetic

    R, sc, lo, hi, rep = synthetic.rounds(2048, 50, 20, seed=20261015)
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    has, fast, value = GC.restate(R, kw, 1.0)
    _, fast_s, value_s = GC.restate(R, kw, 1.0, split=True)
    total, left = int(np.count_nonzero(has)), int(np.count_nonzero(has & ~fast))
    print("binary columns with a missing report", total, "left to the replay", left, "row-split",
          int(np.count_nonzero(has & ~fast_s)))
    assert total == 30418 and left == 4
    assert left <= 0.01 * total
    assert np.array_equal(fast, fast_s)
    assert np.array_equal(value[fast], value_s[fast])


def test_threshold_is_replayed():
    """Column 0 of threshold at 50 x 20: the present-weighted mean is on 1.4 or 1.6 or within 1e-13
    relative of it, and the fast test refuses it even at half the margin."""
    R, kw = GC.build("threshold", 50, 20)
    has, fast, _ = GC.restate(R, kw, 0.5)
    assert has[:, 0].all() and not fast[:, 0].any()
    rep = kw["reputation"]
    for b in range(GC.B):
        x = R[b, :, 0]
        p = ~np.isnan(x)
        w2, w = int(rep[b, p & (x == 2.0)].sum()), int(rep[b, p].sum())  # (exact: integers under 2^53)
        target = 4 if b % 4 < 2 else 6
        d = 10 * w2 - target * w  # the mean less the threshold is d / (10 w)
        if b % 2 == 0:
            assert d == 0
        else:
            assert 0 < d <= 1e-13 * (1.0 + target / 10.0) * 10 * w
    lower, upper, total = GC.replay_bounds("threshold")
    print("threshold: replayed at half the margin", lower, "at twice", upper, "of", total)
    assert GC.B <= lower <= upper < total


def test_wide_totals_differ():
    """wide at 50 x 20: the row-split total and the sequential one differ in at least half of the
    columns with a missing report, so a consumer of the exact total cannot take the split one."""
    R, kw = GC.build("wide", 50, 20)
    rep = GC.normalised(kw, 50)
    seq, spl = GC.sums(R, rep, False)[0], GC.sums(R, rep, True)[0]
    miss = (np.isnan(R) | (R == 0.0)).any(axis=1)
    differ = int(np.count_nonzero((seq != spl) & miss))
    print("wide: totals differ in", differ, "of", int(np.count_nonzero(miss)))
    assert differ >= 0.5 * np.count_nonzero(miss)
    assert np.all(np.abs(seq - spl) <= 67 * 2.0 ** -53 * seq)  # (N + ceil(N / 3)) u, no cancellation


def test_half_ties_sit_on_half():
    """Column 0 of half_ties: an even count of present rows in equal pairs of reputations, one of each
    pair on either side of the middle."""
    R, kw = GC.build("half_ties", 50, 20)
    for b in range(GC.B):
        x, w = R[b, :, 0], kw["reputation"][b]
        p = np.flatnonzero(~np.isnan(x))
        assert len(p) % 2 == 0 and len(p) >= 2
        order = p[np.argsort(x[p])]
        h = len(p) // 2
        assert sorted(w[order[:h]]) == sorted(w[order[h:]])
