"""Crafted batches for the batched kernel's fill-group test (csrc/pcx_batched_round.inc, a12/a13: an
outcome median decided without the sort) and a numpy restatement of that test.  Builders only: the
tests are test_median_shortcut_cpu.py and test_median_shortcut_gpu.py.

Every batch is B = 32 rounds of N x E made from synthetic.rounds, with column 0 always a scaled column
(so every round has at least one outcome median):

* plain: synthetic.rounds as it is (beside column 0);
* no_missing: the scaled columns have no NaN: no fill, no group, every median sorts;
* exact_half: alpha = 0.0 and integer reputations summing to 1024, so smooth_rep is rep / 1024 exactly
  and every partial sum is exact in any order.  In column 0 the rows below the fill sum to exactly half
  the weight and the missing rows have reputation 0: the interpolation median is the mean of the two
  values around the half, and the outcome median, whose walk reaches exactly half before the fill's
  rows, the mean of the fill and the value above it: two different values.  (A fill group of positive
  weight cannot have exactly half the weight below it: the rows below the fill hold at most half the
  PRESENT weight.)  N = 2 has no room for the three parts (below, missing, above): there column 0 has
  one present row and one missing row of reputation 0;
* far_fill: alpha = 1.0, smooth_rep = this_rep, far from the rep the fill was the median of;
* ties: the scaled columns' bounds are (-8, 8) and their reports lo + 2 q, q = 1 .. 8: the rescaled
  reports are the eighths q / 8 exactly, with present rows equal to the fill in most columns;
* dominant: one reporter holds four times the others' reputation together;
* negative: one reporter's reputation is negative (a quarter of the others' mean);
* zero_rows: present reports equal to lo in column 0: they rescale to 0.0, missing by the reference's
  own rule (__init__.py:278), and take the fill;
* all_missing_column: column 0 is NaN in every row: its fill is NaN.

restate(c, ...) restates the test on the C oracle's own outputs (`original`, `filled`, `smooth_rep`) at
a margin of `scale` times the kernel's relative margin, the half test's DBL_EPSILON kept as it is.  Its
sums run in row order, the kernel's in a tree order, and either is within (N + 6) u W of the exact sum
(u = 2^-53, N <= 64: under 2^-46 W) while the relative margin is 2^-44 W + 2^-45 W.  So a median the
restatement decides at scale 16 the kernel decides too (its own sums clear the margin once), and one the
restatement refuses at scale 0 the kernel refuses (a kernel decision clears 2^-44 W, which row-order
sums then clear with no margin): the two counts bound the kernel's shortcut counter from both sides.

The seeds below were chosen on the CPU (the C oracle and restate(), no GPU) so that each batch takes
its path at 50 x 20 in at least 8 of its 32 rounds (the first seed tried held: 19 rounds for far_fill,
all 32 for the others); test_median_shortcut_cpu.py asserts it again.

The negative batch at 2 x 3 also reaches the power iteration with a negative semidefinite covariance
(two reporters, one negative weight: every diagonal entry is negative), which the start column's
choice has to survive.
"""
import functools

import numpy as np

B = 32
KINDS = ("plain", "no_missing", "exact_half", "far_fill", "ties", "dominant", "negative", "zero_rows",
         "all_missing_column")
SHAPES = [(50, 20), (50, 21), (2, 3), (3, 4), (9, 5), (64, 32)]
DBL_EPS = 2.220446049250313e-16
SEED = 5200  # (+ 64 N + E + 1000 * index of the kind)


def _scaled_values(rng, lo, hi, shape):
    z = np.clip(rng.normal(0.6, 0.15, shape), 0.001, 1.0)
    return lo[:, None] + (hi - lo)[:, None] * z


def build(kind, N, E):
    """(reports, keyword arguments of OC.batched / consensus_batched) of one crafted batch."""
    from pyconsensus_amd import synthetic

    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=SEED + 64 * N + E + 1000 * KINDS.index(kind))
    sc, lo, hi, rep = sc.copy(), lo.copy(), hi.copy(), rep.copy()
    rng = np.random.default_rng(31 + 64 * N + E + 1000 * KINDS.index(kind))
    # column 0: a scaled column in every round, the missing cells where the generator put them
    sc[:, 0] = True
    lo[:, 0] = rng.uniform(-100.0, 0.0, B)
    hi[:, 0] = lo[:, 0] + rng.uniform(1.0, 200.0, B)
    R[:, :, 0] = np.where(np.isnan(R[:, :, 0]), np.nan, _scaled_values(rng, lo[:, 0], hi[:, 0], (B, N)))
    kw = {}
    if kind == "plain":
        pass
    elif kind == "no_missing":
        for j in range(E):
            fresh = _scaled_values(rng, lo[:, j], hi[:, j], (B, N))
            R[:, :, j] = np.where(sc[:, j][:, None] & np.isnan(R[:, :, j]), fresh, R[:, :, j])
    elif kind == "exact_half":
        kw["alpha"] = 0.0
        n_miss = max(1, N // 10)
        n_lo = (N - n_miss) // 2
        n_hi = N - n_miss - n_lo

        def parts(n):  # n positive integers summing to 512
            return 1 + rng.multinomial(512 - n, np.full(n, 1.0 / n)) if n else np.zeros(0, dtype=np.int64)

        for b in range(B):
            order = rng.permutation(N)
            r_lo, r_miss, r_hi = order[:n_lo], order[n_lo:n_lo + n_miss], order[n_lo + n_miss:]
            span = hi[b, 0] - lo[b, 0]
            R[b, r_lo, 0] = lo[b, 0] + span * rng.uniform(0.1, 0.4, n_lo)
            R[b, r_hi, 0] = lo[b, 0] + span * rng.uniform(0.6, 0.9, n_hi)
            R[b, r_miss, 0] = np.nan
            rep[b, r_miss] = 0.0
            if n_lo:
                rep[b, r_lo], rep[b, r_hi] = parts(n_lo), parts(n_hi)
            else:  # N = 2: one present row, one missing row of reputation 0
                rep[b, r_hi] = 1024.0 / n_hi
    elif kind == "far_fill":
        kw["alpha"] = 1.0
    elif kind == "ties":
        q = rng.integers(1, 9, (B, N, E)).astype(np.float64)
        lo[sc], hi[sc] = -8.0, 8.0
        R = np.where(sc[:, None, :] & ~np.isnan(R), -8.0 + 2.0 * q, R)
    elif kind == "dominant":
        r = rng.integers(0, N, B)
        others = rep.sum(axis=1) - rep[np.arange(B), r]
        rep[np.arange(B), r] = 4.0 * np.maximum(others, 1.0)
    elif kind == "negative":
        r = rng.integers(0, N, B)
        others = rep.sum(axis=1) - rep[np.arange(B), r]
        rep[np.arange(B), r] = -0.25 * np.maximum(others, 1.0) / max(N - 1, 1)
    elif kind == "zero_rows":
        for b in range(B):
            rows = rng.permutation(N)[:max(1, N // 8)]
            R[b, rows, 0] = lo[b, 0]
            if N > 1:  # (a present row stays beside them where there is room)
                keep = rng.permutation(np.setdiff1d(np.arange(N), rows))[0]
                if np.isnan(R[b, keep, 0]):
                    R[b, keep, 0] = lo[b, 0] + 0.5 * (hi[b, 0] - lo[b, 0])
    elif kind == "all_missing_column":
        R[:, :, 0] = np.nan
    else:
        raise ValueError(kind)
    kw.update(reputation=rep, scaled=sc, lo=lo, hi=hi)
    return R, kw


@functools.lru_cache(maxsize=None)
def batch(kind, N, E):
    """(reports, keyword arguments, the C oracle's outputs) of a crafted batch, computed once."""
    from oracle import pcx_oracle_c as OC

    R, kw = build(kind, N, E)
    return R, kw, OC.batched(R, **kw, threads=4)


def _seq_sum(v):
    t = 0.0
    for a in v:
        t = t + float(a)
    return t


def shortcut_decides(x, w, miss, scale):
    """The kernel's fill-group test of one filled column x with weights w and missing rows `miss`
    at `scale` times its relative margin: (decided, fill)."""
    if not miss.any():
        return False, None
    Wt = _seq_sum(w)
    mid, slack = 0.5 * Wt, scale * 2.0 ** -45 * Wt
    M = scale * 2.0 ** -44 * Wt + slack + DBL_EPS
    if not M < np.inf:
        return False, None
    if not np.all((w >= 0.0) & (w < mid - slack)) or not np.any(w > 0.0):  # (a NaN weight fails the first)
        return False, None
    g = x[np.flatnonzero(miss)[0]]
    if np.isnan(x).any() or not (g != 0.0 and abs(g) < 2.0 ** 1023):  # (a NaN fill fails abs(g) < ...)
        return False, None
    below, group = _seq_sum(w[x < g]), _seq_sum(w[x == g])
    return bool(below <= mid - M and below + group > mid + M), g


def restate(c, scaled, scale):
    """Per (round, scaled column) of the oracle's outputs c: decided [B][E] bool, fill [B][E]."""
    orig, filled, smooth = c["original"], c["filled"], c["smooth_rep"]
    nb, _, E = orig.shape
    decided, fill = np.zeros((nb, E), dtype=bool), np.full((nb, E), np.nan)
    for b in range(nb):
        for j in np.flatnonzero(scaled[b]):
            miss = np.isnan(orig[b, :, j]) | (orig[b, :, j] == 0.0)
            d, g = shortcut_decides(filled[b, :, j], smooth[b], miss, scale)
            if d:
                decided[b, j], fill[b, j] = True, g
    return decided, fill


def counter_bounds(kind, N=50, E=20):
    """(lower, upper, total) of the kernel's shortcut counter over the batch: the medians the
    restatement decides at 16 times the margin, the total less those it refuses at none, the total."""
    _, kw, c = batch(kind, N, E)
    total = int(np.count_nonzero(kw["scaled"]))
    d16, _ = restate(c, kw["scaled"], 16.0)
    d0, _ = restate(c, kw["scaled"], 0.0)
    return int(np.count_nonzero(d16)), int(np.count_nonzero(d0)), total
