"""Crafted batches for the batched kernel's guess sums (csrc/pcx_batched_round.inc, phase a3: the fast
sums of a column's present rows, row-split over three lane groups, and the exact replay) and a numpy
restatement of the fast test.  Builders only: the tests are test_guess_sums_cpu.py and
test_guess_sums_gpu.py.

Every batch is B = 32 rounds of N x E made from synthetic.rounds.  Column 0 is a binary column in every
round (reports 1.0 / 2.0, the missing cells where the generator put them) unless the kind says otherwise:

* plain: the bench generator as it is (beside column 0);
* threshold: column 0's present-weighted mean sits on a catch threshold or within 1e-13 relative of
  it.  Even rounds: integer reputations with 4 of 10 (rounds 0, 4, ...: 1.4 = 1.5 - catch_tol) or 6 of 10
  (rounds 2, 6, ...: 1.6) of the present weight on the twos.  Odd rounds: the present weight is
  10 * 2^40 with 4 * 2^40 + 1 (or 6 * 2^40 + 1) on the twos: the mean lies 9.1e-14 above the threshold,
  6.5e-14 of its value.  Either way the fast test must refuse and the guess come from the replay.
  (N < 3 has no room for a missing row, a one and a two: there the column stays as generated);
* wide: reputations 2^e (1 + u), e uniform in [-40, 40]: the row-split total and the sequential one
  differ in their last bits in most columns;
* half_ties: wide, and column 0 a scaled column with bounds (0, 1), an even count of present rows and
  equal pairs of reputations, one row of each pair below the middle value and one above: the running
  sum of the lower half is exactly half the total, the prescreen refuses, and the sort divides by the
  exact sequential total;
* uniform: reputation = None;
* signed: one reporter's reputation is negative (a quarter of the others' mean): no fast sums;
* zero_weight: the present rows of column 0 all have reputation 0 (the total is 0, the guess NaN's catch);
* all_missing: column 0 (binary) and, where E > 1, the last column (made scaled) are NaN in every row;
* none_missing: no NaN anywhere: no fill;
* nonfinite: an infinite report (+inf in the even rounds, -inf in the odd ones) in column 0, beside a
  missing row.

restate(R, kw, scale) restates the fast test of every binary column with a missing report from
row-order fp64 sums of the normalised reputations, against `scale` times the kernel's margin
1e-12 * sum|rep F| / tot.  The kernel's sums (row-split, fused multiply-adds) are within (2 N + 22) u,
u = 2^-53, of the sums' magnitudes from these (N - 1 additions and N products here, N / 3 + 2 additions
there): under 2^-45 relative at N <= 64, where the margin is 2^-40.
So a column the restatement passes at scale 2 the kernel passes too, and one the kernel passes the
restatement passes at scale 0.5: the two counts bound the kernel's replay counter.
"""
import functools

import numpy as np

import median_shortcut_cases as MC

B = MC.B
KINDS = ("plain", "threshold", "wide", "half_ties", "uniform", "signed", "zero_weight", "all_missing",
         "none_missing", "nonfinite")
SHAPES = [(50, 20), (50, 21), (50, 22), (64, 32), (64, 21), (1, 1), (2, 3), (3, 4), (9, 5)]
SEED = 9100  # (+ 64 N + E + 1000 * index of the kind)
CATCH_TOL = 0.1


def _wide(rng, shape):
    return 2.0 ** rng.integers(-40, 41, shape).astype(np.float64) * (1.0 + rng.random(shape))


def build(kind, N, E):
    """(reports, keyword arguments of OC.batched / consensus_batched) of one batch."""
    from pyconsensus_amd import synthetic

    k = KINDS.index(kind)
    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=SEED + 64 * N + E + 1000 * k)
    sc, lo, hi, rep = sc.copy(), lo.copy(), hi.copy(), rep.copy()
    rng = np.random.default_rng(53 + 64 * N + E + 1000 * k)
    sc[:, 0], lo[:, 0], hi[:, 0] = False, 1.0, 2.0
    R[:, :, 0] = np.where(np.isnan(R[:, :, 0]), np.nan, rng.integers(1, 3, (B, N)).astype(np.float64))
    if kind in ("wide", "half_ties"):
        rep = _wide(rng, (B, N))
    if kind == "threshold" and N >= 3:
        for b in range(B):
            n_miss = max(1, N // 10)
            order = rng.permutation(N)
            r_miss, pres = order[:n_miss], order[n_miss:]
            n2 = max(1, len(pres) // 2)
            twos, ones = pres[:n2], pres[n2:]
            unit = 1 if b % 2 == 0 else 2 ** 40
            w2 = (4 if b % 4 < 2 else 6) * unit + (b % 2)
            w1 = 10 * unit - w2
            if b % 2 == 0 and (len(twos) > 4 or len(ones) > 4):  # small integers: ten units per part
                w2, w1 = 10 * w2, 10 * w1
            R[b, twos, 0], R[b, ones, 0], R[b, r_miss, 0] = 2.0, 1.0, np.nan
            for rows, w in ((twos, w2), (ones, w1)):  # positive integers summing to w
                rep[b, rows] = 1.0
                rep[b, rows[0]] = float(w - (len(rows) - 1))
            assert rep[b, pres].min() >= 1.0
    elif kind == "half_ties":
        sc[:, 0], lo[:, 0], hi[:, 0] = True, 0.0, 1.0
        for b in range(B):
            n_miss = max(1, N // 10)
            if (N - n_miss) % 2:
                n_miss += 1
            n_miss = min(n_miss, N)
            order = rng.permutation(N)
            r_miss, pres = order[:n_miss], order[n_miss:]
            h = len(pres) // 2
            x = np.sort(rng.uniform(0.05, 0.95, 2 * h))
            R[b, pres, 0], R[b, r_miss, 0] = x, np.nan  # pres[q] below the middle, pres[h + q] above
            rep[b, pres[h:]] = rep[b, pres[:h]]
    elif kind == "signed":
        r = rng.integers(0, N, B)
        others = rep.sum(axis=1) - rep[np.arange(B), r]
        rep[np.arange(B), r] = -0.25 * np.maximum(others, 1.0) / max(N - 1, 1)
    elif kind == "zero_weight":
        for b in range(B):
            r_miss = rng.permutation(N)[:max(1, N // 10)]
            R[b, r_miss, 0] = np.nan
            keep = np.zeros(N, dtype=bool)
            keep[r_miss] = True
            rep[b, ~keep] = 0.0
    elif kind == "all_missing":
        R[:, :, 0] = np.nan
        if E > 1:
            sc[:, E - 1] = True
            lo[:, E - 1] = rng.uniform(-100.0, 0.0, B)
            hi[:, E - 1] = lo[:, E - 1] + rng.uniform(1.0, 200.0, B)
            R[:, :, E - 1] = np.nan
    elif kind == "none_missing":
        fresh_b = rng.integers(1, 3, (B, N, E)).astype(np.float64)
        for j in range(E):
            fresh = MC._scaled_values(rng, lo[:, j], hi[:, j], (B, N))
            fill = np.where(sc[:, j][:, None], fresh, fresh_b[:, :, j])
            R[:, :, j] = np.where(np.isnan(R[:, :, j]), fill, R[:, :, j])
    elif kind == "nonfinite":
        for b in range(B):
            order = rng.permutation(N)
            R[b, order[0], 0] = np.inf if b % 2 == 0 else -np.inf
            if N > 1:
                R[b, order[1], 0] = np.nan
    kw = dict(reputation=None if kind == "uniform" else rep, scaled=sc, lo=lo, hi=hi)
    return R, kw


@functools.lru_cache(maxsize=None)
def batch(kind, N, E):
    """(reports, keyword arguments, the C oracle's outputs) of a batch, computed once."""
    from oracle import pcx_oracle_c as OC

    R, kw = build(kind, N, E)
    return R, kw, OC.batched(R, **kw, threads=4)


def normalised(kw, N):
    """[B][N] the reputations as the reference normalises them (numpy's sum, then a division each)."""
    rep = kw["reputation"]
    if rep is None:
        return np.full((B if np.ndim(kw["scaled"]) > 1 else 1, N), 1.0 / float(N))
    return np.stack([r / float(np.sum(r)) for r in np.asarray(rep, dtype=np.float64)])


def sums(X, rep, split):
    """tot, sp, sa [B][E] of the present rows of the reports X [B][N][E] (NaN or 0.0 = missing) under
    the reputations rep [B][N]: in row order, or (split) over the rows g, g + 3, g + 6, ... of each of
    three groups in ascending order, combined as (p0 + p1) + p2 -- the kernel's row-split order."""
    nb, N, E = X.shape
    miss = np.isnan(X) | (X == 0.0)
    with np.errstate(all="ignore"):
        re = np.where(miss, 0.0, rep[:, :, None])
        f = np.where(miss, 0.0, X)

        def run(rows):
            tot, sp, sa = np.zeros((nb, E)), np.zeros((nb, E)), np.zeros((nb, E))
            for i in rows:
                tot = tot + re[:, i]
                sp = sp + re[:, i] * f[:, i]
                sa = sa + np.abs(re[:, i]) * np.abs(f[:, i])
            return tot, sp, sa

        if not split:
            return run(range(N))
        p = [run(range(g, N, 3)) for g in range(3)]
        return tuple((p[0][q] + p[1][q]) + p[2][q] for q in range(3))


def restate(R, kw, scale, split=False, tol=CATCH_TOL):
    """Per (round, binary column with a missing report): has [B][E] bool, fast [B][E] bool (the fast
    test passes at `scale` times the margin), value [B][E] (catch of the fast quotient)."""
    X = np.asarray(R, dtype=np.float64)
    nb, N, E = X.shape
    sc = np.asarray(kw["scaled"]).astype(bool)
    rep = normalised(kw, N)
    has = ~sc & (np.isnan(X) | (X == 0.0)).any(axis=1)
    tot, sp, sa = sums(X, rep, split)
    with np.errstate(all="ignore"):
        acc, margin = sp / tot, scale * (1e-12 * (sa / tot))
        t_lo, t_hi = 1.5 - tol, 1.5 + tol
        fast = (tot > 0.0) & np.isfinite(acc) & np.isfinite(margin) & (np.abs(acc - t_lo) > margin) & (
            np.abs(acc - t_hi) > margin)
        value = np.where(acc < t_lo, 1.0, np.where(acc > t_hi, 2.0, 1.5))
    return has, has & fast, value


def replay_bounds(kind, N=50, E=20):
    """(lower, upper, total) of the kernel's count of replayed binary columns over the batch: those the
    restatement refuses at half the margin, those it refuses at twice the margin, all binary columns
    with a missing report."""
    R, kw = build(kind, N, E)
    has, f_half, _ = restate(R, kw, 0.5)
    _, f_twice, _ = restate(R, kw, 2.0)
    total = int(np.count_nonzero(has))
    return total - int(np.count_nonzero(f_half)), total - int(np.count_nonzero(f_twice)), total
