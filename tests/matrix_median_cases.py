"""Crafted weighted-median columns for the single-matrix path (csrc/pcx_mat_select.hip, pcx_mat_hard.hip,
select() / hard_replay() of pcx_runner.cpp), shared by test_matrix_median_cpu.py (the generators' coverage
and stability, checked on the numpy restatement alone) and test_matrix_median_gpu.py.  Needs no GPU.

One N x 32 matrix per KIND: the first columns are `synthetic.matrix` columns (at least eight of them
binary: the power iteration keeps a well-separated first component), the last ones are crafted, each
scaled on [0, 8] (x / 8 is exact), each steering the column's fill median (phase 1, __init__.py:303) and
outcome median (phase 2, :520-523) into one branch of the selection.  A kind is a reputation vector (a
group that needs its own gets its own matrix) plus alpha; a kind whose column fills with NaN stands alone
too, since a NaN fill poisons the reputations and with them every other column's outcome.

Phase-2 ties: smooth_rep differs between numpy and the GPU in its last bits, so an outcome median that
sits on an exact tie would be decided by rounding.  The tie kinds run with alpha = 0.0 (smooth_rep is
old_rep itself, asserted by `preconditions`); every crafted column of the other kinds must keep its
outcome median when the weights move by +-1e-12 relative (`stability`).

The group the issue calls `fill-outside` (int_dtype=True, present rescaled values in (0.3, 0.9), truncated
fill 0.0) cannot exist: an integer report matrix truncates the RESCALED reports as well (:269 assigns into
the integer array; rescale() of pcx_mat_device.h), so every present value of a scaled column is a nonzero
integer (0 is the missing report, :278), and a truncated median or mean of two of nonzero integers lies
between them.  The guard of k_sel_hist it was meant for (vreuse refused by a changed range) is therefore
not reachable through truncation; kind "int" runs the nearest thing that exists, `fill-truncated`: the
average 1.5 of the middle values 1 and 2, stored as 1."""
import functools
import math
import sys
from fractions import Fraction

import numpy as np

import golden_cases as G

E = 32
LO, HI = 0.0, 8.0
N_SMALL = 2203   # routes (a), (c), (d): three unequal shards of more than one 1,024-row sample span each
N_TIERS = 8200   # route (b): the smallest ragged-16 size above SEL_EXACT_MAX
SEL_EXACT_MAX = 8192  # pcx_internal.h
MAX_SEL_PASSES = 12   # pcx_runner.cpp
ZERO_EVERY = 7        # kinds with sprinkled zero reputations: every 7th reporter

# kind -> (reputation, alpha, int_dtype, crafted groups in column order)
_PLAIN = ("duplicates", "zeros-sprinkled", "one-present-last-rank", "constant", "no-missing", "deep",
          "fill-equals-present")
_COUNT = ("tie-count-far", "tie-count-ulp", "duplicates", "constant", "no-missing", "deep")
KINDS = {
    "given": ("integer", 0.1, False, _PLAIN),
    "nan": ("integer", 0.1, False, _PLAIN + ("zero-weight-only", "all-missing")),
    "none": (None, 0.0, False, _COUNT),            # tie-count-far / tie-count-ulp
    "constant": ("constant", 0.0, False, _COUNT),  # tie-count-given: the same columns, explicit equal weights
    "dyadic": ("dyadic", 0.0, False, ("tie-weights", "duplicates")),
    "thirds": ("thirds", 0.0, False, ("tie-above", "duplicates")),
    "dominant-r0": ("dominant-r0", 0.1, False, ("dominant", "dominant-missing", "duplicates")),
    "dominant-rlast": ("dominant-rlast", 0.1, False, ("dominant", "dominant-missing", "duplicates")),
    "negative": ("negative", 0.1, False, ("duplicates", "fill-equals-present", "negative-weights")),
    "int": (None, 0.0, True, ("fill-truncated", "duplicates-int")),
}
TIE_KINDS = tuple(k for k, v in KINDS.items() if v[1] == 0.0)
NAN_KINDS = ("nan",)


def dkey(x):
    """The selection's order-preserving u64 key of a double (pcx_device.h dkey), as a Python int."""
    u = int(np.float64(x + 0.0).view(np.uint64))
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def _pow2_at_most(n):
    p = 1
    while 2 * p <= n:
        p *= 2
    return p


def _last_rank_row(N):
    """A row of the last of three shards whose reputation is not one of the sprinkled zeros."""
    r = N - 4
    while r % ZERO_EVERY == 0:
        r -= 1
    return r


def dominant_row(kind, N):
    return 5 if kind == "dominant-r0" else _last_rank_row(N)


def zero_weight_rows(N):
    """Three reporters without reputation, one in each of three shards."""
    return [ZERO_EVERY, ZERO_EVERY * (N // (2 * ZERO_EVERY)), ZERO_EVERY * ((N - 1) // ZERO_EVERY)]


# ---------------------------------------------------------------- reputations
def _tie_layout(N):
    """tie-weights: rows 1 .. P carry the column, P the largest power of two <= (N - 1) / 2."""
    return _pow2_at_most((N - 1) // 2)


def _thirds_layout(N):
    """tie-above: rows 1 .. L at 2.0 with raw weight 3, rows L + 1 .. 4 L at 6.0 with raw weight 1."""
    return _pow2_at_most((N - 1) // 8)


def _reputation(mode, N, base, seed):
    if mode is None:
        return None
    if mode == "constant":
        return np.full(N, 3.0)
    r = np.asarray(base, dtype=np.float64).copy()
    if mode == "integer":
        r[::ZERO_EVERY] = 0.0
    elif mode == "negative":  # 10% flipped, as test_matrix_gpu._signed_reputation
        flip = np.random.default_rng(seed).random(N) < 0.1
        r[flip] = -r[flip]
    elif mode in ("dominant-r0", "dominant-rlast"):  # one reporter outweighs all the others together
        d = dominant_row(mode, N)
        r[d] = 2.0 * (r.sum() - r[d]) + 1.0
    elif mode == "dyadic":
        # the total is a power of two: rep / sum(rep) and every partial sum of it are exact.  Rows 1 .. P
        # weigh 1, 3, 3, 1, ... (the tie column puts 2.0, 6.0, 2.0, 6.0, ... on them: 4 a side per four
        # rows), every other row 1, row 0 the rest of the power of two (below half of it)
        P = _tie_layout(N)
        r[:] = 1.0
        r[1:P + 1] = np.tile([1.0, 3.0, 3.0, 1.0], P // 4)
        rest = r[1:].sum()
        total = 2.0 * _pow2_at_most(int(rest))
        r[0] = total - rest
        assert 1.0 <= r[0] < 0.5 * total
    elif mode == "thirds":
        # the total is 3 * 2^m: a raw 3 normalises to 2^-m exactly, a raw 1 to fl(1 / 3) 2^-m, BELOW a third
        L = _thirds_layout(N)
        r[:] = 1.0
        r[1:L + 1] = 3.0
        rest = r[1:].sum()
        total = 3.0 * _pow2_at_most(int(rest) // 3 + 1)
        while total <= rest:
            total *= 2.0
        r[0] = total - rest
        assert 1.0 <= r[0] < 0.5 * total and math.log2(total / 3.0) % 1 == 0
    else:
        raise KeyError(mode)
    return r


def normalized(rep, N):
    """old_rep as the reference forms it (__init__.py:138-145)."""
    if rep is None:
        return np.array([1 / float(N)] * N)
    return np.asarray(rep, dtype=np.float64) / float(np.sum(np.asarray(rep)))


# ---------------------------------------------------------------- the crafted columns
DEEP_TOP = 53  # keys up to bits(0.5) + 2^53, the double 2.0


def deep_keys():
    """(below, above): bit patterns around M = bits(0.5).  M - 2^e for e = 0 .. 60 and the double 1e-300
    below; M + 2^e for e = 0 .. 53 above (0.5 + 2^e 2^-53 up to 1.0, then 2.0)."""
    M = int(np.float64(0.5).view(np.uint64))
    below = [M - (1 << e) for e in range(61)] + [int(np.float64(1e-300).view(np.uint64))]
    above = [M + (1 << e) for e in range(DEEP_TOP + 1)]
    return below, above


def _even_count_with_half(a, n_max):
    """The largest even n <= n_max at which the reference's walk over n equal weights `a` (phase 1: each
    divided by their sequential total, :294-302) stops on the DBL_EPSILON half test -- whether it does
    depends on the rounding of the n sequential additions alone (pcx_seqsum.h replays them)."""
    from oracle.pcx_oracle import weighted_median

    n = n_max - n_max % 2
    while n >= 4:
        r = np.full(n, a)
        w = r / np.cumsum(r)[-1]
        if weighted_median(np.arange(n, dtype=np.float64), w) == (n - 1) / 2.0:
            return n
        n -= 2
    raise AssertionError("no even count whose equal-weight walk stops at the half")


def _column(group, kind, N, base_col, rep, rng):
    """Raw reports (on [0, 8]; NaN = missing) of one crafted column."""
    nan = np.isnan(base_col)
    ints = np.where(nan, np.nan, rng.integers(1, 8, N).astype(np.float64))
    if group in ("duplicates", "negative-weights"):
        return ints  # seven distinct values: every first-pass bucket holds one key
    if group == "zeros-sprinkled":
        # reporters without reputation among the present ones; the column's extremes belong to two of them
        ints[0], ints[1], ints[ZERO_EVERY] = 0.5, np.nan, 7.5
        return ints
    if group == "one-present-last-rank":
        col = np.full(N, np.nan)
        col[_last_rank_row(N)] = 4.0
        return col
    if group == "constant":
        return np.where(nan, np.nan, 3.0)
    if group == "no-missing":
        return rng.uniform(1.0, 7.0, N)
    if group == "fill-equals-present":
        # 30% missing: their weight sits on the fill value, a present report, and carries the outcome median
        col = rng.uniform(1.0, 7.0, N)
        col[rng.random(N) < 0.3] = np.nan
        return col
    if group == "deep":
        below, above = deep_keys()
        rows = rng.permutation(np.flatnonzero(~nan))
        n = len(rows)
        a, b = (3 * n) // 10, (3 * n) // 10 + (7 * n) // 20
        assert b - a >= len(below) and n - b >= len(above)
        bits = np.empty(n, dtype=np.uint64)
        bits[:a] = int(np.float64(0.5).view(np.uint64))  # 30% of the rows on the median itself
        bits[a:b] = np.resize(np.array(below, dtype=np.uint64), b - a)
        bits[b:] = np.resize(np.array(above, dtype=np.uint64), n - b)
        col = np.full(N, np.nan)
        col[rows] = bits.view(np.float64) * 8.0  # (a power of two: exact both ways)
        return col
    if group in ("tie-count-far", "tie-count-ulp"):
        a = normalized(rep, N)[0]
        n = _even_count_with_half(a, (9 * N) // 10)
        rows = rng.permutation(N)[:n]
        col = np.full(N, np.nan)
        if group == "tie-count-far":
            lo_v, hi_v = rng.uniform(1.0, 2.0, n // 2), rng.uniform(6.0, 7.0, n // 2)
            lo_v[0], hi_v[0] = 2.0, 6.0
        else:
            lo_v, hi_v = rng.uniform(1.0, 4.9, n // 2), rng.uniform(5.1, 7.0, n // 2)
            lo_v[0], hi_v[0] = 5.0, np.nextafter(5.0, 8.0)
        col[rows[:n // 2]], col[rows[n // 2:]] = lo_v, hi_v
        return col
    if group == "tie-weights":
        P = _tie_layout(N)
        col = np.full(N, np.nan)
        col[1:P + 1] = np.tile([2.0, 6.0, 2.0, 6.0], P // 4)
        return col
    if group == "tie-above":
        L = _thirds_layout(N)
        col = np.full(N, np.nan)
        col[1:L + 1], col[L + 1:4 * L + 1] = 2.0, 6.0
        return col
    if group in ("dominant", "dominant-missing"):
        d = dominant_row(kind, N)
        ints[d] = 3.0 if group == "dominant" else np.nan
        ints[(d + 1) % N] = np.nan
        return ints
    if group == "zero-weight-only":
        col = np.full(N, np.nan)
        col[zero_weight_rows(N)] = [5.0, 2.0, 6.0]
        return col
    if group == "all-missing":
        return np.full(N, np.nan)
    raise KeyError(group)


class Case:
    """One matrix: inputs (read only), the crafted columns {group: column}, and how to call with them."""

    def __init__(self, kind, N, R, sc, lo, hi, rep, alpha, int_dtype, cols):
        self.kind, self.N, self.R, self.sc, self.lo, self.hi, self.rep = kind, N, R, sc, lo, hi, rep
        self.alpha, self.int_dtype, self.cols = alpha, int_dtype, cols
        for a in (R, sc, lo, hi) + (() if rep is None else (rep,)):
            a.setflags(write=False)

    @property
    def bounds(self):
        from pyconsensus_amd import synthetic

        return synthetic.bounds_list(self.sc, self.lo, self.hi)

    def oracle_kw(self):
        """Constructor arguments of OracleCPU and of the drop-in Oracle (a fresh reports array: both
        rescale it in place)."""
        return dict(reports=self.R.copy(), event_bounds=self.bounds, reputation=self.rep, alpha=self.alpha)

    @property
    def crafted(self):
        return sorted(self.cols.values())


@functools.lru_cache(maxsize=None)
def case(kind, N):
    from pyconsensus_amd import synthetic

    mode, alpha, int_dtype, groups = KINDS[kind]
    seed = 7000 + N
    R, sc, lo, hi, base_rep = synthetic.matrix(N, E, seed=seed)
    R, sc, lo, hi = R.copy(), sc.copy(), lo.copy(), hi.copy()
    first = E - len(groups)
    assert np.count_nonzero(~sc[:first]) >= 8, "fewer than eight binary columns left"
    rep = _reputation(mode, N, base_rep, seed)
    rng = np.random.default_rng(seed + 1)
    cols = {}
    if int_dtype:
        return _int_case(kind, N, R, sc, lo, hi, alpha, groups, rng)
    for k, g in enumerate(groups):
        j = first + k
        col = _column(g, kind, N, R[:, j], rep, rng)
        sc[j], lo[j], hi[j] = True, LO, HI
        R[:, j] = col
        cols[g] = j
    return Case(kind, N, R, sc, lo, hi, rep, alpha, False, cols)


def _int_case(kind, N, R, sc, lo, hi, alpha, groups, rng):
    """An int64 report matrix (no NaN: 0 is the missing report).  The base's scaled columns become noisy
    copies of binary ones; a crafted column scaled on [0, 8] holds raw 8 k .. 8 k + 7 for the rescaled,
    truncated value k (:269)."""
    binary = np.flatnonzero(~sc)
    for j in np.flatnonzero(sc):
        src = R[:, binary[j % len(binary)]]
        R[:, j] = np.where(rng.random(N) < 0.2, 3.0 - src, src)
        sc[j], lo[j], hi[j] = False, 1.0, 2.0
    R[np.isnan(R)] = 0.0
    first = E - len(groups)
    cols = {}
    for k, g in enumerate(groups):
        j = first + k
        col = np.zeros(N)
        if g == "fill-truncated":  # an even count under equal weights, the middle values 1 and 2: 1.5 -> 1
            n = _even_count_with_half(1 / float(N), (9 * N) // 10)
            rows = rng.permutation(N)[:n]
            col[rows[:n // 2]] = rng.integers(8, 16, n // 2)
            col[rows[n // 2:]] = rng.integers(16, 24, n // 2)
        else:  # duplicates-int: the values 1 .. 7
            col = np.where(rng.random(N) < 0.1, 0.0, rng.integers(8, 64, N).astype(np.float64))
        sc[j], lo[j], hi[j] = True, LO, HI
        R[:, j] = col
        cols[g] = j
    return Case(kind, N, R.astype(np.int64), sc, lo, hi, None, alpha, True, cols)


@functools.lru_cache(maxsize=None)
def reference(kind, N):
    """OracleCPU's result of one case, flat (golden_cases.flat_result), computed once and read only."""
    from oracle.pcx_oracle import OracleCPU

    ref = G.flat_result(OracleCPU(**case(kind, N).oracle_kw()).consensus())
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference_filled(kind, N):
    """OracleCPU.interpolate alone (phase 1: not poisoned by another column's NaN fill)."""
    from oracle.pcx_oracle import OracleCPU

    o = OracleCPU(**case(kind, N).oracle_kw())
    F = np.asarray(o.interpolate(o.reports), dtype=np.float64)
    F.setflags(write=False)
    return F


# ---------------------------------------------------------------- what the reference did with them
def rescaled(c, j):
    """The column as phase 1 sees it: (x - lo) / (hi - lo), truncated in an integer matrix; NaN = missing."""
    x = (np.asarray(c.R[:, j], dtype=np.float64) - c.lo[j]) / float(c.hi[j] - c.lo[j])
    if c.int_dtype:
        x = np.trunc(x)
    return np.where(np.isnan(x) | (x == 0.0), np.nan, x)


def column_pairs(c, ref, j):
    """(values, weights) of column j's two medians: phase 1 (:287-303) and phase 2 (:520-523)."""
    x = rescaled(c, j)
    present = ~np.isnan(x)
    r = ref["agents.old_rep"][present]
    with np.errstate(all="ignore"):
        w1 = r / (np.cumsum(r)[-1] if r.size else 0)
    return (x[present], w1), (ref["filled"][:, j], ref["agents.smooth_rep"])


def fill_of(c, ref, j):
    """The value the reference filled column j's missing cells with (None: nothing was missing)."""
    miss = np.isnan(rescaled(c, j))
    if not miss.any():
        return None
    v = ref["filled"][miss, j]
    assert np.all(bits_equal(v, v[0])), "a column has one fill"
    return float(v[0])


def bits_equal(a, b):
    """Bit for bit, NaNs matching NaNs (tall_cases.bits_equal)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def model_passes(keys, median_key):
    """Histogram passes of the selection's narrowing (k_sel_range, shift_for, k_sel_step) over a set of
    keys whose median is known: a pass bins [lo, hi] into 256 buckets of 2^shift keys, shift =
    bits(hi - lo) - 8, and keeps the extreme keys of the bucket holding the median; a one-key bucket ends."""
    keys = np.array(sorted(set(keys)), dtype=object)
    lo, hi, n = keys[0], keys[-1], 0
    while True:
        n += 1
        bits = (hi - lo).bit_length()
        sh = bits - 8 if bits > 8 else 0
        b = (median_key - lo) >> sh
        inside = [k for k in keys if lo <= k <= hi and (k - lo) >> sh == b]
        if inside[0] == inside[-1]:
            return n
        lo, hi = inside[0], inside[-1]


def deep_bits(c, j):
    """bits(hi - lo) of the deep column's first pass."""
    x = rescaled(c, j)
    x = x[~np.isnan(x)]
    return (dkey(x.max()) - dkey(x.min())).bit_length()


def deep_min_passes(c, j):
    """ceil(bits / 8): a pass over a range of b > 8 bits keeps one bucket of 2^(b - 8) keys, so it narrows
    by at least 8 bits; the deep column's keys M +- 2^e put one of M +- 2^(b - 9) into the bucket of M
    (its half-width), so every pass narrows by exactly 8, and the pass whose range has <= 8 bits ends with
    one-key buckets: 62 -> 54 -> ... -> 6 is 8 = ceil(62 / 8) passes in each phase."""
    return -(-deep_bits(c, j) // 8)


def preconditions(c, ref):
    """What each group was made for shows in the reference's own outputs."""
    raw, fin = ref["events.outcomes_raw"], ref["events.outcomes_final"]
    old, smooth = ref["agents.old_rep"], ref["agents.smooth_rep"]
    first = E - len(c.cols)
    assert np.count_nonzero(~c.sc[:first]) >= 8
    assert all(c.sc[j] and c.lo[j] == LO and c.hi[j] == HI for j in c.crafted)
    if c.kind in TIE_KINDS:  # alpha = 0.0: the outcome medians weigh old_rep itself
        assert np.array_equal(smooth.view(np.uint64), old.view(np.uint64))
    if c.kind in NAN_KINDS:  # one NaN fill: every reputation and outcome is NaN
        assert np.isnan(smooth).all() and np.isnan(raw[c.sc]).all()
    else:
        assert np.isfinite(smooth).all() and np.isfinite(raw).all()
    if KINDS[c.kind][0] == "integer":
        assert np.all(old[::ZERO_EVERY] == 0.0) and np.count_nonzero(old == 0.0) == len(old[::ZERO_EVERY])
    if c.kind == "negative":
        assert 0.05 * c.N < np.count_nonzero(old < 0.0) < 0.15 * c.N
    if c.kind == "constant":
        assert len(set(old.tolist())) == 1
    for g, j in c.cols.items():
        x = rescaled(c, j)
        present = x[~np.isnan(x)]
        fill = fill_of(c, ref, j)
        nan_kind = c.kind in NAN_KINDS
        if g in ("duplicates", "negative-weights", "duplicates-int"):
            vals = {k / 8.0 for k in range(1, 8)} if not c.int_dtype else {float(k) for k in range(1, 8)}
            assert set(present.tolist()) == vals and fill in vals and (nan_kind or raw[j] in vals), (g, fill, raw[j])
        elif g == "zeros-sprinkled":
            assert old[0] == 0.0 and old[ZERO_EVERY] == 0.0
            assert x[0] == present.min() and x[ZERO_EVERY] == present.max()
            assert np.count_nonzero(present == x[0]) == 1 and np.count_nonzero(present == x[ZERO_EVERY]) == 1
            assert fill in {k / 8.0 for k in range(1, 8)}
        elif g == "one-present-last-rank":
            r = _last_rank_row(c.N)
            assert len(present) == 1 and x[r] == 0.5 and r >= c.N - c.N // 3 and old[r] > 0.0
            assert fill == 0.5 and (nan_kind or (raw[j] == 0.5 and fin[j] == 4.0))
        elif g == "constant":
            assert set(present.tolist()) == {0.375} and fill == 0.375 and (nan_kind or raw[j] == 0.375)
        elif g == "no-missing":
            assert fill is None and len(set(present.tolist())) == c.N
        elif g == "fill-equals-present":
            assert fill in set(present.tolist()) and (nan_kind or raw[j] == fill), (fill, raw[j])
        elif g == "deep":
            below, above = deep_keys()
            want = {float(np.uint64(b).view(np.float64)) for b in below + above} | {0.5}
            assert set(present.tolist()) == want
            assert deep_bits(c, j) == 62 and deep_min_passes(c, j) == 8 <= MAX_SEL_PASSES
            assert fill == 0.5 and (nan_kind or raw[j] == 0.5), (fill, raw[j])
            # the model of the narrowing takes exactly that many passes in either phase (the fill is a
            # present value: phase 2 walks the same keys)
            assert model_passes([dkey(v) for v in present], dkey(0.5)) == 8
        elif g in ("tie-count-far", "tie-count-ulp"):
            s = np.sort(present)
            n = len(s)
            a, b = (0.25, 0.75) if g == "tie-count-far" else (0.625, float(np.nextafter(0.625, 1.0)))
            assert n % 2 == 0 and s[n // 2 - 1] == a and s[n // 2] == b
            assert fill == (a + b) / 2.0, (g, fill)
            assert len(set(present.tolist())) == n
        elif g == "tie-weights":
            assert fill == 0.5 and raw[j] == 0.5 and fin[j] == 4.0, (fill, raw[j], fin[j])
            w = old[~np.isnan(x)]
            assert len(set(w.tolist())) > 1  # unequal weights: the weight walk, not the equal-weight count
            assert 2 * sum(Fraction(v) for v in w[present == 0.25]) == sum(Fraction(v) for v in w)
        elif g == "tie-above":
            # exactly, the weight at 0.25 is MORE than half (by ~1e-17 of it): the crossing bucket is the
            # first one and its upper prefix is the one near the half; the reference's float walk does
            # not stop there (it walks on: the average 0.5 on the half test, or 0.75 past it)
            w = old[~np.isnan(x)]
            low, tot = sum(Fraction(v) for v in w[present == 0.25]), sum(Fraction(v) for v in w)
            assert 0 < 2 * low - tot < Fraction(1, 10 ** 15) * tot
            assert fill in (0.5, 0.75), fill
        elif g == "dominant":
            d = dominant_row(c.kind, c.N)
            assert old[d] > 0.5 and smooth[d] > 0.5 and x[d] == 0.375
            assert fill == 0.375 and raw[j] == 0.375 and fin[j] == 3.0, (fill, raw[j])
        elif g == "dominant-missing":
            d = dominant_row(c.kind, c.N)
            assert np.isnan(x[d]) and fill in {k / 8.0 for k in range(1, 8)} and raw[j] == fill
        elif g in ("zero-weight-only", "all-missing"):
            assert np.isnan(fill)
            if g == "zero-weight-only":
                assert len(present) == 3 and np.all(old[~np.isnan(x)] == 0.0)
            else:
                assert len(present) == 0
        elif g == "fill-truncated":
            s = np.sort(present)
            n = len(s)
            assert n % 2 == 0 and s[n // 2 - 1] == 1.0 and s[n // 2] == 2.0 and fill == 1.0, fill
        else:
            raise KeyError(g)
    if c.kind in ("dominant-r0", "dominant-rlast"):
        d = dominant_row(c.kind, c.N)
        assert (d < c.N // 3) if c.kind == "dominant-r0" else (d >= c.N - c.N // 3)


def stability(c, ref, seeds=(1, 2)):
    """Every crafted column's outcome median is unchanged when its weights move by +-1e-12 relative
    (so the last bits of the GPU's smooth_rep cannot decide it).  Returns the columns checked."""
    from oracle.pcx_oracle import weighted_median

    assert c.kind not in TIE_KINDS
    smooth = ref["agents.smooth_rep"]
    for seed in seeds:
        sign = np.random.default_rng(seed).choice([-1.0, 1.0], c.N)
        w = smooth * (1.0 + 1e-12 * sign)
        for g, j in c.cols.items():
            m = weighted_median(ref["filled"][:, j], w)
            m = np.nan if m is None else m
            assert bits_equal(m, ref["events.outcomes_raw"][j]), (c.kind, g, seed, m, ref["events.outcomes_raw"][j])
    return c.crafted


# ---------------------------------------------------------------- weightedstats, word for word
def weightedstats_weighted_median(data, weights):
    """weightedstats.weighted_median(data, weights) as published (the reference imports it at
    __init__.py:44 and calls it at :303 and :520-523; the package is not vendored -- this is the text
    tests/golden/make_golden.py injects to produce the golden vectors), on Python lists."""
    midpoint = 0.5 * sum(weights)
    if any([j > midpoint for j in weights]):
        return data[weights.index(max(weights))]
    if any([j > 0 for j in weights]):
        sorted_data, sorted_weights = zip(*sorted(zip(data, weights)))
        cumulative_weight = 0
        below_midpoint_index = 0
        while cumulative_weight <= midpoint:
            below_midpoint_index += 1
            cumulative_weight += sorted_weights[below_midpoint_index - 1]
        cumulative_weight -= sorted_weights[below_midpoint_index - 1]
        if abs(cumulative_weight - midpoint) < sys.float_info.epsilon:
            bounds = sorted_data[below_midpoint_index - 2:below_midpoint_index]
            return sum(bounds) / float(len(bounds))
        return sorted_data[below_midpoint_index - 1]
    return None
