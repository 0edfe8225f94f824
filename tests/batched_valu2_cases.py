"""Crafted 50 x 20 batches for the compiled batched kernel (csrc/pcx_batched.hip, csrc/pcx_batched_round.inc):
old = np.dot(rep, F) formed as the third vector of the n1 / n2 pass (`OLD3`), the covariance's divisions
through one reciprocal of the token sum (`div_rn`, csrc/pcx_fastdiv.h) and the normalisations' square
roots without the range scaling (`sqrt_uniform`); and for the interpolation medians' prescreen
(`wave_wmedian_screen`), whose tail rows, reputations of -0.0 and of a wide range, and counts of medians
per round no other file places (a below-sum form taken four rows per statement under the compare's
lane mask was built against them, measured slower and is not in the source: DESIGN.md 5.2).
Builders only: the tests are test_batched_valu2_cpu.py and test_batched_valu2_gpu.py.

Every batch is B = 256 rounds of 50 x 20 (the two controls on the dynamic kernels: 6 x 4 and 50 x 21);
the six prescreen kinds of interp_prescreen_cases.py come as they are there, 32 rounds each.
batch(name) returns (reports, keyword arguments of OC.batched / consensus_batched, the C oracle's
outputs), computed once per session.
"""
import functools

import numpy as np

import interp_prescreen_cases as IP

B, N, E = 256, 50, 20
IP_KINDS = ("plain", "ties", "signed", "collision", "near_half", "exact_half")
PAIRINGS = ((7,), (4, 5), (2, 3, 17), (0, 1, 9, 18, 19))  # 1, 2, 3 and 5 interpolation medians
TIE_SEED = 902  # synthetic.rounds(256, 50, 20): the oracle reports branch 3 or 4 in 10 rounds (chosen on the CPU)
BIG = 2.0 ** 80

PRESCREEN = ("tail_only_present", "tail_only_missing", "tail_median", "minus_zero_rep", "wide_rep", "negative_rep",
             "no_rep", "median_counts")
OLD = ("old_pca", "old_absolute", "old_cokurtosis", "old_no_rep", "old_int", "old_ties")
CONTROLS = ("control_6x4", "control_50x21")
COV = ("cov_agreed_column", "cov_denom_zero", "cov_denom_negative", "cov_synthetic")
SQRT = ("sqrt_unscaled", "sqrt_2m233", "sqrt_2m260")
NAMES = PRESCREEN + OLD + CONTROLS + COV + SQRT


def _base(seed, scaled_cols, na_frac=0.0, rep_range=(1, 100)):
    """B rounds whose scaled events are `scaled_cols` (one tuple, or one per round: round b takes entry
    b % len), synthetic's reports and integer reputations."""
    from pyconsensus_amd import synthetic

    rng = np.random.default_rng(seed)
    pats = scaled_cols if scaled_cols and isinstance(scaled_cols[0], tuple) else (tuple(scaled_cols),)
    sc = np.zeros((B, E), bool)
    for b in range(B):
        sc[b, list(pats[b % len(pats)])] = True
    lo = np.where(sc, rng.uniform(-100.0, 0.0, (B, E)), 1.0)
    hi = np.where(sc, lo + rng.uniform(1.0, 200.0, (B, E)), 2.0)
    truth = rng.integers(1, 3, (B, E)).astype(np.float64)
    R = synthetic._reports(rng, sc, lo, hi, truth, N, na_frac)
    rep = rng.integers(rep_range[0], rep_range[1], (B, N)).astype(np.float64)
    return rng, R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi)


def _synthetic(seed, n=N, e=E, **extra):
    from pyconsensus_amd import synthetic

    R, sc, lo, hi, rep = synthetic.rounds(B, n, e, seed=seed)
    return R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi, **extra)


def _binary(seed):
    """Binary reports with no missing cell, integer reputations."""
    rng = np.random.default_rng(seed)
    R = rng.integers(1, 3, (B, N, E)).astype(np.float64)
    return R, dict(reputation=rng.integers(1, 100, (B, N)).astype(np.float64))


def _tail_median(rng, R, kw):
    """Column 0 (bounds (0, 1): the rescale is the identity): three missing rows among 0..47, and the
    weighted median's value 0.5 in row 48 (even rounds) or 49 (odd), the rows below it and above it
    holding less than half the weight each."""
    kw["scaled"][:, 0], kw["lo"][:, 0], kw["hi"][:, 0] = True, 0.0, 1.0
    rep = kw["reputation"]
    for b in range(B):
        cross = 48 + b % 2
        head = rng.permutation(48)
        miss = head[:3]
        rest = rng.permutation(np.append(head[3:], 97 - cross))  # (the other of rows 48, 49 stays present)
        low, high = rest[:23], rest[23:]
        R[b, low, 0] = rng.uniform(0.1, 0.3, len(low))
        R[b, high, 0] = rng.uniform(0.7, 0.9, len(high))
        R[b, cross, 0] = 0.5
        R[b, miss, 0] = np.nan
        rep[b] = rng.integers(1, 10, N)
        p = ~np.isnan(R[b, :, 0])
        rep[b, cross] = abs(rep[b, p & (R[b, :, 0] < 0.5)].sum() - rep[b, p & (R[b, :, 0] > 0.5)].sum()) + 4.0


def build(name):
    """(reports, keyword arguments) of one batch."""
    if name == "tail_only_present":  # column 4: rows 48 and 49 the only present ones
        rng, R, kw = _base(701, (4, 13))
        R[:, :48, 4] = np.nan
        rep = kw["reputation"]  # (equal weights would put the running sum on half: the mean of the two)
        rep[:, 49] = np.where(rep[:, 49] == rep[:, 48], rep[:, 49] + 1.0, rep[:, 49])
    elif name == "tail_only_missing":  # column 4: rows 48 and 49 the only missing ones
        rng, R, kw = _base(702, (4, 13))
        R[:, 48:, 4] = np.nan
    elif name == "tail_median":
        rng, R, kw = _base(703, (0, 13))
        _tail_median(rng, R, kw)
    elif name == "minus_zero_rep":  # one reporter per round with a reputation of -0.0, present in the medians' columns
        rng, R, kw = _base(704, (4, 5, 13), na_frac=0.1)
        z = rng.integers(0, N, B)
        kw["reputation"][np.arange(B), z] = -0.0
        for j in (4, 5, 13):
            fresh = kw["lo"][:, j] + 0.37 * (kw["hi"][:, j] - kw["lo"][:, j])
            R[np.arange(B), z, j] = np.where(np.isnan(R[np.arange(B), z, j]), fresh, R[np.arange(B), z, j])
    elif name == "wide_rep":  # reputations from 2^-90 to 2^90
        rng, R, kw = _base(705, (4, 5, 13), na_frac=0.1)
        kw["reputation"] = 2.0 ** rng.integers(-90, 91, (B, N)).astype(np.float64)
        kw["reputation"][:, 0], kw["reputation"][:, 1] = 2.0 ** -90, 2.0 ** 90
    elif name == "negative_rep":
        rng, R, kw = _base(706, (4, 5, 13, 19), na_frac=0.1)
        kw["reputation"][:, 3] = -2.0
    elif name == "no_rep":
        rng, R, kw = _base(707, (4, 5, 13, 19), na_frac=0.1)
        kw["reputation"] = None
    elif name == "median_counts":  # round b: PAIRINGS[b % 4] are its scaled columns with missing reports
        pats = tuple(p + ((10,) if 10 not in p else (11,)) for p in PAIRINGS)
        rng, R, kw = _base(708, pats)
        for b in range(B):
            for j in PAIRINGS[b % len(PAIRINGS)]:
                R[b, rng.choice(N, 5, replace=False), j] = np.nan
    elif name == "old_pca":
        R, kw = _synthetic(711)
    elif name == "old_absolute":
        R, kw = _synthetic(712, algorithm="absolute")
    elif name == "old_cokurtosis":
        R, kw = _synthetic(713, algorithm="cokurtosis")
        kw["aux_scores"] = np.random.default_rng(713).normal(size=(B, N))
    elif name == "old_no_rep":
        R, kw = _synthetic(714)
        kw["reputation"] = None
    elif name == "old_int":
        R, kw = _synthetic(715, int_dtype=True)
    elif name == "old_ties":
        R, kw = _synthetic(TIE_SEED)
    elif name == "control_6x4":
        R, kw = _synthetic(716, 6, 4)
    elif name == "control_50x21":
        R, kw = _synthetic(717, 50, 21)
    elif name == "cov_agreed_column":  # binary column 6: every reporter files the same report, none missing
        rng, R, kw = _base(721, (3, 12), na_frac=0.05)
        R[:, :, 6] = rng.integers(1, 3, (B, 1)).astype(np.float64)
        # reputations k / 64: every partial sum of the weighted mean is exact, so the column's mean is its
        # value, its centred reports are zeros and its covariance entries exact zeros
        kw["reputation"] = np.ones((B, N))
        kw["reputation"][:, 0] = 64.0 - (N - 1)
    elif name in ("cov_denom_zero", "cov_denom_negative"):
        # Raw reputations 2^80 and -2^80 in rows 0 and 16 cancel exactly in numpy's pairwise total (one
        # accumulator, consecutive terms), which is 10^6: rows 1 and 33 hold it.  The two large tokens
        # absorb every other token of lanes 0..31 in the SPEC's tree sum and cancel, so the token sum is
        # row 33's token alone: int(1.5e-6 * 1e6) = 1 and denom = 0, or int(0.5e-6 * 1e6) = 0 and denom = -1.
        rng, R, kw = _base(722, (3, 12))  # (no missing report: these reputations are no subject for the fill)
        small = 1.5 if name == "cov_denom_zero" else 0.5
        rep = np.zeros((B, N))
        rep[:, 0], rep[:, 16], rep[:, 1], rep[:, 33] = BIG, -BIG, 1e6 - small, small
        kw["reputation"] = rep
    elif name == "cov_synthetic":
        R, kw = _synthetic(20261015)
    elif name == "sqrt_unscaled":
        R, kw = _binary(731)
    elif name == "sqrt_2m233":
        R, kw = _binary(731)
        R = R * 2.0 ** -233
    elif name == "sqrt_2m260":
        R, kw = _binary(731)
        R = R * 2.0 ** -260
    else:
        raise KeyError(name)
    return R, kw


@functools.lru_cache(maxsize=None)
def batch(name):
    """(reports, keyword arguments, the C oracle's outputs) of a batch, computed once."""
    if name in IP_KINDS:
        return IP.batch(name, N, E)
    from oracle import pcx_oracle_c as OC

    R, kw = build(name)
    return R, kw, OC.batched(R, **kw, threads=8)


def missing(c):
    """[B][N][E]: the report is NaN or zero after the rescale (the oracle's `original`)."""
    o = c["original"]
    return np.isnan(o) | (o == 0.0)


def check(name):
    """Assert on the ORACLE's own outputs that the batch is what it claims to be (CPU only)."""
    R, kw, c = batch(name)
    sc = None if kw.get("scaled") is None else np.asarray(kw["scaled"]).astype(bool)
    miss, o, f, r = missing(c), c["original"], c["filled"], c["old_rep"]
    n_med = (miss.any(axis=1) & sc).sum(1) if sc is not None else np.zeros(len(R), int)
    if name in IP_KINDS:
        has, d2, _ = IP.restate(c, sc, 2.0)
        _, dh, _ = IP.restate(c, sc, 0.5)
        if name in IP.CRAFTED or name == "exact_half":
            has, d2, dh = has[:, :1], d2[:, :1], dh[:, :1]
        rounds = np.count_nonzero(d2.any(axis=1)) if name in ("plain", "ties", "signed") else \
            np.count_nonzero((has & ~dh).any(axis=1))
        assert rounds >= 8, (name, rounds)
    elif name == "tail_only_present":
        assert np.all(miss[:, :48, 4]) and not miss[:, 48:, 4].any()
        fill = f[:, 0, 4]
        assert np.all((fill == o[:, 48, 4]) | (fill == o[:, 49, 4])), "the median is row 48's or row 49's report"
        assert np.any(fill == o[:, 48, 4]) and np.any(fill == o[:, 49, 4])
    elif name == "tail_only_missing":
        assert not miss[:, :48, 4].any() and np.all(miss[:, 48:, 4])
        _, d2, _ = IP.restate(c, sc, 2.0)
        assert np.count_nonzero(d2[:, 4]) > 0.9 * B, "the prescreen decides nearly all of them"
    elif name == "tail_median":
        assert not miss[:, 48:, 0].any() and np.all(miss[:, :48, 0].sum(1) == 3)
        assert np.all(o[np.arange(B), 48 + np.arange(B) % 2, 0] == 0.5)
        assert np.all(f[:, :, 0][miss[:, :, 0]] == 0.5), "the median is row 48's / 49's report"
        _, d2, _ = IP.restate(c, sc, 2.0)
        assert np.count_nonzero(d2[:, 0]) > 0.9 * B
    elif name == "minus_zero_rep":
        z = (r == 0.0) & np.signbit(r)
        assert np.all(z.sum(1) == 1) and np.all(r >= 0.0), "-0.0 passes the prescreen's rep >= 0"
        assert np.all(n_med >= 1)
        zrow = z.argmax(1)
        assert not miss[np.arange(B), zrow][:, [4, 5, 13]].any(), "the -0.0 row is present in the medians' columns"
        _, d2, _ = IP.restate(c, sc, 2.0)
        assert np.count_nonzero(d2) > 0.5 * n_med.sum()
    elif name == "wide_rep":
        assert np.all(r.max(1) / r.min(1) >= 2.0 ** 150) and np.all(r > 0.0) and np.all(n_med >= 1)
    elif name == "negative_rep":
        assert np.all(r.min(1) < 0.0) and np.all(n_med >= 1)
    elif name == "no_rep":
        assert np.all(r == 1.0 / N) and np.all(n_med >= 1)
    elif name == "median_counts":
        assert np.array_equal(n_med, np.array([len(PAIRINGS[b % len(PAIRINGS)]) for b in range(B)]))
        assert set(n_med) == {1, 2, 3, 5}
        has, d2, _ = IP.restate(c, sc, 2.0)
        assert np.count_nonzero(d2) > 0.9 * np.count_nonzero(has)
    elif name in OLD:
        br = np.bincount(c["branch"], minlength=6)
        if name == "old_absolute":
            assert br[5] == B, "absolute never reaches the nonconformity block"
        elif name == "old_cokurtosis":
            assert br[3] + br[4] == B and br[3] and br[4], "a caller-scored round goes straight to d - old"
        else:
            assert br[1] and br[2] and br[1] + br[2] + br[3] + br[4] == B
        if name == "old_ties":
            assert br[3] + br[4] >= 8, "the rank rule ties in at least 8 rounds"
        if name == "old_no_rep":
            assert np.all(r == 1.0 / N)
        if name == "old_int":
            assert np.all(o[~np.isnan(o)] == np.trunc(o[~np.isnan(o)]))
    elif name in CONTROLS:
        assert R.shape[1:] == ((6, 4) if name == "control_6x4" else (50, 21))
    elif name == "cov_agreed_column":
        assert not miss[:, :, 6].any() and np.all(f[:, :, 6] == f[:, :1, 6])
        assert np.all(c["adj_first_loadings"][:, 6] == 0.0) and np.all(c["flags"] == 0)
        assert np.all(c["certainty"][:, 6] > 0.99)
    elif name == "cov_denom_zero":
        assert np.all(r[:, 33] == 1.5e-6) and np.all(np.trunc(r[:, 33] * 1e6) == 1.0)
        assert np.all(c["flags"] == 2), "every covariance entry is a quotient by zero: not finite"
        assert np.all(c["pi_iters"] == 0)
    elif name == "cov_denom_negative":
        assert np.all(r[:, 33] == 0.5e-6) and np.all(np.trunc(r[:, 33] * 1e6) == 0.0)
        assert np.count_nonzero(c["flags"] == 0) > 0.8 * B and np.all((c["flags"] == 0) | (c["flags"] == 2))
        assert np.all(c["pi_iters"][c["flags"] == 0] > 0)
    elif name == "cov_synthetic":
        assert np.all(c["flags"] == 0)
    elif name in SQRT:
        _, _, c0 = batch("sqrt_unscaled")
        assert not miss.any() and np.all(c["flags"] == 0)
        assert np.array_equal(c["pi_iters"], c0["pi_iters"]) and c0["pi_iters"].min() >= 9
        top = np.log2(np.abs(c["scores"]).max(1))
        k = {"sqrt_unscaled": 0, "sqrt_2m233": 233, "sqrt_2m260": 260}[name]
        # scores ~ 2^(2 - k): the covariance's columns ~ 2^(-2 k), their sums of squares ~ 2^(-4 k), which is
        # normal and below 2^-767 at k = 233 (2^-932) and subnormal at k = 260 (2^-1040)
        assert np.all(np.abs(top + k) < 4.0), (name, top.min(), top.max())
    else:
        raise KeyError(name)
