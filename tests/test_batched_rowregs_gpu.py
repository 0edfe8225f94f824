"""The compiled 50 x 20 batched kernel's column loops over a register-held row (csrc/pcx_batched_round.inc,
`ROWREG`): the rescale and the NA masks, whose per-lane missing bits the fill reads and whose per-column
masks the guesses and the interpolation medians read, and the certainty's hit masks.

Every case is 256 rounds of 50 x 20, compared bit for bit on every output (`original`, `filled`,
`nas_filled` and `na_row` included) with the C oracle, after asserting on the ORACLE's own outputs that
the case is what it claims to be:

* column extremes: every event scaled, none, scaled events only at columns 0 and 19, and only at 15 and
  16 (the ends and the seam of the 16-byte row reads);
* missing patterns: a column missing in every row but one, a reporter with every report missing, missing
  reports only in rows 48 and 49, and none at all;
* zeros: reports that rescale to 0.0 (equal to `lo`) and -0.0 in a binary column, also with int_dtype;
* interpolation medians: rounds with exactly 1, 2, 3 and 5 scaled columns that have missing reports
  (adjacent and far apart), two adjacent columns of which the prescreen refuses the first and decides
  the second, and the reverse, and rounds with a negative reputation;
* certainty: a column every reporter agrees with, one none agrees with, and columns with exactly 8 and
  exactly 9 hits;
* controls on the dynamic kernels (6 x 4 and 50 x 21).
"""
import numpy as np
import pytest

import interp_prescreen_cases as IP
from test_batched_pi_gpu import _assert_bitexact, _np

B, N, E = 256, 50, 20


def base(seed, scaled_cols, na_frac=0.0, rep_range=(1, 100)):
    """B rounds whose scaled events are `scaled_cols` (one tuple, or one per round: round b takes entry
    b % len), synthetic.rounds' reports and integer reputations."""
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


def _oracle(R, kw):
    from oracle import pcx_oracle_c as OC

    return OC.batched(R, **kw, threads=8)


def _compare(R, kw, c, what):
    from pyconsensus_amd.batched import consensus_batched

    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    assert {"original", "filled", "nas_filled", "na_row"} <= set(g)
    _assert_bitexact(g, c, what)
    return g


def _missing(c):
    """[B][N][E]: the report is NaN or zero after the rescale (the oracle's `original`)."""
    o = c["original"]
    return np.isnan(o) | (o == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [tuple(range(E)), (), (0, 19), (15, 16)], ids=["all", "none", "0_19", "15_16"])
def test_scaled_column_extremes(gpu_lib, cols):
    _, R, kw = base(601 + len(cols) + sum(cols), cols, na_frac=0.1)
    c = _oracle(R, kw)
    pres = ~np.isnan(R)
    rescaled = (c["original"] != R) & pres
    assert np.all(rescaled.any(axis=(0, 1)) == np.isin(np.arange(E), cols)), "exactly the scaled columns are rescaled"
    assert _missing(c)[:, :, list(cols)].any() or not cols
    _compare(R, kw, c, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["column_but_one", "reporter", "rows_48_49", "none"])
def test_missing_patterns(gpu_lib, case):
    rng, R, kw = base(620 + len(case), (3, 12, 19), na_frac=0.1 if case == "reporter" else 0.0)
    if case == "column_but_one":
        for j in (3, 7):  # a scaled and a binary column
            keep = rng.integers(0, N, B)
            m = np.ones((B, N), bool)
            m[np.arange(B), keep] = False
            R[:, :, j] = np.where(m, np.nan, R[:, :, j])
    elif case == "reporter":
        R[:, 5, :] = np.nan
        R[:, 49, :] = np.nan
    elif case == "rows_48_49":
        R[:, 48:50, :] = np.where(rng.random((B, 2, E)) < 0.5, np.nan, R[:, 48:50, :])
    c = _oracle(R, kw)
    miss = _missing(c)
    if case == "column_but_one":
        assert np.all(miss[:, :, 3].sum(1) == N - 1) and np.all(miss[:, :, 7].sum(1) == N - 1)
    elif case == "reporter":
        assert np.all(np.isnan(c["original"][:, 5, :])) and np.all(np.isnan(c["original"][:, 49, :]))
        assert np.all(c["participation_rows"][:, 5] == 1.0) and np.all(c["na_row"][:, 5] == 0.0)
    elif case == "rows_48_49":
        assert not miss[:, :48, :].any() and np.all(miss[:, 48:, :].any(axis=(1, 2)))
        assert miss[:, 48:, :][:, :, [3, 12, 19]].any(axis=1).sum() > B, "interpolation medians among them"
    else:
        assert not miss.any() and np.all(c["nas_filled"] == 0.0) and np.all(c["na_row"] == 0.0)
        assert np.array_equal(c["filled"], c["original"])
    _compare(R, kw, c, case)


@pytest.mark.gpu
@pytest.mark.parametrize("int_dtype", [False, True], ids=["f64", "int"])
def test_reports_that_rescale_to_zero(gpu_lib, int_dtype):
    rng, R, kw = base(640, (0, 15, 16, 19))
    lo = kw["lo"]
    zs = np.zeros((B, N, E), bool)
    for j in (0, 16, 19):  # scaled: a report equal to lo rescales to exactly +0.0
        zs[:, :, j] = rng.random((B, N)) < 0.08
        R[:, :, j] = np.where(zs[:, :, j], lo[:, j][:, None], R[:, :, j])
    for j in (1, 18):      # binary: -0.0 stays -0.0
        zs[:, :, j] = rng.random((B, N)) < 0.08
        R[:, :, j] = np.where(zs[:, :, j], -0.0, R[:, :, j])
    kw["int_dtype"] = int_dtype
    c = _oracle(R, kw)
    o = c["original"]
    if not int_dtype:
        assert np.all(o[zs] == 0.0) and np.count_nonzero(np.signbit(o[zs])) > B and np.count_nonzero(~np.signbit(o[zs])) > B
        assert np.array_equal(c["nas_filled"], zs.sum(1).astype(np.float64)), "the column counts are the zeros placed"
        assert np.array_equal(c["na_row"], zs.sum(2).astype(np.float64)), "and the row counts"
    else:  # (truncation sends every rescaled report below 1 to zero as well)
        assert np.all(o[zs] == 0.0) and np.all(c["nas_filled"] >= zs.sum(1)) and np.all(c["na_row"] >= zs.sum(2))
    assert np.array_equal(c["nas_filled"], (o == 0.0).sum(1).astype(np.float64))
    assert np.array_equal(c["na_row"], (o == 0.0).sum(2).astype(np.float64))
    _compare(R, kw, c, "zeros")


PAIRINGS = ((7,), (4, 5), (0, 19), (2, 3, 17), (0, 1, 9, 18, 19))


def _knock_out(rng, R, b, j, k=5):
    R[b, rng.choice(N, k, replace=False), j] = np.nan


@pytest.mark.gpu
def test_median_pass_counts(gpu_lib):
    """Round b has PAIRINGS[b % 5] as its scaled columns with missing reports (and a scaled column 10
    or 11 without any): 1, 2, 2, 3 and 5 interpolation medians -- a lone column, two adjacent and two
    far apart, three, and five with both ends of the row among them."""
    pats = tuple(p + ((10,) if 10 not in p else (11,)) for p in PAIRINGS)
    rng, R, kw = base(660, pats)
    for b in range(B):
        for j in PAIRINGS[b % 5]:
            _knock_out(rng, R, b, j)
    c = _oracle(R, kw)
    n_med = (_missing(c).any(axis=1) & kw["scaled"]).sum(1)
    assert np.array_equal(n_med, np.array([len(PAIRINGS[b % 5]) for b in range(B)]))
    assert np.all(kw["scaled"].sum(1) == n_med + 1)
    # the prescreen decides nearly all of them (restated on the oracle's outputs at twice the margin)
    has, dec, _ = IP.restate(c, kw["scaled"], 2.0)
    assert np.array_equal(has.sum(1), n_med) and np.count_nonzero(dec) > 0.9 * np.count_nonzero(has)
    _compare(R, kw, c, "pairings")


@pytest.mark.gpu
@pytest.mark.parametrize("refused", ["first", "second"])
def test_pair_with_one_column_refused(gpu_lib, refused):
    """Columns 4 and 5 go through the prescreen one after the other.  One reporter holds three quarters of the
    reputation: present in the refused column (the SPEC's dominant-weight exit, which the prescreen
    leaves to the sort: the fill is that reporter's own report) and missing in the other, whose median
    the prescreen decides."""
    rng, R, kw = base(670 + len(refused), (4, 5, 13))
    A, Bc = (4, 5) if refused == "first" else (5, 4)
    dom = rng.integers(0, N, B)
    rep = kw["reputation"]
    for b in range(B):
        rows = np.delete(np.arange(N), dom[b])
        R[b, rng.choice(rows, 5, replace=False), A] = np.nan
        R[b, rng.choice(rows, 4, replace=False), Bc] = np.nan
        R[b, dom[b], Bc] = np.nan
        pres = np.flatnonzero(~np.isnan(R[b, :, Bc]))
        if rep[b, pres].sum() % 2 == 0:  # an odd integer total: no sum of present reputations lies on half
            rep[b, pres[0]] += 1.0
        rep[b, dom[b]] = 3.0 * (rep[b].sum() - rep[b, dom[b]])
    c = _oracle(R, kw)
    o, f, r = c["original"], c["filled"], c["old_rep"]
    for b in range(B):
        assert not IP.screen_decides(o[b, :, A], r[b], 0.5)[0], "refused even at half the margin"
        assert IP.screen_decides(o[b, :, Bc], r[b], 2.0)[0], "decided even at twice the margin"
        mA = np.isnan(o[b, :, A])
        assert mA.sum() == 5 and np.all(f[b, mA, A] == o[b, dom[b], A]), "the dominant reporter's report fills"
        mB = np.isnan(o[b, :, Bc])
        assert mB.sum() == 5 and np.all(f[b, mB, Bc] == IP.screen_decides(o[b, :, Bc], r[b], 2.0)[1])
    _compare(R, kw, c, refused)


@pytest.mark.gpu
def test_negative_reputation_rounds_do_not_prescreen(gpu_lib):
    rng, R, kw = base(680, (4, 5, 13, 19))
    for b in range(B):
        for j in (4, 5, 19):
            _knock_out(rng, R, b, j)
    kw["reputation"][::2, 3] = -2.0
    c = _oracle(R, kw)
    assert np.all(c["old_rep"][::2].min(1) < 0.0) and np.all(c["old_rep"][1::2].min(1) > 0.0)
    assert np.all((_missing(c).any(axis=1) & kw["scaled"]).sum(1) == 3)
    _compare(R, kw, c, "negative")


@pytest.mark.gpu
def test_certainty_hit_counts(gpu_lib):
    """Column 1 (binary): every reporter files the outcome, 50 hits.  Column 6 (binary): the reporters
    split evenly, the outcome is caught at 1.5 and nobody filed that: no hit, certainty NaN.  Columns 2
    and 17 (scaled, bounds (0, 1)): 8 and 9 reporters share the weighted median's value, the others
    are distinct, 21 below and the rest above."""
    rng, R, kw = base(690, (2, 17), rep_range=(50, 60))
    kw["lo"][:, [2, 17]], kw["hi"][:, [2, 17]] = 0.0, 1.0
    R[:, :, 1] = 2.0
    for b in range(B):
        R[b, :, 6] = 1.0 + (rng.permutation(N) < N // 2)
        for j, k in ((2, 8), (17, 9)):
            x = np.concatenate([rng.uniform(0.1, 0.4, 21), np.full(k, 0.5), rng.uniform(0.6, 0.9, N - 21 - k)])
            R[b, :, j] = x[rng.permutation(N)]
    c = _oracle(R, kw)
    hits = (c["filled"] == c["outcomes_adjusted"][:, None, :]).sum(1)
    assert np.all(hits[:, 1] == 50) and np.all(hits[:, 2] == 8) and np.all(hits[:, 17] == 9)
    assert np.all(c["outcomes_adjusted"][:, 6] == 1.5) and np.all(hits[:, 6] == 0)
    assert np.all(np.isnan(c["certainty"][:, 6])) and np.all(c["certainty"][:, 1] > 0.99)
    _compare(R, kw, c, "certainty")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 4), (50, 21)], ids=["6x4", "50x21"])
def test_dynamic_kernels_as_before(gpu_lib, shape):
    from pyconsensus_amd import synthetic

    n, e = shape
    R, sc, lo, hi, rep = synthetic.rounds(B, n, e, seed=607 + e)
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    _compare(R, kw, _oracle(R, kw), shape)
