"""The compiled 50 x 20 batched kernel's in-row broadcasts (csrc/pcx_batched.hip, "broadcasts inside the
16-lane row"): the power iteration keeps its vector as two row-spread registers, columns 0..15 taken
from the first and columns 16..19 from the second by `v_fmac_f64_dpp ... row_newbcast`, and the scores
take the column means and the loading the same way in all four lane rows (reporters 48 and 49 sit in
row 3).

Every case is 256 rounds, compared bit for bit on every output (`pi_iters`, `flags` and `branch`
included) with the C oracle, after asserting on the ORACLE's own outputs that the case is what it
claims to be:

* the variance in events 16..19 (the second register), in events 0..15 (the first), and shared by
  events 15 and 16 (the seam between them);
* loadings that are exactly zero on events 0..15, so that the sign rule reads its first nonzero
  component from a lane of row 1;
* a nearly repeated leading eigenvalue (the loop runs into the in-loop squarings);
* `reputation=None`, and 10 % missing reports: the scores of reporters 48 and 49;
* controls on the dynamic kernels, whose text has no such instruction: 6 x 4 and 50 x 21.
"""
import numpy as np
import pytest

from test_batched_pi_gpu import (ITERS_IN_LOOP_SQUARING, _assert_bitexact, _dyadic_reputation, _np,
                                 check_side_branches, side_rounds)

B, N, E = 256, 50, 20


def crafted_rounds(strong, seed, unanimous=(), dyadic=False):
    """B binary rounds whose variance sits in the events `strong`: a group of 20 reporters (drawn per
    round) files the opposite answer on every strong event and three more reporters flip each strong
    event on their own (no two strong columns are equal); every other event has one dissenter, or
    none if it is in `unanimous`."""
    rng = np.random.default_rng(seed)
    truth = rng.integers(1, 3, (B, 1, E)).astype(np.float64)
    R = np.repeat(truth, N, axis=1)
    flip = np.zeros((B, N, E), bool)
    order = np.argsort(rng.random((B, N)), axis=1)
    group = np.zeros((B, N), bool)
    np.put_along_axis(group, order[:, :20], True, axis=1)
    b = np.arange(B)
    for j in range(E):
        if j in strong:
            flip[:, :, j] = group
            for _ in range(3):
                flip[b, rng.integers(0, N, B), j] ^= True
        elif j not in unanimous:
            flip[b, rng.integers(0, N, B), j] = True
    R = np.where(flip, 3.0 - R, R)
    rep = _dyadic_reputation(B, N) if dyadic else rng.integers(1, 100, (B, N)).astype(np.float64)
    return R, dict(reputation=rep)


def _oracle(R, kw):
    from oracle import pcx_oracle_c as OC

    return OC.batched(R, **kw, threads=8)


def _compare(R, kw, c, what):
    from pyconsensus_amd.batched import consensus_batched

    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    _assert_bitexact(g, c, what)
    return g


def _ran(c):
    assert np.all(c["flags"] & 3 == 0) and np.all(c["pi_iters"] > 0), "the power iteration ran in every round"


@pytest.mark.gpu
def test_variance_in_events_16_to_19(gpu_lib):
    R, kw = crafted_rounds(strong=(16, 17, 18, 19), seed=501)
    c = _oracle(R, kw)
    _ran(c)
    assert np.all(np.argmax(np.abs(c["adj_first_loadings"]), axis=1) >= 16)
    _compare(R, kw, c, "events 16..19")


@pytest.mark.gpu
def test_variance_in_events_0_to_15(gpu_lib):
    R, kw = crafted_rounds(strong=tuple(range(16)), seed=502)
    c = _oracle(R, kw)
    _ran(c)
    assert np.all(np.argmax(np.abs(c["adj_first_loadings"]), axis=1) < 16)
    _compare(R, kw, c, "events 0..15")


@pytest.mark.gpu
def test_variance_shared_by_events_15_and_16(gpu_lib):
    R, kw = crafted_rounds(strong=(15, 16), seed=503)
    c = _oracle(R, kw)
    _ran(c)
    top2 = np.sort(np.argsort(np.abs(c["adj_first_loadings"]), axis=1)[:, -2:], axis=1)
    assert np.all(top2 == np.array([15, 16]))
    _compare(R, kw, c, "events 15 and 16")


@pytest.mark.gpu
def test_first_nonzero_loading_in_row_1(gpu_lib):
    R, kw = crafted_rounds(strong=(16, 17, 18, 19), seed=504, unanimous=tuple(range(16)), dyadic=True)
    c = _oracle(R, kw)
    _ran(c)
    ld = c["adj_first_loadings"]
    assert np.all(ld[:, :16] == 0.0)
    assert np.all(np.argmax(ld != 0.0, axis=1) >= 16) and np.all(np.any(ld != 0.0, axis=1))
    _compare(R, kw, c, "zeros on events 0..15")


@pytest.mark.gpu
def test_nearly_repeated_leading_eigenvalue(gpu_lib):
    R, kw, kinds = side_rounds(N, E)
    c = _oracle(R, kw)
    check_side_branches(c, kinds)  # (ITERS_IN_LOOP_SQUARING on the degenerate rounds' pi_iters)
    assert np.count_nonzero(c["pi_iters"][kinds["degen"]] >= ITERS_IN_LOOP_SQUARING) >= 8
    _compare(R, kw, c, "side rounds")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["uniform", "missing"])
def test_scores_of_lane_row_3(gpu_lib, case):
    from pyconsensus_amd import synthetic

    if case == "uniform":
        R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=505, reputation=False)
        assert rep is None
    else:
        R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=506, na_frac=0.1)
        frac = np.isnan(R).mean()
        assert 0.08 < frac < 0.12, frac
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    c = _oracle(R, kw)
    s = c["scores"][:, 48:50]
    assert np.all(np.isfinite(s)) and np.count_nonzero(s) > B, "reporters 48 and 49 have scores"
    g = _compare(R, kw, c, case)
    assert np.array_equal(g["scores"][:, 48:50], s)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 4), (50, 21)], ids=["6x4", "50x21"])
def test_dynamic_kernels_as_before(gpu_lib, shape):
    from pyconsensus_amd import synthetic

    n, e = shape
    R, sc, lo, hi, rep = synthetic.rounds(B, n, e, seed=507 + e)
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    _compare(R, kw, _oracle(R, kw), shape)
