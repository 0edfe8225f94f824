"""The edge batteries of the workgroup round kernel (test_medium_edges_gpu.py) without a GPU: every
input of the mask, side-branch and weighted-median batteries is built and run through the C SPEC
(oracle/pcx_oracle_batched.c, NMAX = 256), which must return for each batch, and every precondition
the GPU comparison rests on is asserted on the SPEC's own outputs -- the flags, step counts, branch
rules, component counts, filled values and outcomes the rounds were made for.  A later change to
`synthetic.rounds` or to a generator cannot quietly empty a branch."""
import numpy as np
import pytest

import medium_edges as M


def _workgroup(shape, alg):
    from pyconsensus_amd.batched import route

    assert route(shape[0], shape[1], alg) == "workgroup"


def _returned(c, nb):
    assert set(M.MUST) | {"filled", "original"} <= set(c)
    assert all(len(v) == nb for v in c.values())


@pytest.mark.parametrize("case", M.MASK_CASES, ids=M.mask_id)
def test_mask_batches(case):
    shape, alg, config = case
    _workgroup(shape, alg)
    c = M.mask_spec(*case)  # (raises if the SPEC rejects the batch)
    _returned(c, M.MASK_B)
    M.mask_preconditions(shape, alg, config, c)


@pytest.mark.parametrize("case", M.SIDE_CASES, ids=M.side_id)
def test_side_batches(case):
    shape, alg = case
    _workgroup(shape, alg)
    _, _, kinds = M.side_inputs(*case)
    c = M.side_spec(*case)
    _returned(c, M.SIDE_B)
    M.side_preconditions(shape, alg, c, kinds)


def test_side_batches_measured_counts():
    """The counts the batteries were sized by (seed 11, 96 rounds, PCA): rounds at or past the in-loop
    squaring / below it, and rounds that stop at the iteration cap."""
    want = {(65, 33): (22, 10, 0), (33, 64): (25, 7, 0), (100, 50): (29, 3, 4), (200, 34): (30, 2, 9),
            (256, 64): (30, 2, 9)}
    for shape, (late, early, maxit) in want.items():
        _, _, kinds = M.side_inputs(shape, "PCA")
        assert M.side_counts(M.side_spec(shape, "PCA"), kinds) == (32, 32, maxit, late, early), shape


@pytest.mark.parametrize("case", M.MEDIAN_CASES, ids=M.side_id)
def test_median_batches(case):
    shape, alg = case
    _workgroup(shape, alg)
    R, _, groups = M.median_inputs(*case)
    c = M.median_spec(*case)
    _returned(c, M.MEDIAN_B)
    M.median_preconditions(shape, alg, R, c, groups)


@pytest.mark.parametrize("case", [c for c in M.MEDIAN_CASES if c[1] != "PCA"], ids=M.side_id)
def test_outcome_median_over_nan_values_equals_the_restatement(case):
    """Under "absolute" and "clusterfeck" the reputations stay finite where the crafted column was
    filled with NaN, so the outcome median sorts NaN values: the SPEC's order is the numpy
    restatement's (np.lexsort: a NaN after every number), every slot of the sorted pairs written.
    (A rank rule that compares NaN with < and == alone leaves slots unwritten, and the median then
    read whatever the stack held.)"""
    from oracle.pcx_oracle import weighted_median

    shape, alg = case
    js = shape[1] - 1
    _, _, groups = M.median_inputs(*case)
    c = M.median_spec(*case)
    n = 0
    for name in M.MEDIAN_GROUPS:
        for b in groups[name]:
            x, w = c["filled"][b, :, js], c["smooth_rep"][b]
            want = weighted_median(x, w)
            want = np.nan if want is None else float(want)
            got = float(c["outcomes_raw"][b, js])
            assert got == want or (got != got and want != want), (name, int(b), got, want)
            n += bool(np.isnan(x).any() and np.isfinite(w).all())
    assert n == 2 * M.MEDIAN_GROUP  # the zero-weight-only and scaled-column-missing groups


def test_median_generator_layout():
    """What the generator promises about its inputs at every shape: the crafted column's bounds and
    integer reports, the tie group's dyadic weights, the dominant reporter's weight."""
    for N, E in M.SHAPES + M.WAVE_SHAPES:
        R, kw, groups = M.median_rounds(N, E)
        js, rep = E - 1, kw["reputation"]
        assert sorted(np.concatenate(list(groups.values())).tolist()) == list(range(M.MEDIAN_B))
        assert kw["scaled"][:, js].all() and (kw["lo"][:, js] == 0.0).all() and (kw["hi"][:, js] == 8.0).all()
        col = R[:, :, js]
        assert np.all(np.isnan(col) | ((col == np.trunc(col)) & (col >= 1.0) & (col <= 7.0)))
        for b in groups["tie"]:
            present = np.flatnonzero(~np.isnan(col[b]))
            P = len(present)
            assert P & (P - 1) == 0 and P <= N - 1 < 2 * P and present[0] == 1 and present[-1] == P
            assert np.count_nonzero(col[b] == 2.0) == np.count_nonzero(col[b] == 6.0) == P // 2
            total = rep[b].sum()
            assert total == 2.0 ** round(np.log2(total)) and np.all(rep[b, 1:] == 1.0)
        for b in groups["dominant"]:
            d = int(np.argmax(rep[b]))
            assert rep[b, d] == 2.0 * (rep[b].sum() - rep[b, d]) + 1.0 and col[b, d] == 3.0 and np.isnan(col[b]).any()
        for b in groups["zero-weight-only"]:
            present = ~np.isnan(col[b])
            assert present.sum() == 3 and np.all(rep[b, present] == 0.0)
        for b in groups["zeros-sprinkled"]:
            assert np.all(rep[b, ::3] == 0.0) and np.isnan(col[b]).any()
        for b in groups["one-present"]:
            assert np.count_nonzero(~np.isnan(col[b])) == 1 and np.nansum(col[b]) == 4.0
        assert np.isnan(col[groups["scaled-column-missing"]]).all()
        bm = groups["binary-column-missing"]
        assert np.isnan(R[bm, :, 0]).all() and not kw["scaled"][bm, 0].any()


@pytest.mark.parametrize("alg", M.RAGGED_ALGS)
def test_ragged_battery(alg):
    """The ragged launch's rounds: the first 24 of each side kind and every median group, four
    one-wave shapes, shuffled; the SPEC returns for each shape and the launch mixes the exits."""
    per, order = M.ragged_inputs()
    assert len(per) == len(M.WAVE_SHAPES) and len(order) == 4 * (3 * M.RAGGED_TAKE + M.MEDIAN_B)
    assert len(set(order)) == len(order) and order != sorted(order)
    M.ragged_preconditions(alg)
