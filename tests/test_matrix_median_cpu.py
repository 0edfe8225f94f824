"""The crafted weighted-median columns of the single-matrix path (matrix_median_cases.py), checked on the
numpy restatement alone: each group's precondition holds in OracleCPU's own outputs, no crafted column's
outcome median hangs on the last bits of its weights, and pcx_oracle.weighted_median agrees with the
published weightedstats text on every crafted column's (values, weights).  Needs no GPU."""
import numpy as np
import pytest

import matrix_median_cases as M

CASES = [(k, n) for n in (M.N_SMALL, M.N_TIERS) for k in M.KINDS]
case_id = lambda kn: "%s_%d" % kn


@pytest.mark.parametrize("kn", CASES, ids=case_id)
def test_preconditions(kn):
    c = M.case(*kn)
    assert c.R.shape == (kn[1], M.E) and M.E <= 32
    M.preconditions(c, M.reference(*kn))


@pytest.mark.parametrize("kn", [kn for kn in CASES if kn[0] not in M.TIE_KINDS], ids=case_id)
def test_outcome_medians_do_not_hang_on_the_weights_last_bits(kn):
    c = M.case(*kn)
    assert M.stability(c, M.reference(*kn)) == c.crafted


@pytest.mark.parametrize("kn", CASES, ids=case_id)
def test_interpolate_alone_matches_consensus_fill(kn):
    """OracleCPU.interpolate (the phase-1 reference of the GPU tests) is the `filled` of consensus()."""
    assert np.all(M.bits_equal(M.reference_filled(*kn), M.reference(*kn)["filled"]))


@pytest.mark.parametrize("kn", CASES, ids=case_id)
def test_weighted_median_is_weightedstats(kn):
    """Both medians of every crafted column: the restatement (np.cumsum, np.lexsort) against the
    package's own statements on Python lists."""
    from oracle.pcx_oracle import weighted_median

    c, ref = M.case(*kn), M.reference(*kn)
    seen = set()
    for g, j in c.cols.items():
        for phase, (x, w) in enumerate(M.column_pairs(c, ref, j), 1):
            # (nothing present, or NaN weights -- 0 / 0 of the zero-weight-only column, the NaN
            # smooth_rep beside a NaN fill: no comparison is true, both return None)
            got = weighted_median(x, w)
            want = M.weightedstats_weighted_median(x.tolist(), w.tolist())
            assert (got is None) == (want is None), (g, phase)
            assert got is None or M.bits_equal(got, want), (g, phase, got, want)
            seen.add((g, phase))
    assert len(seen) == 2 * len(c.cols)


def test_deep_column_passes_follow_from_its_key_range():
    """ceil(bits / 8): the narrowing model on the deep column's keys, and on a column that narrows faster
    (the bound is what the deep column's spacing forces, not what any column takes)."""
    c = M.case("given", M.N_SMALL)
    j = c.cols["deep"]
    x = M.rescaled(c, j)
    keys = [M.dkey(v) for v in x[~np.isnan(x)]]
    assert M.model_passes(keys, M.dkey(0.5)) == M.deep_min_passes(c, j) == 8
    jd = c.cols["duplicates"]
    xd = M.rescaled(c, jd)
    assert M.model_passes([M.dkey(v) for v in xd[~np.isnan(xd)]], M.dkey(0.5)) == 1
