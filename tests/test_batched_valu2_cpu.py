"""The batches of batched_valu2_cases.py on the CPU: each is what it claims to be, asserted on the C
oracle's own outputs.  No GPU."""
import pytest

import batched_valu2_cases as VC


@pytest.mark.parametrize("name", VC.IP_KINDS + VC.NAMES)
def test_case_is_what_it_claims(name):
    VC.check(name)


def test_denominator_recipe():
    """The two reputation vectors of cov_denom_*: numpy's pairwise total is 10^6 exactly, and the tokens
    int(rep * 1e6) summed in the SPEC's tree order (a butterfly inside each 16-lane row, then
    (R0 + R1) + (R2 + R3)) give 1 and 0."""
    import numpy as np

    for name, want in (("cov_denom_zero", 1.0), ("cov_denom_negative", 0.0)):
        _, kw, c = VC.batch(name)
        raw = kw["reputation"][0]
        assert float(np.sum(raw)) == 1e6  # (add.reduce of 50 doubles: numpy's pairwise order)
        tok = np.zeros(64)
        tok[:VC.N] = np.trunc(c["old_rep"][0] * 1e6)
        v = tok.copy()
        for d in (1, 2, 4, 8):
            v = v + v[np.arange(64) ^ d]
        assert float((v[0] + v[16]) + (v[32] + v[48])) == want
