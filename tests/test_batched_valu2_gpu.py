"""The compiled 50 x 20 batched kernel's old = np.dot(rep, F) as the third vector of the n1 / n2 pass, the
covariance's divisions through one reciprocal and the normalisations' square roots without the range
scaling, and the interpolation medians' prescreen at its tail rows and odd reputations
(csrc/pcx_batched.hip, csrc/pcx_batched_round.inc).

Every batch of batched_valu2_cases.py through consensus_batched with filled=True, original=True, compared
with the C oracle bit for bit on every output, `branch`, `flags` and `pi_iters` included, after the
case's own assertions on the oracle's outputs (test_batched_valu2_cpu.py runs those alone)."""
import numpy as np
import pytest

import batched_valu2_cases as VC
from test_batched_pi_gpu import _assert_bitexact, _np


def _run(name):
    from pyconsensus_amd.batched import consensus_batched

    VC.check(name)
    R, kw, c = VC.batch(name)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    assert {"original", "filled", "branch", "flags", "pi_iters", "certainty"} <= set(g)
    _assert_bitexact(g, c, name)
    return g, c


@pytest.mark.gpu
@pytest.mark.parametrize("name", VC.IP_KINDS + VC.PRESCREEN)
def test_prescreen(gpu_lib, name):
    _run(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", VC.OLD + VC.CONTROLS)
def test_old_in_the_nonconformity_pass(gpu_lib, name):
    g, c = _run(name)
    assert np.array_equal(g["branch"], c["branch"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", VC.COV)
def test_covariance_division(gpu_lib, name):
    g, c = _run(name)
    assert np.array_equal(g["flags"], c["flags"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", VC.SQRT)
def test_square_root_ranges(gpu_lib, name):
    g, c = _run(name)
    assert np.array_equal(g["pi_iters"], c["pi_iters"])
