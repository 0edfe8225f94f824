"""Tall rounds in ragged batches on the GPU (csrc/pcx_tall_ragged.hip, consensus_ragged(..., tall=True);
DESIGN.md 5.5.3): every output of every round above 256 reporters bit for bit against the C SPEC built
for 1024 reporters (tests/tall_ragged_cases.py), NaNs matching NaNs; every other round against the
wide ragged call on the batch without the tall rounds.  The inputs' coverage is asserted on the plan
and the SPEC alone in test_tall_ragged_cpu.py."""
import numpy as np
import pytest

import tall_cases as T
import tall_ragged_cases as G

pytestmark = pytest.mark.gpu

BOTH = G.EVERY + ("filled", "original")


def _host(out):
    from pyconsensus_amd.batched import ragged_to_host

    return ragged_to_host(out)


def _names(host):
    return [k for k in host if not k.startswith("_")]


def _rounds_equal(a, ia, b, ib, what):
    """Round ia of host result a and round ib of host result b: the same bytes in every output."""
    from pyconsensus_amd.batched import ragged_round

    ga, gb = ragged_round(a, ia), ragged_round(b, ib)
    assert set(ga) == set(gb)
    for k in ga:
        assert np.asarray(ga[k]).tobytes() == np.asarray(gb[k]).tobytes(), (what, k)


_MIX = {}


def _mix(filled=True):
    """The mixed call on the host (run once per variant, left unchanged)."""
    from pyconsensus_amd.batched import consensus_ragged

    if filled not in _MIX:
        reports, kw = G.ragged_args(G.mix_rounds())
        _MIX[filled] = _host(consensus_ragged(reports, tall=True, filled=filled, original=filled, **kw))
    return _MIX[filled]


def test_mixed_call_tall_rounds_bitexact_vs_spec(gpu_lib):
    from pyconsensus_amd.batched import ragged_round

    g = _mix()
    for b, s in enumerate(G.MIX_SHAPES):
        if G.is_tall(s):
            G.assert_round(ragged_round(g, b), G.mix_spec(b), 0, (b, s), must=BOTH)


def test_mixed_call_small_rounds_are_the_wide_calls(gpu_lib):
    from pyconsensus_amd.batched import consensus_ragged

    small = [b for b, s in enumerate(G.MIX_SHAPES) if not G.is_tall(s)]
    assert len(small) == 4
    reports, kw = G.ragged_args(G.mix_rounds(), small)
    w = _host(consensus_ragged(reports, wide=True, filled=True, original=True, **kw))
    g = _mix()
    for k, b in enumerate(small):
        _rounds_equal(g, b, w, k, G.MIX_SHAPES[b])


def test_per_round_sets_bitexact_vs_spec(gpu_lib):
    from pyconsensus_amd.batched import consensus_ragged, ragged_round

    reports, kw = G.ragged_args(G.sets_rounds())
    g = _host(consensus_ragged(reports, tall=True, per_round=[q for _, q in G.SETS_CASES], aux_scores=G.sets_aux(),
                               filled=True, original=True, **kw))
    for b, case in enumerate(G.SETS_CASES):
        G.assert_round(ragged_round(g, b), G.sets_spec(b), 0, case, must=BOTH)


@pytest.mark.parametrize("battery", ["bounds", "side", "nan"])
def test_batteries_through_the_ragged_entry(gpu_lib, battery):
    """Crafted masks, the side battery and the NaN rank path at 513 x 33, null `filled` / `original`:
    the filled matrix lives in the tall segment's own scratch slots."""
    from pyconsensus_amd.batched import consensus_ragged, ragged_round

    if battery == "bounds":
        R, kw = T.mask_inputs(G.BATTERY_SHAPE, "bounds")
        c = T.mask_spec(G.BATTERY_SHAPE, "bounds")
    elif battery == "side":
        R, kw, _ = T.side_inputs(G.BATTERY_SHAPE)
        c = T.side_spec(G.BATTERY_SHAPE)
    else:
        R, kw, _ = T.nan_inputs()
        c = T.nan_spec()
    reports, rkw = G.battery_args(R, kw)
    g = _host(consensus_ragged(reports, tall=True, **rkw))
    assert "filled" not in g and "original" not in g
    for b in range(len(R)):
        G.assert_round(ragged_round(g, b), c, b, (battery, b))


def test_tall_segment_in_chunks(gpu_lib):
    """pcx_test_scratch_cap at two slots of the largest tall round: seven tall rounds in four chunks,
    and the workgroup rounds' chunks under the same cap.  The same bytes."""
    import torch
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import consensus_ragged

    reports, kw = G.ragged_args(G.mix_rounds())
    whole = _mix(filled=False)
    ctx = _lib.context(torch.cuda.current_device())
    per_round = (1024 * 64 + 64 * 64) * 8  # the tall segment's slot: its largest N E and E E
    _lib.check(gpu_lib.pcx_test_scratch_cap(ctx, 2 * per_round))
    try:
        capped = _host(consensus_ragged(reports, tall=True, **kw))
    finally:
        _lib.check(gpu_lib.pcx_test_scratch_cap(ctx, 0))
    for name in _names(whole):
        assert capped[name].tobytes() == whole[name].tobytes(), name
    f = _mix()
    for name in capped:
        if not name.startswith("_"):
            assert capped[name].tobytes() == f[name].tobytes(), name  # and with the caller's `filled`


def test_no_tall_round_is_the_params_call(gpu_lib):
    from pyconsensus_amd.batched import consensus_ragged

    small = [b for b, s in enumerate(G.MIX_SHAPES) if not G.is_tall(s)]
    reports, kw = G.ragged_args(G.mix_rounds(), small)
    per_round = [{}, {"alpha": 0.3}, {"algorithm": "hierarchical"}, {"algorithm": "big-five"}]
    a = _host(consensus_ragged(reports, tall=True, per_round=per_round, filled=True, original=True, **kw))
    b = _host(consensus_ragged(reports, wide=True, per_round=per_round, filled=True, original=True, **kw))
    for name in _names(a):
        assert a[name].tobytes() == b[name].tobytes(), name


def test_calls_are_asynchronous_and_ordered(gpu_lib):
    """Two calls back to back on one stream without a synchronise between them (they share the context's
    scratch and take the two staging slots in turn): each gives the bytes of its synchronised run."""
    import torch
    from pyconsensus_amd.batched import consensus_ragged

    ra, kwa = G.ragged_args(G.mix_rounds())
    rb, kwb = G.ragged_args(G.sets_rounds())
    more = dict(per_round=[q for _, q in G.SETS_CASES], aux_scores=G.sets_aux())
    torch.cuda.synchronize()
    a1 = consensus_ragged(ra, tall=True, **kwa)
    b1 = consensus_ragged(rb, tall=True, **kwb, **more)
    torch.cuda.synchronize()
    a1, b1 = _host(a1), _host(b1)
    a2 = _mix(filled=False)
    b2 = _host(consensus_ragged(rb, tall=True, **kwb, **more))
    for x, y in ((a1, a2), (b1, b2)):
        for name in _names(x):
            assert x[name].tobytes() == y[name].tobytes(), name


def test_deterministic(gpu_lib):
    from pyconsensus_amd.batched import consensus_ragged

    reports, kw = G.ragged_args(G.mix_rounds())
    again = _host(consensus_ragged(reports, tall=True, filled=True, original=True, **kw))
    first = _mix()
    for name in _names(first):
        assert again[name].tobytes() == first[name].tobytes(), name
