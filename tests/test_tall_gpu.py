"""Tall batched rounds on the GPU (csrc/pcx_tall.hip, consensus_batched(..., tall=True)): every output
bit for bit against the C SPEC built for 1024 reporters (tests/tall_cases.py), NaNs matching NaNs, at the
smallest shapes at which each new thing can go wrong (tall_cases.SYNTH_SHAPES); then that nothing changes
where the route is not tall, that the call is asynchronous, and that it is deterministic.  The inputs'
own coverage is asserted on the SPEC alone in test_tall_cpu.py."""
import numpy as np
import pytest

import tall_cases as T

pytestmark = pytest.mark.gpu

EVERY = ("old_rep", "this_rep", "smooth_rep", "scores", "na_row", "participation_rows", "relative_part",
         "reporter_bonus", "adj_first_loadings", "outcomes_raw", "outcomes_adjusted", "outcomes_final", "certainty",
         "consensus_reward", "nas_filled", "participation_columns", "author_bonus", "participation", "avg_certainty",
         "branch", "flags", "pi_iters", "components")


def _np(outs):
    return {k: v.cpu().numpy() for k, v in outs.items() if not k.startswith("_")}


def _tall(R, kw, **more):
    from pyconsensus_amd.batched import consensus_batched, route

    N, E = R.shape[1:]
    assert route(N, E, kw.get("algorithm", "PCA"), tall=True) == "tall"
    return _np(consensus_batched(R, tall=True, **kw, **more))


def _assert_bitexact(g, c, what, must=EVERY):
    assert set(must) <= set(g) <= set(c), (what, set(must) - set(g), set(g) - set(c))
    for k, v in g.items():
        same = T.bits_equal(v, c[k])
        assert np.all(same), (what, k, int(np.size(same) - np.count_nonzero(same)))


@pytest.mark.parametrize("shape", T.SYNTH_SHAPES, ids=T.sid)
def test_pca_bitexact_vs_spec(gpu_lib, shape):
    R, kw = T.synth_inputs(shape)
    _assert_bitexact(_tall(R, kw, filled=True, original=True), T.synth_spec(shape), shape, must=EVERY + ("filled", "original"))


@pytest.mark.parametrize("case", T.ALG_CASES, ids=lambda c: "%s_%s" % (c[0] if c[0] == "capacity" else T.sid(c[0]), c[1]))
def test_algorithms_bitexact_vs_spec(gpu_lib, case):
    shape, alg = case
    R, kw = T.synth_inputs(shape, alg)
    _assert_bitexact(_tall(R, kw, filled=True, original=True), T.synth_spec(shape, alg), case,
                     must=EVERY + ("filled", "original"))


@pytest.mark.parametrize("config", T.CONFIGS)
@pytest.mark.parametrize("shape", T.BATTERY_SHAPES, ids=T.sid)
def test_masks_bitexact_vs_spec(gpu_lib, shape, config):
    R, kw = T.mask_inputs(shape, config)
    _assert_bitexact(_tall(R, kw, filled=True, original=True), T.mask_spec(shape, config), (shape, config),
                     must=EVERY + ("filled", "original"))


@pytest.mark.parametrize("shape", [(513, 33), (1024, 64)], ids=T.sid)
def test_masks_without_filled_and_original(gpu_lib, shape):
    """Null `filled` / `original`: the filled matrix lives in the kernel's own scratch."""
    R, kw = T.mask_inputs(shape, "bounds")
    g = _tall(R, kw)
    assert "filled" not in g and "original" not in g
    _assert_bitexact(g, T.mask_spec(shape, "bounds"), shape)


@pytest.mark.parametrize("shape", T.BATTERY_SHAPES, ids=T.sid)
def test_side_branches_bitexact_vs_spec(gpu_lib, shape):
    R, kw, _ = T.side_inputs(shape)
    _assert_bitexact(_tall(R, kw, filled=True, original=True), T.side_spec(shape), shape,
                     must=EVERY + ("filled", "original"))


def test_nan_rank_path_bitexact_vs_spec(gpu_lib):
    R, kw, _ = T.nan_inputs()
    _assert_bitexact(_tall(R, kw, filled=True), T.nan_spec(), "nan", must=EVERY + ("filled",))


def _bytes_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("case", [(100, 50, "PCA"), (256, 64, "PCA"), (300, 20, "hierarchical")],
                         ids=lambda c: "%dx%d_%s" % c)
def test_other_routes_keep_their_bytes(gpu_lib, case):
    """tall=True changes nothing where the route is not tall: the workgroup kernel up to 256 x 64,
    the scheduler for a clustering above."""
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched, route

    N, E, alg = case
    assert route(N, E, alg, tall=True) == route(N, E, alg) != "tall"
    R, sc, lo, hi, rep = synthetic.rounds(4, N, E, seed=41)
    kw = dict(algorithm=alg, filled=True, original=True)
    a = _np(consensus_batched(R, rep, sc, lo, hi, **kw))
    b = _np(consensus_batched(R, rep, sc, lo, hi, tall=True, **kw))
    _bytes_equal(a, b, case)


def test_tall_agrees_with_the_scheduler_within_tolerance(gpu_lib):
    """300 x 20 PCA: the scheduler gives the single-matrix path's arithmetic, the tall route the SPEC's;
    the continuous outputs agree within tests/parity.py's tolerance, the binary events' outcomes exactly."""
    from parity import ATOL, RTOL
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched

    R, sc, lo, hi, rep = synthetic.rounds(4, 300, 20, seed=43)
    s = _np(consensus_batched(R, rep, sc, lo, hi))
    g = _tall(R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi))
    _assert_bitexact(g, T.spec(R, sc, lo, hi, rep), "300x20")
    for k in ("smooth_rep", "this_rep", "scores", "adj_first_loadings", "outcomes_raw", "outcomes_final", "certainty",
              "consensus_reward", "reporter_bonus", "author_bonus", "participation_rows", "participation_columns"):
        err = np.abs(g[k] - s[k])
        print(k, float(err.max()))
        assert np.all(err <= ATOL + RTOL * np.abs(s[k])), (k, float(err.max()))
    binary = ~np.asarray(sc, dtype=bool)
    assert np.array_equal(g["outcomes_final"][binary], s["outcomes_final"][binary])


def test_calls_are_asynchronous_and_ordered(gpu_lib):
    """Two back-to-back calls on one stream and one synchronise give the bytes of two synchronised
    calls (the calls share the context's scratch: stream order keeps them apart)."""
    import torch
    from pyconsensus_amd.batched import consensus_batched

    Ra, kwa = T.synth_inputs((513, 33))
    Rb, kwb = T.synth_inputs((640, 62))
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda R, kw: (torch.as_tensor(R, device=dev), {k: torch.as_tensor(np.asarray(v, dtype=np.uint8 if k == "scaled" else np.float64), device=dev)
                                                          for k, v in kw.items()})
    (Ra, kwa), (Rb, kwb) = up(Ra, kwa), up(Rb, kwb)
    torch.cuda.synchronize()
    a1 = consensus_batched(Ra, tall=True, **kwa)
    b1 = consensus_batched(Rb, tall=True, **kwb)
    torch.cuda.synchronize()
    a2 = consensus_batched(Ra, tall=True, **kwa)
    torch.cuda.synchronize()
    b2 = consensus_batched(Rb, tall=True, **kwb)
    torch.cuda.synchronize()
    _bytes_equal(_np(a1), _np(a2), "first call")
    _bytes_equal(_np(b1), _np(b2), "second call")
    _assert_bitexact(_np(a1), T.synth_spec((513, 33)), "first call")
    _assert_bitexact(_np(b1), T.synth_spec((640, 62)), "second call")


def test_deterministic_at_capacity(gpu_lib):
    R, kw = T.synth_inputs((1024, 64))
    a, b = _tall(R, kw, filled=True), _tall(R, kw, filled=True)
    for k in a:
        v, w = a[k], b[k]
        if v.dtype.kind == "f":
            v, w = v.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(v, w), k
