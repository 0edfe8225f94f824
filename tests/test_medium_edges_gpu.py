"""The workgroup-per-round kernel (csrc/pcx_medium.hip, rounds above 64 x 32 up to 256 x 64) on crafted
rounds that take its side branches, bit for bit (NaN equal to NaN) against the C SPEC
(oracle/pcx_oracle_batched.c, NMAX = 256) on every output the GPU returns, `flags`, `pi_iters`,
`branch`, `components`, `filled` and `original` included.  No tolerance anywhere: the SPEC is the
reference and equality is the criterion.  Every case asserts ``route(N, E, alg) == "workgroup"``.
Inputs, SPEC runs and preconditions come from medium_edges.py; test_medium_edges_cpu.py asserts the
same preconditions without a GPU.

Shapes (medium_edges.SHAPES): 65 x 33, 129 x 3, 33 x 64, 100 x 50, 200 x 34, 256 x 64 -- the row
chunks of the median compaction and of the NaN rank path (nq = 2, 3, 4), odd E across the 2-bit flag
words, ragged / single / all 256 covariance tiles, the LDS carve at capacity.

1. Masks: `crafted_rounds` of test_batched_masks_gpu.py (a row all NaN, a row all 0.0, a column with
   one report, a column all 0.0, reports at `lo` / `hi`) in its five configurations; PCA at the six
   shapes, the other algorithms and the three clusterings at 65 x 33 and 100 x 50; and once with
   ``filled=False, original=False`` (the kernel's scratch F, null output pointers).
2. Covariance and power-iteration exits: 96 rounds of test_batched_pi_gpu.side_rounds (32 identical
   reporters: ZERO_COV; 32 overflowing bounds: SVD_FAIL; 32 nearly repeated eigenvalues: the in-loop
   squarings and, at 100 x 50, 200 x 34 and 256 x 64, the PI_MAXIT exit).
3. Weighted-median paths: medium_edges.median_rounds, seven groups of eight rounds over
   `synthetic.rounds`, the last column scaled on [0, 8] with small integer reports.
4. The one-wave forms of 2 and 3 (7 x 20, 50 x 20, 63 x 31, 64 x 32) shuffled into one
   `consensus_ragged` launch: a round that leaves the power iteration at once beside one that runs
   to the cap under the descriptor path (PCA, big-five; "absolute" on top, where the one-wave
   kernel's outcome median ranks NaN values beside finite reputations).

Found by battery 3 and fixed with it: the rank placement compared NaN values with `<` and `==`
alone, so every NaN took rank 0 and the slots above the numbers stayed unwritten -- the SPEC then
read its stack and the kernels stale LDS (`outcomes_raw` of the NaN-filled column under "absolute",
"clusterfeck" and "cokurtosis", every shape).  The order is now numpy's (a NaN after every number),
the numpy restatement's `np.lexsort`, in the SPEC and in both kernels.

Which `wmedian` branch the crafted column of battery 3 takes, counted once on the CPU with an
instrumented copy of the SPEC (calls of 8 per group; "network" = the stable order without a NaN, the
kernel's bitonic network; "NaN rank" = the order with a NaN among the values, the kernel's rank path;
"+ tie" = the walk stops exactly at the middle and averages).  The fill column is the same at all
six shapes and under every algorithm:

======================  ===================  ===========================================================
group                   fill median          outcome median
======================  ===================  ===========================================================
tie                     network + tie, 8     PCA: dominant 7 + network 1 (65 x 33, 129 x 3), dominant 8
                                             (33 x 64), network 8 (100 x 50, 200 x 34, 256 x 64);
                                             absolute: network 8, at 256 x 64 all 8 + tie;
                                             clusterfeck: dominant 8 (65 x 33), network 8 (256 x 64)
dominant                dominant 8           dominant 8
zero-weight-only        no positive          PCA: no positive weight 8 (NaN reputations);
                        weight 8 (0 / 0)     absolute, clusterfeck: NaN rank 8 (nq = 2, 3, 4)
zeros-sprinkled         network 8            network 8
one-present             dominant 8 (n = 1)   network 8
scaled-column-missing   no positive          PCA: no positive weight 8;
                        weight 8 (n = 0)     absolute, clusterfeck: NaN rank 8
binary-column-missing   network 8            network 8
======================  ===================  ===========================================================

(The other scaled columns of these rounds add 100-280 network calls per group at the wide shapes,
some ending in a tie: 127 of them under "absolute" at 256 x 64 in the tie group, whose dyadic
reputations make exact half sums common; one fill of the binary-column-missing group at 33 x 64 ends
in a tie too.)  The one-wave forms at 50 x 20, 63 x 31 and 64 x 32 take the PCA column's branches with
"network 8" in the tie group's outcome; at 7 x 20 every third reporter without reputation leaves a
dominant one in 6 fills and 2 outcomes of the zeros-sprinkled group.
"""
import numpy as np
import pytest

import medium_edges as M

pytestmark = pytest.mark.gpu


def _np(outs):
    return {k: v.cpu().numpy() for k, v in outs.items() if not k.startswith("_")}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind != "f":
        return a == b
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def _assert_bitexact(g, c, what, must=M.MUST + ("filled", "original")):
    assert set(must) <= set(g) <= set(c), (what, set(must) - set(g), set(g) - set(c))
    for k, v in g.items():
        same = _same_bits(v, c[k])
        rounds = np.flatnonzero(~same.reshape(len(same), -1).all(axis=1))
        assert len(rounds) == 0, "%s: %s differs from the SPEC in %d entries, rounds %s" % (
            what, k, int(np.size(same) - np.count_nonzero(same)), rounds[:12].tolist())


def _run(shape, alg, R, kw, **extra):
    from pyconsensus_amd.batched import consensus_batched, route

    assert route(shape[0], shape[1], alg) == "workgroup"
    extra = dict(dict(filled=True, original=True), **extra)
    return _np(consensus_batched(R, **kw, **extra))


@pytest.mark.parametrize("case", M.MASK_CASES, ids=M.mask_id)
def test_masks_bitexact(gpu_lib, case):
    shape, alg, config = case
    c = M.mask_spec(*case)
    M.mask_preconditions(shape, alg, config, c)
    R, kw = M.mask_inputs(*case)
    _assert_bitexact(_run(shape, alg, R, kw), c, M.mask_id(case))


@pytest.mark.parametrize("shape", M.MASK_NOFILL, ids=M.sid)
def test_masks_without_filled_and_original(gpu_lib, shape):
    """``filled=False, original=False``: the filled matrix lives in the kernel's scratch and both
    output pointers are null; every remaining output equals the SPEC."""
    R, kw = M.mask_inputs(shape, "PCA", "bounds")
    g = _run(shape, "PCA", R, kw, filled=False, original=False)
    assert "filled" not in g and "original" not in g
    _assert_bitexact(g, M.mask_spec(shape, "PCA", "bounds"), "%s without filled / original" % M.sid(shape),
                     must=M.MUST + ("nas_filled", "na_row", "participation_rows", "participation_columns"))


@pytest.mark.parametrize("case", M.SIDE_CASES, ids=M.side_id)
def test_side_branches_bitexact(gpu_lib, case):
    shape, alg = case
    R, kw, kinds = M.side_inputs(*case)
    c = M.side_spec(*case)
    M.side_preconditions(shape, alg, c, kinds)
    _assert_bitexact(_run(shape, alg, R, kw), c, M.side_id(case))


@pytest.mark.parametrize("case", M.MEDIAN_CASES, ids=M.side_id)
def test_median_paths_bitexact(gpu_lib, case):
    shape, alg = case
    R, kw, groups = M.median_inputs(*case)
    c = M.median_spec(*case)
    M.median_preconditions(shape, alg, R, c, groups)
    _assert_bitexact(_run(shape, alg, R, kw), c, M.side_id(case))


@pytest.mark.parametrize("alg", M.RAGGED_ALGS)
def test_side_and_median_rounds_in_one_ragged_launch(gpu_lib, alg):
    """The one-wave forms of batteries 2 and 3, four shapes shuffled into one launch: each round
    equals the SPEC run on its own shape, on every output."""
    from pyconsensus_amd.batched import consensus_ragged, ragged_round, ragged_to_host

    per, order = M.ragged_inputs()
    M.ragged_preconditions(alg)
    ref = M.ragged_spec(alg)
    rounds = [(per[k][bat][0][b], {name: v[b] for name, v in per[k][bat][1].items()}) for k, bat, b in order]
    pick = lambda name: [kw[name] for _, kw in rounds]
    extra = {k: v for k, v in M._algorithm_kw(alg, 0, 0, 0).items()}
    host = ragged_to_host(consensus_ragged([r for r, _ in rounds], pick("reputation"), pick("scaled"), pick("lo"),
                                           pick("hi"), filled=True, original=True, **extra))
    names = [k for k in host if not k.startswith("_")]
    assert set(M.MUST + ("filled", "original")) <= set(names) <= set(ref[0]["side"])
    for i, (k, bat, b) in enumerate(order):
        g = ragged_round(host, i)
        for name in names:
            assert _same_bits(g[name], ref[k][bat][name][b]).all(), (alg, i, M.WAVE_SHAPES[k], bat, b, name)
