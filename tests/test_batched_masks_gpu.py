"""The batched kernel's missing-report bookkeeping (per-row NaN / zero bit masks, per-column zero
counts, the rescale loop over the scaled columns only) and its np.dot passes, bit for bit against
the C oracle (oracle/pcx_oracle_batched.c) on every output, `original` and `filled` included.

Mask cases: 48 rounds of `synthetic.rounds` with crafted entries written over them, six rounds per
pattern -- a row entirely NaN; a row entirely 0.0; a column with one present report; a column
entirely 0.0 (at 64 x 32 that is a column of 64 zeros beside a row of 32 NaN, the counters'
maxima); a scaled column with reports exactly at `lo` (they rescale to 0.0 and count as zeros
after the rescale) and at `hi`, some missing; the same column with nothing missing; untouched
rounds.  Each batch runs as it is, without bounds, with bounds but no scaled column, with every
column scaled, and with int_dtype (truncated reports, 0 for NaN, the crafted column alone scaled).
Shapes: 50 x 20 on both compiled instantiations (PCA packed, big-five unpacked), 64 x 32, 1 x 6,
30 x 1 and 7 x 5 on the dynamic ones.

Every crafted batch was run through the C oracle on the CPU first: it rejects none of them (it
returns for each; where a round has no usable report its outputs are NaN on both sides), so no
pattern was dropped.

np.dot cases: PCA rounds over E in {2, 3, 5, 17, 32} and N in {1, 2, 3, 6, 50, 64}, 32 rounds
each: OpenBLAS's block, pair and tail orders (ob_vecmat), with the two nonconformity products in
one pass on lanes j and 32 + j (lane 63 at E = 32); `branch`, `flags` and `pi_iters` included.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, GROUP = 48, 6
SHAPES = [(50, 20, "PCA"), (50, 20, "big-five"), (64, 32, "PCA"), (1, 6, "PCA"), (30, 1, "PCA"), (7, 5, "PCA")]
CONFIGS = ["bounds", "nobounds", "noscaled", "allscaled", "int"]
LO, HI = -8.0, 42.0  # the crafted scaled column's bounds (integers: int_dtype keeps reports at lo and hi there)


def _np(outs):
    return {k: v.cpu().numpy() for k, v in outs.items() if not k.startswith("_")}


def _assert_bitexact(g, c, what, must=()):
    assert set(must) <= set(g) <= set(c), (what, set(must) - set(g), set(g) - set(c))
    for k, v in g.items():
        same = (v == c[k]) | (np.isnan(v) & np.isnan(c[k])) if v.dtype.kind == "f" else (v == c[k])
        assert np.all(same), (what, k, int(np.size(same) - np.count_nonzero(same)))


def crafted_rounds(N, E, config, seed=31):
    """(reports, keyword arguments) of one mask case."""
    from pyconsensus_amd import synthetic

    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=seed + 64 * N + E)
    sc, lo, hi = sc.copy(), lo.copy(), hi.copy()
    rng = np.random.default_rng(seed)
    g = lambda k: np.arange(k * GROUP, (k + 1) * GROUP)
    js = E - 1  # the crafted scaled column
    for b in g(0):  # a row entirely NaN
        R[b, rng.integers(N), :] = np.nan
    for b in g(1):  # a row entirely 0.0
        R[b, rng.integers(N), :] = 0.0
    for b in g(2):  # a column with one present report
        j, keep = rng.integers(E), rng.integers(N)
        v = R[b, keep, j]
        R[b, :, j] = np.nan
        R[b, keep, j] = 1.0 if np.isnan(v) else v
    for b in g(3):  # a column entirely 0.0 (beside a row entirely NaN: both counters at their maxima)
        R[b, rng.integers(N), :] = np.nan
        R[b, :, rng.integers(E)] = 0.0
    for k in (4, 5):  # a scaled column with reports exactly at lo and at hi; group 5 has nothing missing
        for b in g(k):
            sc[b, js], lo[b, js], hi[b, js] = True, LO, HI
            col = LO + (HI - LO) * rng.integers(1, 8, N) / 8.0
            at = rng.random(N)
            col[at < 0.3] = LO
            col[at > 0.8] = HI
            col[0] = LO
            if k == 4 and N > 2:
                col[rng.integers(1, N)] = np.nan
            R[b, :, js] = col
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    if config == "nobounds":
        kw.update(scaled=None, lo=None, hi=None)
    elif config == "noscaled":
        kw["scaled"] = np.zeros_like(sc)
    elif config == "allscaled":
        kw["scaled"] = np.ones_like(sc)
    elif config == "int":  # integer reports (0 = missing); only the crafted column stays scaled, the
        # others' truncated rescale would leave them without a present report in every round
        R = np.where(np.isnan(R), 0.0, np.trunc(R))
        only = np.zeros_like(sc)
        only[4 * GROUP:6 * GROUP, js] = True
        kw.update(scaled=only, int_dtype=True)
    return R, kw


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_%s" % s for s in SHAPES])
def test_masks_bitexact_vs_c_oracle(gpu_lib, shape, config):
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd.batched import consensus_batched

    N, E, alg = shape
    R, kw = crafted_rounds(N, E, config)
    if alg != "PCA":
        kw.update(algorithm=alg, max_components=5, variance_threshold=0.75)
    c = OC.batched(R, **kw, threads=4)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    _assert_bitexact(g, c, (shape, config),
                     must=("original", "filled", "na_row", "nas_filled", "participation_rows",
                           "participation_columns", "reporter_bonus", "author_bonus"))


NPDOT_SHAPES = [(N, E) for E in (2, 3, 5, 17, 32) for N in (1, 2, 3, 6, 50, 64)]


@pytest.mark.parametrize("shape", NPDOT_SHAPES, ids=["%dx%d" % s for s in NPDOT_SHAPES])
def test_npdot_orders_bitexact_vs_c_oracle(gpu_lib, shape):
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched

    N, E = shape
    R, sc, lo, hi, rep = synthetic.rounds(32, N, E, seed=7000 + 64 * N + E)
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    c = OC.batched(R, **kw, threads=4)
    g = _np(consensus_batched(R, filled=True, original=True, **kw))
    _assert_bitexact(g, c, shape, must=("branch", "flags", "pi_iters", "outcomes_raw", "smooth_rep"))
