"""Tall rounds in ragged batches and simulator studies without a GPU: the new
entries exist under ABI 9, pcx_ragged_plan_tall's figures re-derived in Python, its refusals by round and
reason, the tall study's check by cell, the old entries' limits and words untouched, the coverage of
the inputs that test_tall_ragged_gpu.py runs (asserted on the plan and the SPEC alone), and the study's
mcc at 1024 reporters against exact integer arithmetic."""
import ctypes as C
import math

import numpy as np
import pytest

import tall_cases as T
import tall_ragged_cases as G
from pyconsensus_amd import _abi

NEW = ("pcx_ragged_plan_tall", "pcx_consensus_ragged_tall_f64", "pcx_sim_study_tall_check", "pcx_sim_sweep_plan_tall",
       "pcx_simulate_study_tall_f64", "pcx_simulate_tall_f64")


def _lib():
    from pyconsensus_amd import _lib

    return _lib.lib()


def _sim():
    import importlib

    return importlib.import_module("pyconsensus_amd.simulate")


def _sets(*qs):
    return [dict(G.DEFAULTS, **q) for q in qs]


def test_new_entries_exist_under_abi_9():
    h = _lib()
    assert h.pcx_abi_version() == 9
    for name in NEW:
        assert hasattr(h, name), name


# ------------------------------------------------------------------ the plan
HAND = [((257, 5), 0), ((6, 4), 0), ((1024, 64), 0), ((100, 50), 0), ((513, 33), 1), ((50, 20), 2), ((300, 64), 3),
        ((256, 64), 0), ((1024, 1), 1), ((65, 3), 2), ((64, 32), 3), ((300, 40), 4)]
HAND_SETS = _sets({}, {"algorithm": "absolute"}, {"algorithm": "hierarchical"}, {"algorithm": "big-five"},
                  {"algorithm": "fixed-variance"})


def _segment(N, E, alg):
    """A small round's launch segment, from the public plan queries of one round."""
    from pyconsensus_amd.batched import ragged_plan

    if N <= 64 and E <= 32:
        return ("wave", 2 if alg in ("hierarchical", "clusterfeck") else 1 if alg in ("big-five", "fixed-variance") else 0)
    counts = ragged_plan([(N, E)], alg, wide=True)[1]
    return ("workgroup", alg in ("hierarchical", "clusterfeck"), counts.index(1))


def test_plan_tall_figures_rederived():
    from pyconsensus_amd.batched import ragged_plan_tall

    shapes, of = [s for s, _ in HAND], [q for _, q in HAND]
    totals, n_launches, n_tall, lds = ragged_plan_tall(shapes, HAND_SETS, of)
    assert totals == (sum(n for n, _ in shapes), sum(e for _, e in shapes), sum(n * e for n, e in shapes))
    tall = [(s, HAND_SETS[q]["algorithm"]) for s, q in HAND if s[0] > 256]
    assert n_tall == len(tall) == 6
    h = _lib()
    each = [h.pcx_tall_lds_bytes(N, E, _abi.ALGORITHMS[a]) for (N, E), a in tall]
    assert all(0 < x <= T.LDS_LIMIT for x in each)
    assert lds == max(each) == h.pcx_tall_lds_bytes(1024, 64, _abi.ALGORITHMS["PCA"])
    small = {_segment(N, E, HAND_SETS[q]["algorithm"]) for (N, E), q in HAND if N <= 256}
    assert n_launches == len(small) + 1
    assert len(small) >= 5  # two one-wave groups, the clustering and the plain workgroup instantiation


def test_plan_tall_without_a_tall_round_is_plan_params():
    from pyconsensus_amd.batched import ragged_plan_params, ragged_plan_tall

    small = [(s, q) for s, q in HAND if s[0] <= 256]
    shapes, of = [s for s, _ in small], [q for _, q in small]
    totals, n_launches, n_tall, lds = ragged_plan_tall(shapes, HAND_SETS, of)
    assert (totals, n_launches) == ragged_plan_params(shapes, HAND_SETS, of)
    assert (n_tall, lds) == (0, 0)
    assert ragged_plan_tall([], HAND_SETS, []) == ((0, 0, 0), 0, 0, 0)


def _plan_tall_raw(shapes, sets, of):
    from pyconsensus_amd.batched import _params_array

    sh = np.asarray(shapes, dtype=np.int32).reshape(-1, 2)
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    of = np.ascontiguousarray(of, dtype=np.int32)
    arr = _params_array(sets)
    bad_r, bad_p = C.c_int64(-2), C.c_int64(-2)
    h = _lib()
    rc = h.pcx_ragged_plan_tall(len(sh), n.ctypes.data, e.ctypes.data, len(sets), C.cast(arr, C.c_void_p),
                                of.ctypes.data, None, None, C.byref(bad_r), C.byref(bad_p), None, None)
    return rc, bad_r.value, bad_p.value, h.pcx_last_error().decode()


@pytest.mark.parametrize("shapes,of,round_,words", [
    ([(50, 20), (1025, 4)], [0, 0], 1, ("round 1 is 1025 x 4", "[1, 1024] x [1, 64]")),
    ([(300, 65)], [0], 0, ("round 0 is 300 x 65", "[1, 1024] x [1, 64]")),
    ([(50, 20), (256, 64), (300, 10)], [0, 1, 1], 2, ("round 2 is 300 x 10 under hierarchical", "256 reporters")),
    ([(1024, 64)], [2], 0, ("round 0 is 1024 x 64 under big-five", "does not fit")),
    ([(300, 10), (300, 10)], [0, 3], 1, ("round 1 has param_of 3", "[0, 3)")),
], ids=["1025x4", "300x65", "hierarchical", "big-five-1024x64", "param_of"])
def test_plan_tall_refusals_name_round_and_reason(shapes, of, round_, words):
    sets = _sets({}, {"algorithm": "hierarchical"}, {"algorithm": "big-five"})
    rc, bad_r, bad_p, msg = _plan_tall_raw(shapes, sets, of)
    assert rc == -1 and bad_r == round_ and bad_p == -1, (rc, bad_r, bad_p, msg)
    for w in words:
        assert w in msg, msg


def test_plan_tall_refuses_a_kmeans_set():
    rc, bad_r, bad_p, msg = _plan_tall_raw([(300, 10)], _sets({}, {"algorithm": "k-means"}), [0])
    assert rc == -1 and bad_r == -1 and bad_p == 1 and "parameter set 1" in msg and "k-means" in msg, msg


def test_old_entries_keep_their_limits_and_words():
    from pyconsensus_amd._lib import PcxError
    from pyconsensus_amd.batched import ragged_plan, ragged_plan_kmeans, ragged_plan_params

    sweep_plan = _sim().sweep_plan
    for call in (lambda: ragged_plan_params([(257, 4)], _sets({}), [0]), lambda: ragged_plan([(257, 4)], wide=True),
                 lambda: ragged_plan_kmeans([(257, 4)], _sets({}), [0], 2)):
        with pytest.raises(PcxError, match=r"round 0 is 257 x 4; a round must be within \[1, 256\] x \[1, 64\]"):
            call()
    with pytest.raises(PcxError, match=r"cell 0: is 257 x 4; a cell's rounds must be within \[1, 256\] x \[1, 64\]"):
        sweep_plan([G.cell(2, 257, 4, 1)])


# ------------------------------------------------------------------ the study's check
def test_study_tall_check_by_cell():
    from pyconsensus_amd._lib import PcxError

    M = _sim()
    cells = [G.cell(4, 50, 20, 1), G.cell(2, 1024, 64, 2)]
    totals, counts, lds = M.sweep_plan(cells, tall=True)
    assert list(totals) == [6, 4 * 50 + 2 * 1024, 4 * 20 + 2 * 64, 4 * 50 * 20 + 2 * 1024 * 64]
    assert list(counts) == [4, 0, 0, 0]  # the tall cell counts in no launch class
    assert M.study_check(cells, None, tall=True) is None
    for alg, why in (("big-five", "does not fit"), ("clusterfeck", "256 reporters")):
        with pytest.raises(PcxError, match=r"cell 1: is 1024 x 64 under %s; .*%s" % (alg, why)):
            M.sweep_plan(cells, tall=True, algorithm=alg)
        with pytest.raises(PcxError, match=r"cell 1: is 1024 x 64 under %s" % alg):  # as the cell's own set
            M.sweep_plan([cells[0], dict(cells[1], algorithm=alg)], tall=True)
    with pytest.raises(PcxError, match="cokurtosis is not simulated"):
        M.sweep_plan(cells, tall=True, algorithm="cokurtosis")
    with pytest.raises(PcxError, match="cell 1: cokurtosis is not simulated"):
        M.sweep_plan([cells[0], dict(cells[1], algorithm="cokurtosis")], tall=True)
    with pytest.raises(PcxError, match=r"cell 0: is 1025 x 4; a cell's rounds must be within \[1, 1024\] x \[1, 64\]"):
        M.sweep_plan([G.cell(1, 1025, 4, 1)], tall=True)
    with pytest.raises(PcxError, match="cell 1: has 2 rounds, its base cell 0 has 4"):
        M.study_check(cells, [-1, 0], tall=True)
    # without a tall cell: the figures of the call without `tall`
    small = [G.cell(4, 50, 20, 1), G.cell(2, 256, 64, 2)]
    for a, b in zip(M.sweep_plan(small, tall=True), M.sweep_plan(small)):
        assert list(a) == list(b)


def test_tall_and_kmeans_restarts_exclude_each_other(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)  # (the ValueError comes before any device use)
    M = _sim()
    from pyconsensus_amd.batched import consensus_ragged

    with pytest.raises(ValueError, match="tall=True"):
        M.sweep([G.cell(2, 300, 4, 1)], tall=True, kmeans_restarts=2)
    with pytest.raises(ValueError, match="tall=True"):
        M.study([G.cell(2, 300, 4, 1)], tall=True, kmeans_restarts=2)
    with pytest.raises(ValueError, match="tall=True"):
        M.simulate(2, 300, 4, tall=True, kmeans_restarts=2)
    with pytest.raises(ValueError, match="tall=True"):
        consensus_ragged([np.ones((300, 4))], tall=True, kmeans_restarts=2)


# ------------------------------------------------------------------ coverage of the GPU tests' inputs
def test_mixed_call_reaches_every_plan_branch():
    plans = {s: T.plan(*s) for s in G.MIX_SHAPES if G.is_tall(s)}
    assert len(plans) == 7 and all(p is not None for p in plans.values()), plans
    assert plans[257, 5][0] == 4 and plans[513, 33][0] == 2 and plans[1024, 64][0] == 1  # median waves
    assert plans[257, 5][2] == 1 and plans[640, 62][2] == 2 and plans[1024, 64][2] == 4  # np.dot chunks
    assert plans[1024, 1][2] == 1 and plans[1024, 1][1] >= 4
    h = _lib()
    lds = {s: h.pcx_tall_lds_bytes(s[0], s[1], 0) for s in plans}
    # the launch's LDS is one round's (640 x 62's); every other round carves less, each a figure of its own
    assert max(lds.values()) == lds[640, 62] > lds[1024, 64] and len(set(lds.values())) == len(lds)
    for s, q in G.SETS_CASES:
        assert T.plan(s[0], s[1], q.get("algorithm", "PCA")) is not None, (s, q)


def test_mixed_call_spec_runs_finite_rounds():
    """The SPEC's own rounds of the mixed call are ordinary ones: power iteration ran, a rank-rule
    branch was taken, no failure flag."""
    for b, s in enumerate(G.MIX_SHAPES):
        if not G.is_tall(s):
            continue
        c = G.mix_spec(b)
        assert c["flags"][0] & (T.ZERO_COV | T.SVD_FAIL) == 0 and c["pi_iters"][0] > 0, (s, c["flags"], c["pi_iters"])
        assert 1 <= c["branch"][0] <= 4 and np.isfinite(c["smooth_rep"]).all(), s


def test_set_rounds_on_the_spec():
    comps = []
    for b, (s, q) in enumerate(G.SETS_CASES):
        c = G.sets_spec(b)
        assert np.isfinite(c["smooth_rep"]).all(), (s, q)
        if q.get("algorithm") == "absolute":
            assert c["branch"][0] == 5 and c["pi_iters"][0] == 0  # PCX_BRANCH_NONE: no rank rule, no PCA
        comps.append(int(c["components"][0]))
    assert comps[0] == comps[1] == comps[2] == comps[4] == -1 and comps[3] > 1  # (fixed-variance alone counts)


def test_batteries_reach_their_exits_on_the_spec():
    """The crafted masks, the side battery and the NaN rank path (nine elements a lane at 513 reporters:
    more than the four of the 256-reporter kernel) are in the batches that the ragged entry runs."""
    R, kw = T.mask_inputs(G.BATTERY_SHAPE, "bounds")
    T.mask_preconditions(G.BATTERY_SHAPE, "bounds", R, kw, T.mask_spec(G.BATTERY_SHAPE, "bounds"))
    R, kw, kinds = T.side_inputs(G.BATTERY_SHAPE)
    T.side_preconditions(G.BATTERY_SHAPE, T.side_spec(G.BATTERY_SHAPE), kinds)
    R, kw, groups = T.nan_inputs()
    assert R.shape[1:] == G.BATTERY_SHAPE and -(-R.shape[1] // 64) == 9  # a wave's lanes hold nine reporters each
    T.nan_preconditions(R, T.nan_spec(), groups)


# ------------------------------------------------------------------ mcc at 1024 reporters
@pytest.mark.parametrize("tp,fn,fp,tn", [(512, 0, 0, 512), (256, 256, 256, 256), (1, 2, 3, 1018), (511, 1, 1, 511),
                                         (300, 212, 100, 412), (1023, 0, 1, 0), (333, 333, 179, 179), (0, 512, 512, 0)])
def test_mcc_is_exact_at_1024_reporters(tp, fn, fp, tn):
    """TP + FP + FN + TN = 1024: every product of the mcc is an integer below 2^53, so the detail metric
    is the correctly rounded quotient of exact integers."""
    N = tp + fn + fp + tn
    assert N == 1024
    liar = np.array([1] * (tp + fn) + [0] * (fp + tn), dtype=np.uint8)[None]
    punished = np.array([1] * tp + [0] * fn + [1] * fp + [0] * tn, dtype=bool)
    old = np.full((1, N), 1.0 / N)
    smooth = np.where(punished, 0.5 / N, 1.0 / N)[None]
    perm = np.random.default_rng(tp + 3 * fp).permutation(N)
    liar, old, smooth = liar[:, perm], old[:, perm], smooth[:, perm]
    rounds = dict(scaled=np.zeros((1, 1), np.uint8), lo=np.zeros((1, 1)), hi=np.ones((1, 1)), truth=np.ones((1, 1)),
                  liar=liar)
    d = _sim().detail_host(rounds, old, smooth, np.ones((1, 1)))[0]
    assert tuple(d[6:10]) == (tp, fn, fp, tn)
    num, p, q = tp * tn - fp * fn, (tp + fp) * (tp + fn), (tn + fp) * (tn + fn)
    assert max(tp * tn, fp * fn, p, q, p * q) < 2 ** 53
    if p * q == 0:
        assert np.isnan(d[10])
        return
    want = num / math.sqrt(p * q)  # (exact operands: one correctly rounded sqrt, one correctly rounded division)
    assert d[10] == want
    root = math.isqrt(p * q)
    if root * root == p * q and num % root == 0:
        assert d[10] == num // root
