"""Inputs, SPEC runs and preconditions of the workgroup round kernel's edge batteries, shared by
test_medium_edges_cpu.py (the generators' coverage, checked on the C SPEC alone) and
test_medium_edges_gpu.py (csrc/pcx_medium.hip against the SPEC, bit for bit).  Needs no GPU."""
import functools

import numpy as np

from oracle import pcx_oracle_c as OC
from pyconsensus_amd import _abi
from test_batched_masks_gpu import B as MASK_B, CONFIGS, crafted_rounds
from test_batched_pi_gpu import ITERS_IN_LOOP_SQUARING, _dyadic_reputation, side_rounds

# 65 x 33: one row past a 64-lane chunk of the median compaction, E odd (flag words straddle rows), nine
# 4 x 4 tiles with a ragged last one; 129 x 3: three row chunks (nq = 3 in the NaN rank path), a single
# tile, np.dot's tail orders; 33 x 64: fewer rows than a wave at the widest E, all 256 tile threads own a
# tile, a bitonic network of 64 slots; 100 x 50: the documented workload shape; 200 x 34: many PI_MAXIT
# rounds; 256 x 64: every counter and the LDS carve at capacity (nq = 4, a network of 256 slots)
SHAPES = [(65, 33), (129, 3), (33, 64), (100, 50), (200, 34), (256, 64)]
WAVE_SHAPES = [(7, 20), (50, 20), (63, 31), (64, 32)]  # the ragged battery's one-wave forms
CLUSTERINGS = ("hierarchical", "clusterfeck", "k-means")
ZERO_COV, SVD_FAIL, PI_MAXIT = _abi.FLAG_ZERO_COV, _abi.FLAG_SVD_FAIL, _abi.FLAG_PI_MAXIT
MUST = ("flags", "pi_iters", "branch", "components", "smooth_rep", "outcomes_final")
# the cut at which the crafted `bounds` batches leave this_rep finite in >= 3/4 of the rounds (the
# clusters are not all the same size); chosen on the SPEC, asserted by mask_preconditions
HIERARCHY_THRESHOLD = {(65, 33): 1.5, (100, 50): 1.5}


def sid(shape):
    return "%dx%d" % tuple(shape)


def _algorithm_kw(alg, nb, N, E):
    from pyconsensus_amd.batched import kmeans_draws

    kw = {} if alg == "PCA" else dict(algorithm=alg)
    if alg in ("big-five", "fixed-variance"):
        kw.update(max_components=5, variance_threshold=0.75)
    elif alg == "hierarchical":
        kw["hierarchy_threshold"] = HIERARCHY_THRESHOLD[N, E]
    elif alg == "k-means":
        kw["kmeans_init"] = kmeans_draws(nb, N, random_state=np.random.RandomState(N + E))
    elif alg == "cokurtosis":
        kw["aux_scores"] = np.random.default_rng(900 + N + E).normal(size=(nb, N))
    return kw


def _frozen(c):
    for v in c.values():
        v.setflags(write=False)
    return c


def finite_rounds(c):
    return int(np.isfinite(c["this_rep"]).all(axis=1).sum())


# ---------------------------------------------------------------- battery 1: masks
MASK_ALGS_EXTRA = ("absolute", "big-five", "fixed-variance") + CLUSTERINGS
MASK_CASES = [(s, "PCA", cfg) for s in SHAPES for cfg in CONFIGS] + \
             [(s, alg, cfg) for s in ((65, 33), (100, 50)) for alg in MASK_ALGS_EXTRA for cfg in CONFIGS]
MASK_NOFILL = [(65, 33), (256, 64)]  # filled=False, original=False: the kernel's scratch F, null outputs


def mask_id(case):
    return "%s_%s_%s" % (sid(case[0]), case[1], case[2])


@functools.lru_cache(maxsize=None)
def mask_inputs(shape, alg, config):
    N, E = shape
    R, kw = crafted_rounds(N, E, config)
    kw.update(_algorithm_kw(alg, MASK_B, N, E))
    return R, kw


@functools.lru_cache(maxsize=None)
def mask_spec(shape, alg, config):
    """The SPEC's outputs of one mask case, computed once and shared (read only)."""
    R, kw = mask_inputs(shape, alg, config)
    return _frozen(OC.batched(R, **kw, threads=8))


def mask_preconditions(shape, alg, config, c):
    assert len(c["flags"]) == MASK_B
    if alg == "hierarchical" and config == "bounds":
        assert finite_rounds(c) >= 3 * MASK_B // 4, finite_rounds(c)


# ---------------------------------------------------------------- battery 2: covariance and power-iteration exits
SIDE_B = 96
SIDE_CASES = [(s, "PCA") for s in SHAPES] + \
             [(s, alg) for s in ((65, 33), (256, 64)) for alg in ("big-five", "fixed-variance", "cokurtosis")] + \
             [(s, alg) for s in ((65, 33), (100, 50)) for alg in CLUSTERINGS]
MAXIT_SHAPES = {(100, 50), (200, 34), (256, 64)}


def side_id(case):
    return "%s_%s" % (sid(case[0]), case[1])


@functools.lru_cache(maxsize=None)
def side_inputs(shape, alg):
    N, E = shape
    R, kw, kinds = side_rounds(N, E, seed=11, nb=SIDE_B)
    kw.update(_algorithm_kw(alg, SIDE_B, N, E))
    return R, kw, kinds


@functools.lru_cache(maxsize=None)
def side_spec(shape, alg):
    R, kw, _ = side_inputs(shape, alg)
    return _frozen(OC.batched(R, **kw, threads=8))


def side_counts(c, kinds):
    """Rounds of each flagged branch: (ZERO_COV, SVD_FAIL, PI_MAXIT, degenerate rounds at or past the
    in-loop squaring, degenerate rounds below it)."""
    it = c["pi_iters"][kinds["degen"]]
    f = c["flags"]
    return (int(np.count_nonzero(f & ZERO_COV)), int(np.count_nonzero(f & SVD_FAIL)),
            int(np.count_nonzero(f & PI_MAXIT)), int(np.count_nonzero(it >= ITERS_IN_LOOP_SQUARING)),
            int(np.count_nonzero((it > 0) & (it < ITERS_IN_LOOP_SQUARING))))


def side_preconditions(shape, alg, c, kinds):
    """The SPEC itself took the exits the 96 rounds were made for."""
    N, E = shape
    ident, wide, degen = kinds["ident"], kinds["wide"], kinds["degen"]
    assert len(ident) == len(wide) == len(degen) == 32 and len(c["flags"]) == SIDE_B
    if alg != "cokurtosis":  # (cokurtosis takes no covariance: no power iteration, flags stay 0)
        assert np.all(c["flags"][ident] & ZERO_COV) and np.all(c["pi_iters"][ident] == 0)
        assert np.all(c["flags"][wide] & SVD_FAIL)
        assert np.all(c["flags"][degen] & (ZERO_COV | SVD_FAIL) == 0)
        _, _, maxit, late, early = side_counts(c, kinds)
        if shape != (129, 3):  # (E = 3 converges in 11-13 steps)
            assert late >= 8, "too few rounds reach the in-loop squaring"
            assert early >= 1, "no round stops before the in-loop squaring"
        if shape in MAXIT_SHAPES:
            assert maxit >= 1, "no round stops at the iteration cap"
    if alg == "PCA":
        assert {1, 2, 3} <= set(c["branch"].tolist()), sorted(set(c["branch"].tolist()))
        # zero scores: the reputation update's "sum == 0, add 1" bump gives every reporter 1 / N
        assert np.all(c["this_rep"][ident] == 1.0 / N)
        # NaN scores: this_rep is masked, and with it the participation columns (rep_masked)
        assert np.isnan(c["this_rep"][wide]).all() and np.all(c["participation_columns"][wide] == 1.0)
    if alg == "fixed-variance":
        assert len(set(c["components"].tolist())) > 1, set(c["components"].tolist())
    if alg in CLUSTERINGS:  # identical reporters: every distance zero, one cluster
        finite = np.isfinite(c["this_rep"][ident]).all(axis=1)
        nan = np.isnan(c["this_rep"][ident]).all(axis=1)
        assert finite.all() if alg == "clusterfeck" else nan.all(), (alg, int(finite.sum()), int(nan.sum()))


# ---------------------------------------------------------------- battery 3: weighted-median paths
MEDIAN_GROUPS = ("tie", "dominant", "zero-weight-only", "zeros-sprinkled", "one-present", "scaled-column-missing",
                 "binary-column-missing")
MEDIAN_GROUP = 8
MEDIAN_B = MEDIAN_GROUP * len(MEDIAN_GROUPS)
MEDIAN_LO, MEDIAN_HI = 0.0, 8.0
# ("absolute" at 129 x 3 on top: the NaN rank path of the outcome median with nq = 3)
MEDIAN_CASES = [(s, "PCA") for s in SHAPES] + [(s, alg) for s in ((65, 33), (256, 64))
                                               for alg in ("absolute", "clusterfeck")] + [((129, 3), "absolute")]


def median_rounds(N, E, seed=53):
    """(reports, keyword arguments, {group: round indices}): groups of eight rounds written over
    `synthetic.rounds`, the last column scaled on [0, 8] with small integer reports, each group
    steering that column's fill median (and the outcome median) into one path."""
    from pyconsensus_amd import synthetic

    R, sc, lo, hi, rep = synthetic.rounds(MEDIAN_B, N, E, seed=seed + 64 * N + E)
    sc, lo, hi = sc.copy(), lo.copy(), hi.copy()
    rng = np.random.default_rng(seed)
    js = E - 1
    sc[:, js], lo[:, js], hi[:, js] = True, MEDIAN_LO, MEDIAN_HI
    R[:, :, js] = np.where(np.isnan(R[:, :, js]), np.nan, rng.integers(1, 8, (MEDIAN_B, N)).astype(np.float64))
    groups = {name: np.arange(k * MEDIAN_GROUP, (k + 1) * MEDIAN_GROUP) for k, name in enumerate(MEDIAN_GROUPS)}
    P = 1
    while 2 * P <= N - 1:
        P *= 2
    for b in groups["tie"]:  # P present reports of weight 1 / P each, half at 2.0 and half at 6.0: the
        # walk stops exactly at the middle and averages (dyadic weights: every partial sum is exact)
        rep[b] = _dyadic_reputation(1, N)[0]
        R[b, :, js] = np.nan
        R[b, 1:P + 1, js] = np.where(np.arange(P) % 2 == 0, 2.0, 6.0)
    for b in groups["dominant"]:  # one reporter outweighs all the others together
        d, m = rng.choice(N, 2, replace=False)
        rep[b, d] = 2.0 * (rep[b].sum() - rep[b, d]) + 1.0
        R[b, d, js] = 3.0
        R[b, m, js] = np.nan
    for b in groups["zero-weight-only"]:  # the only present reports come from reporters without reputation
        z = rng.choice(N, 3, replace=False)
        rep[b, z] = 0.0
        col = np.full(N, np.nan)
        col[z] = R[b, z, js]
        col[z] = np.where(np.isnan(col[z]), 5.0, col[z])
        R[b, :, js] = col
    for b in groups["zeros-sprinkled"]:  # every third reporter without reputation, some of them present
        rep[b, ::3] = 0.0
        R[b, 1, js] = np.nan
        R[b, 0, js] = 2.0
    for b in groups["one-present"]:
        R[b, :, js] = np.nan
        R[b, rng.integers(N), js] = 4.0
    for b in groups["scaled-column-missing"]:  # np_ == 0
        R[b, :, js] = np.nan
    for b in groups["binary-column-missing"]:
        sc[b, 0], lo[b, 0], hi[b, 0] = False, 1.0, 2.0
        R[b, :, 0] = np.nan
    return R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi), groups


@functools.lru_cache(maxsize=None)
def median_inputs(shape, alg):
    N, E = shape
    R, kw, groups = median_rounds(N, E)
    kw.update(_algorithm_kw(alg, MEDIAN_B, N, E))
    return R, kw, groups


@functools.lru_cache(maxsize=None)
def median_spec(shape, alg):
    R, kw, _ = median_inputs(shape, alg)
    return _frozen(OC.batched(R, **kw, threads=8))


def median_preconditions(shape, alg, R, c, groups):
    """What each group was made for shows in the SPEC's own outputs.  (The flags are the power
    iteration's: "absolute" runs none, so the flag conditions hold for the other algorithms.)"""
    js = shape[1] - 1
    pi = alg != "absolute"
    fill = lambda b: c["filled"][b, np.isnan(R[b, :, js]), js]  # the filled cells of the crafted column
    for b in groups["tie"]:
        assert np.all(fill(b) == 0.5) and c["outcomes_final"][b, js] == 4.0, (b, fill(b)[:1], c["outcomes_final"][b, js])
    for b in groups["dominant"]:
        assert np.all(fill(b) == 0.375) and c["outcomes_final"][b, js] == 3.0, (b, fill(b)[:1], c["outcomes_final"][b, js])
    for b in groups["one-present"]:
        assert np.all(fill(b) == 0.5) and c["outcomes_final"][b, js] == 4.0, (b, fill(b)[:1], c["outcomes_final"][b, js])
    for b in groups["zero-weight-only"]:
        assert np.all(np.isnan(fill(b)))
    if pi:
        assert np.all(c["flags"][groups["zero-weight-only"]] & SVD_FAIL)
        assert np.all(c["flags"][groups["scaled-column-missing"]] & SVD_FAIL)
    for name in ("zeros-sprinkled", "binary-column-missing"):
        assert np.all(c["flags"][groups[name]] == 0), (name, c["flags"][groups[name]])
        assert not np.isnan(c["smooth_rep"][groups[name]]).any(), name


# ---------------------------------------------------------------- battery 4: the same rounds, ragged
RAGGED_TAKE = 24  # rounds of each group (the median groups hold eight: all of them)
# ("absolute" on top: its reputations stay finite beside a NaN-filled column, so the one-wave kernel's
# outcome median ranks NaN values; under PCA and big-five those rounds' reputations are NaN)
RAGGED_ALGS = ("PCA", "big-five", "absolute")


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    """Per one-wave shape the side and median batches, and the shuffled launch order as (shape
    index, battery, round of that batch)."""
    per, order = [], []
    for k, (N, E) in enumerate(WAVE_SHAPES):
        Rs, kws, kinds = side_rounds(N, E, seed=11, nb=SIDE_B)
        Rm, kwm, groups = median_rounds(N, E)
        per.append(dict(side=(Rs, kws), median=(Rm, kwm)))
        order += [(k, "side", int(b)) for v in kinds.values() for b in v[:RAGGED_TAKE]]
        order += [(k, "median", int(b)) for v in groups.values() for b in v[:RAGGED_TAKE]]
    np.random.default_rng(20261019).shuffle(order)
    return per, [(int(k), str(bat), int(b)) for k, bat, b in order]


@functools.lru_cache(maxsize=None)
def ragged_spec(alg):
    """The SPEC's outputs of the ragged battery's batches, each run on its own shape."""
    per, _ = ragged_inputs()
    out = []
    for (N, E), d in zip(WAVE_SHAPES, per):
        out.append({bat: _frozen(OC.batched(R, **kw, threads=8, **_algorithm_kw(alg, len(R), N, E)))
                    for bat, (R, kw) in d.items()})
    return out


def ragged_preconditions(alg):
    """One launch holds rounds that leave the power iteration at once beside rounds that run into
    the in-loop squarings and to the cap ("absolute" runs no power iteration: NaN-filled columns
    beside finite reputations instead)."""
    per, order = ragged_inputs()
    ref = ragged_spec(alg)
    if alg == "absolute":
        n = 0
        for k, bat, b in order:
            if bat == "median":
                js = WAVE_SHAPES[k][1] - 1
                n += bool(np.isnan(ref[k][bat]["filled"][b, :, js]).any() and np.isfinite(ref[k][bat]["smooth_rep"][b]).all())
        assert n >= 4 * 2 * MEDIAN_GROUP, n
        return
    flags = np.array([ref[k][bat]["flags"][b] for k, bat, b in order])
    iters = np.array([ref[k][bat]["pi_iters"][b] for k, bat, b in order])
    assert np.count_nonzero(flags & ZERO_COV) >= 4 * RAGGED_TAKE
    assert np.count_nonzero(flags & SVD_FAIL) >= 4 * RAGGED_TAKE
    assert np.count_nonzero(flags & PI_MAXIT) >= 1
    assert np.count_nonzero(iters >= ITERS_IN_LOOP_SQUARING) >= 8
    assert np.count_nonzero(flags == 0) >= len(order) // 4
