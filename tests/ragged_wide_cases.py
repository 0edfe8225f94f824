"""Inputs, SPEC runs and preconditions of the wide ragged batches (rounds up to 256 x 64 in one
call: pcx_consensus_ragged_wide_f64), shared by test_ragged_wide_cpu.py (the plan, and the inputs'
preconditions on the C SPEC alone) and test_ragged_wide_gpu.py (the kernels against the SPEC, bit for
bit).  Needs no GPU.  The SPEC runs are computed once per process and shared read-only."""
import copy
import functools

import numpy as np

import golden_cases as G
import medium_edges as M
import parity as P
from test_batched_pi_gpu import side_rounds

ALGORITHMS = ["PCA", "absolute", "big-five", "fixed-variance", "cokurtosis", "hierarchical", "clusterfeck"]
# where an offset, a pitch, a carve, the wave / workgroup boundary or a launch-class boundary shows
MIX_SHAPES = [(1, 1), (50, 20), (64, 32), (65, 1), (1, 33), (65, 33), (64, 33), (129, 3), (33, 64), (2, 64),
              (100, 50), (200, 34), (256, 1), (256, 64)]
MIX_ROUNDS = 256
# static LDS of the workgroup kernel (profiles/ragged_wide/resources.txt), the LDS allocation unit and
# a CU's LDS, the kernel's rounds per CU by registers
STATIC_LDS, LDS_UNIT, CU_LDS, VGPR_ROUNDS = 4288, 1280, 160 * 1024, 3


def is_wave(N, E):
    return N <= 64 and E <= 32


def launch_class(N, E, alg):
    """The issue's formula, from pcx_medium_lds_bytes: min(3, floor(160 KiB / (dynamic + static LDS
    rounded up to the allocation unit)))."""
    from pyconsensus_amd import _abi, _lib

    dyn = _lib.lib().pcx_medium_lds_bytes(N, E, _abi.ALGORITHMS[alg])
    assert dyn > 0, (N, E, alg)
    wg = -(-(dyn + STATIC_LDS) // LDS_UNIT) * LDS_UNIT
    return min(VGPR_ROUNDS, CU_LDS // wg)


def alg_kw(alg):
    kw = dict(algorithm=alg)
    if alg in ("big-five", "fixed-variance"):
        kw.update(max_components=5, variance_threshold=0.75)  # (5 > E for four of the shapes: capped per round)
    return kw


def _frozen(c):
    for v in c.values():
        v.setflags(write=False)
    return c


# ---------------------------------------------------------------- the seeded mix
@functools.lru_cache(maxsize=None)
def mix():
    """Per shape its rounds (synthetic.rounds) and, per round of the shuffled order, (shape index,
    index among that shape's rounds)."""
    from pyconsensus_amd import synthetic

    rng = np.random.default_rng(20261020)
    which = np.concatenate([np.arange(len(MIX_SHAPES)), rng.integers(0, len(MIX_SHAPES), MIX_ROUNDS - len(MIX_SHAPES))])
    rng.shuffle(which)
    per, order, seen = [], [], [0] * len(MIX_SHAPES)
    for k, (N, E) in enumerate(MIX_SHAPES):
        R, sc, lo, hi, rep = synthetic.rounds(int(np.sum(which == k)), N, E, seed=1700 + k)
        aux = np.random.default_rng(1900 + k).normal(size=(R.shape[0], N))
        per.append(dict(R=R, scaled=sc, lo=lo, hi=hi, reputation=rep, aux=aux))
    for k in which:
        order.append((int(k), seen[k]))
        seen[k] += 1
    return per, order


@functools.lru_cache(maxsize=None)
def mix_spec(alg):
    """The C SPEC's outputs of the mix's rounds, one run per shape."""
    from oracle import pcx_oracle_c as OC

    ref = []
    for d in mix()[0]:
        kw = alg_kw(alg)
        if alg == "cokurtosis":
            kw["aux_scores"] = d["aux"]
        ref.append(_frozen(OC.batched(d["R"], d["scaled"], d["lo"], d["hi"], d["reputation"], threads=8, **kw)))
    return ref


def mix_call(order, alg):
    """(positional arguments, keyword arguments) of consensus_ragged for the mix's rounds `order`."""
    per, _ = mix()
    pick = lambda key: [per[k][key][i] for k, i in order]
    kw = alg_kw(alg)
    if alg == "cokurtosis":
        kw["aux_scores"] = pick("aux")
    return (pick("R"), pick("reputation"), pick("scaled"), pick("lo"), pick("hi")), kw


# ---------------------------------------------------------------- side branches and median paths
SIDE_SHAPES = [(65, 33), (100, 50), (256, 64), (7, 20), (64, 32)]
SIDE_TAKE = 12  # rounds of each kind or group (the median groups hold eight: all of them)
SIDE_ALGS = ("PCA", "big-five", "absolute", "hierarchical")


def _spread(v):
    """SIDE_TAKE of a kind's rounds, evenly over the kind (the degenerate-eigenvalue rounds grow
    harder with their index: the ones that reach the iteration cap are in the second half)."""
    v = np.asarray(v)
    return v if len(v) <= SIDE_TAKE else v[np.round(np.linspace(0, len(v) - 1, SIDE_TAKE)).astype(int)]


def _take(R, kw, idx):
    return R[idx], {k: v[idx] for k, v in kw.items()}


@functools.lru_cache(maxsize=None)
def side_inputs():
    """Per shape the rounds taken from medium_edges' side and median batteries (and, for the side
    rounds, the kinds' indices among those taken), and the shuffled launch order as (shape index,
    battery, round among those taken)."""
    per, order = [], []
    for k, (N, E) in enumerate(SIDE_SHAPES):
        Rs, kws, kinds = side_rounds(N, E, seed=11, nb=M.SIDE_B)
        Rm, kwm, groups = M.median_rounds(N, E)
        si = np.concatenate([_spread(v) for v in kinds.values()])
        mi = np.concatenate([_spread(v) for v in groups.values()])
        at, sub = 0, {}
        for name, v in kinds.items():
            n = len(_spread(v))
            sub[name] = np.arange(at, at + n)
            at += n
        per.append(dict(side=_take(Rs, kws, si), median=_take(Rm, kwm, mi), kinds=sub))
        order += [(k, "side", b) for b in range(len(si))] + [(k, "median", b) for b in range(len(mi))]
    np.random.default_rng(20261020).shuffle(order)
    return per, [(int(k), str(bat), int(b)) for k, bat, b in order]


def side_alg_kw(alg):
    kw = {} if alg == "PCA" else dict(algorithm=alg)
    if alg == "big-five":
        kw["max_components"] = 5
    return kw


@functools.lru_cache(maxsize=None)
def side_spec(alg):
    """The SPEC's outputs of the taken rounds, each batch run on its own shape."""
    from oracle import pcx_oracle_c as OC

    run = lambda R, kw: _frozen(OC.batched(R, **kw, threads=8, **side_alg_kw(alg)))
    return [{bat: run(*d[bat]) for bat in ("side", "median")} for d in side_inputs()[0]]


def side_preconditions(alg):
    """medium_edges.ragged_preconditions' thresholds, scaled to the rounds taken here: five shapes
    of SIDE_TAKE rounds per side kind (there: four shapes of 24), all eight rounds of a median group."""
    per, order = side_inputs()
    ref = side_spec(alg)
    shapes = len(SIDE_SHAPES)
    if alg == "absolute":  # no power iteration: NaN-filled columns beside finite reputations instead
        n = 0
        for k, bat, b in order:
            if bat == "median":
                js = SIDE_SHAPES[k][1] - 1
                c = ref[k][bat]
                n += bool(np.isnan(c["filled"][b, :, js]).any() and np.isfinite(c["smooth_rep"][b]).all())
        assert n >= shapes * 2 * M.MEDIAN_GROUP, n
        return
    counts = np.array([M.side_counts(ref[k]["side"], per[k]["kinds"]) for k in range(shapes)]).sum(axis=0)
    zero_cov, svd_fail, maxit, late, _ = (int(x) for x in counts)
    assert zero_cov >= shapes * SIDE_TAKE and svd_fail >= shapes * SIDE_TAKE, (zero_cov, svd_fail)
    assert maxit >= 1, "no round stops at the iteration cap"
    assert late >= 8 * (shapes * SIDE_TAKE) // (4 * M.RAGGED_TAKE), late  # (there: 8 of 4 x 24 degenerate rounds)
    flags = np.array([ref[k][bat]["flags"][b] for k, bat, b in order])
    assert np.count_nonzero(flags == 0) >= len(order) // 4


# ---------------------------------------------------------------- consensus_many
README = dict(reports=[[0.2, 0.7, 1, 1], [0.3, 0.5, 1, 1], [0.1, 0.7, 1, 1],
                       [0.5, 0.7, 2, 1], [0.1, 0.2, 2, 2], [0.1, 0.2, 2, 2]],
              reputation=[1, 2, 10, 9, 4, 2],
              event_bounds=[{"scaled": True, "min": 0.1, "max": 0.5}, {"scaled": True, "min": 0.2, "max": 0.7},
                            {"scaled": False, "min": 1, "max": 2}, {"scaled": False, "min": 1, "max": 2}])
MANY_GOLDENS = 6
MANY_WIDE = [(70, 5, 11), (100, 50, 12), (256, 64, 13)]  # (N, E, synthetic.matrix seed)


def many_problems():
    """Fresh copies (Oracle rescales a caller's float matrix in place) of the README example, six
    goldens of at most 64 x 32 taken kind by kind, and a 70 x 5, a 100 x 50 and a 256 x 64 problem
    with bounds and reputation."""
    from pyconsensus_amd import synthetic

    ps = [copy.deepcopy(README)]
    kinds = {}
    for name, case in sorted(list(G.kat().items()) + list(G.mixed().items())):
        N, E = case["in_reports"].shape
        if name not in P.EXCLUDED and name not in P.KNOWN_MISMATCH["exact"] and N <= 64 and E <= 32:
            kinds.setdefault((bool(case["in_has_bounds"]), bool(case["in_has_rep"]), bool(case["in_int_dtype"])),
                             []).append(case)
    picked = [v[i] for i in range(MANY_GOLDENS) for _, v in sorted(kinds.items()) if i < len(v)][:MANY_GOLDENS]
    assert len(picked) == MANY_GOLDENS
    for case in picked:
        kw = G.oracle_args(case)
        kw.pop("algorithm")
        ps.append(kw)
    for N, E, seed in MANY_WIDE:
        R, sc, lo, hi, rep = synthetic.matrix(N, E, seed=seed)
        ps.append(dict(reports=R, event_bounds=synthetic.bounds_list(sc, lo, hi), reputation=rep))
    return ps


def abi_named(flat):
    """A golden_cases.flat_result dict under the ABI's names (parity.compare's `ours`)."""
    return {P.ABI_NAME[k]: v for k, v in flat.items() if k in P.ABI_NAME}
