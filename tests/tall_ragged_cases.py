"""Inputs and SPEC runs of the tall rounds in ragged batches and simulator studies (DESIGN.md 5.5.3 /
5.4.5: csrc/pcx_tall_ragged.hip, consensus_ragged(..., tall=True), sweep / study / simulate(...,
tall=True)), shared by test_tall_ragged_cpu.py, test_tall_ragged_gpu.py and test_tall_sim_gpu.py.  The
reference of every tall round is the SPEC built for 1024 reporters (tall_cases.spec); one round per
tall shape, since its weighted medians over 1024 reporters are slow.  Needs no GPU.  No test here."""
import functools

import numpy as np

import tall_cases as T
from sim_sweep_cases import cell

bits_equal = T.bits_equal
EVERY = ("old_rep", "this_rep", "smooth_rep", "scores", "na_row", "participation_rows", "relative_part",
         "reporter_bonus", "adj_first_loadings", "outcomes_raw", "outcomes_adjusted", "outcomes_final", "certainty",
         "consensus_reward", "nas_filled", "participation_columns", "author_bonus", "participation", "avg_certainty",
         "branch", "flags", "pi_iters", "components")
DEFAULTS = dict(algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
                hierarchy_threshold=0.5, cluster_threshold=None)

# ------------------------------------------------------------------ the mixed call (PCA)
# tall_cases.SYNTH_SHAPES (four, two and one median waves; one, two and four np.dot chunks; E == 1; the
# deepest pairwise tree) and 300 x 50, with two one-wave and two workgroup rounds between them: the
# launch's LDS is its largest plan's (the 640 x 62 round's: 157,008 B against the 1024 x 64 round's
# 156,688 B), and every other tall round carves its own plan out of it
MIX_SHAPES = [(257, 5), (6, 4), (1024, 64), (100, 50), (513, 33), (50, 20), (640, 62), (256, 64), (1023, 7), (1024, 1),
              (300, 50)]


def is_tall(shape):
    return shape[0] > 256


@functools.lru_cache(maxsize=None)
def round_inputs(shape, seed):
    """One synthetic round as a batch of one: (R (1,N,E), keywords with (1, .) arrays)."""
    from pyconsensus_amd import synthetic

    N, E = shape
    R, sc, lo, hi, rep = synthetic.rounds(1, N, E, seed=seed)
    return R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi)


def mix_rounds():
    return [round_inputs(s, 3100 + k) for k, s in enumerate(MIX_SHAPES)]


def ragged_args(rounds, idx=None):
    """consensus_ragged's (reports, keywords) of a list of one-round batches (`idx`: a subset, in order)."""
    idx = range(len(rounds)) if idx is None else idx
    reports = [rounds[b][0][0] for b in idx]
    kw = {k: [rounds[b][1][k][0] for b in idx] for k in ("reputation", "scaled", "lo", "hi")}
    return reports, kw


@functools.lru_cache(maxsize=None)
def mix_spec(b):
    """The SPEC's outputs of round b of the mixed call (a tall round), as a batch of one."""
    R, kw = mix_rounds()[b]
    return T._frozen(T.spec(R, **kw))


# ------------------------------------------------------------------ per-round parameter sets
SETS_CASES = [
    ((513, 33), {"alpha": 0.2, "catch_tolerance": 0.15}),
    ((513, 33), {"algorithm": "absolute", "alpha": 0.3, "catch_tolerance": 0.2}),
    ((300, 64), {"algorithm": "big-five", "max_components": 5, "alpha": 0.05, "catch_tolerance": 0.12}),
    ((300, 40), {"algorithm": "fixed-variance", "variance_threshold": 0.75, "alpha": 0.4, "catch_tolerance": 0.05}),
    ((513, 33), {"algorithm": "cokurtosis", "alpha": 0.25, "catch_tolerance": 0.08}),
]


def sets_rounds():
    return [round_inputs(s, 3200 + k) for k, (s, _) in enumerate(SETS_CASES)]


def sets_aux():
    """aux_scores per round: the cokurtosis round's scores, None elsewhere."""
    return [np.random.default_rng(3300 + k).normal(size=s[0]) if q.get("algorithm") == "cokurtosis" else None
            for k, (s, q) in enumerate(SETS_CASES)]


@functools.lru_cache(maxsize=None)
def sets_spec(b):
    R, kw = sets_rounds()[b]
    q = dict(SETS_CASES[b][1])
    aux = sets_aux()[b]
    if aux is not None:
        q["aux_scores"] = aux[None]
    return T._frozen(T.spec(R, **kw, **q))


# ------------------------------------------------------------------ batteries through the ragged entry
BATTERY_SHAPE = (513, 33)


def battery_args(R, kw):
    """An equal-shape batch (R (B,N,E), tall_cases keywords) as consensus_ragged's lists and keywords."""
    kw = dict(kw)
    lists = {}
    for k in ("reputation", "scaled", "lo", "hi"):
        v = kw.pop(k, None)
        if v is not None:
            v = np.asarray(v)
            lists[k] = [v[b] for b in range(len(R))] if v.ndim == 2 else [v] * len(R)
    return [R[b] for b in range(len(R))], dict(lists, **kw)


def assert_round(g, c, b, what, must=EVERY):
    """Round outputs `g` (ragged_round of a host result) against row b of the SPEC's batch outputs `c`."""
    assert set(must) <= set(g) <= set(c), (what, set(must) - set(g), set(g) - set(c))
    for k, v in g.items():
        same = bits_equal(np.asarray(v), np.asarray(c[k][b]).reshape(np.shape(v)))
        assert np.all(same), (what, k, int(np.size(same) - np.count_nonzero(same)))


# ------------------------------------------------------------------ the simulator's cells
# three tall cells (four, two and one median waves) and two small ones; cells 1 and 4 share a seed
STUDY_T = 2
STUDY_CELLS = [cell(3, 257, 5, 71, na_frac=0.15, scaled_frac=0.4), cell(2, 513, 33, 72, na_frac=0.1, scaled_frac=0.25),
               cell(2, 1024, 64, 73, na_frac=0.05, scaled_frac=0.1), cell(4, 50, 20, 74, na_frac=0.1, scaled_frac=0.25),
               cell(3, 100, 50, 72, na_frac=0.1, scaled_frac=0.3)]
PAIR_CELLS = [dict(cell(6, 512, 20, 81), algorithm="PCA"), dict(cell(6, 512, 20, 81), algorithm="absolute")]
TWIN_CELL = cell(3, 1024, 3, 91, na_frac=0.2, scaled_frac=0.5)
SIM_FIELDS = ("rounds", "reporters", "events")
