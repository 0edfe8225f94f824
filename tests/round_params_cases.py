"""Cases and helpers of the per-round consensus parameters, shared by
test_round_params_cpu.py and test_round_params_gpu.py: the mixed ragged batch and its eight parameter
sets, the study's cells and their five sets.  Needs no GPU.  No test here."""
import functools

import numpy as np

import sim_sweep_cases as W

cell = W.cell
same_bits = W.same_bits

PARAM_KEYS = ("algorithm", "catch_tolerance", "alpha", "max_components", "variance_threshold",
              "hierarchy_threshold", "cluster_threshold")

# ------------------------------------------------------------------ the mixed ragged batch
# 1 x 1 and an odd small shape, the one-wave limit, just past it each way, and two larger workgroup
# rounds: with the eight sets below they reach the one-wave kernel's three instantiation groups and
# the workgroup kernel's three launch classes in both of its instantiations (test_round_params_cpu.py
# checks that on the plan)
MIX_SHAPES = [(1, 1), (3, 33), (64, 32), (65, 3), (5, 3), (100, 50), (256, 64)]
MIX_ROUNDS = 32
MIX_SETS = [
    {},                                                    # PCA at the defaults
    {"alpha": 0.3, "catch_tolerance": 0.2},                # PCA
    {"algorithm": "absolute"},
    {"algorithm": "big-five", "max_components": 5},        # above E = 3: capped on the device
    {"algorithm": "fixed-variance", "variance_threshold": 0.7},
    {"algorithm": "cokurtosis"},
    {"algorithm": "hierarchical", "hierarchy_threshold": 0.7},
    {"algorithm": "clusterfeck"},                          # the default threshold: log10(E_b) / 1.77 per round
]


def mix_shape_index(b):
    """Round b's shape: 7 shapes against 8 sets, so shape k meets the sets k, k - 1, .. k - 4 (mod 8)
    and two neighbouring rounds never share a set."""
    return b % len(MIX_SHAPES)


def mix_set_index(b):
    return b % len(MIX_SETS)


def mix_shapes():
    return [MIX_SHAPES[mix_shape_index(b)] for b in range(MIX_ROUNDS)]


def set_name(q):
    return q.get("algorithm", "PCA")


@functools.lru_cache(maxsize=None)
def mix_inputs():
    """(reports, reputation, scaled, lo, hi, aux_scores): lists over the rounds, with missing values,
    scaled bounds and raw reputations (synthetic.rounds, as tests/ragged_wide_cases.py)."""
    from pyconsensus_amd import synthetic

    per = []
    for k, (N, E) in enumerate(MIX_SHAPES):
        n = sum(1 for b in range(MIX_ROUNDS) if mix_shape_index(b) == k)
        R, sc, lo, hi, rep = synthetic.rounds(n, N, E, seed=2300 + k)
        aux = np.random.default_rng(2400 + k).normal(size=(n, N))
        per.append((R, rep, sc, lo, hi, aux))
    seen = [0] * len(MIX_SHAPES)
    out = [[] for _ in range(6)]
    for b in range(MIX_ROUNDS):
        k = mix_shape_index(b)
        for dst, src in zip(out, per[k]):
            dst.append(src[seen[k]])
        seen[k] += 1
    return tuple(out)


# ------------------------------------------------------------------ the study
STUDY_T = 3
STUDY_BASES = [cell(40, 1, 1, 31, liar_frac=0.4), cell(7, 5, 3, 32, liar_frac=0.4), cell(5, 64, 32, 33),
               cell(3, 65, 33, 34)]
STUDY_SETS = [
    {"alpha": 0.1},                                        # PCA
    {"alpha": 0.5},                                        # PCA
    {"algorithm": "absolute"},
    {"algorithm": "hierarchical"},
    {"algorithm": "clusterfeck", "cluster_threshold": 0.4},
]


def study_cells():
    """Every base cell under every set, base after base (so pair_with="first" pairs a cell with its
    base's alpha = 0.1 cell), then a copy of the 5 x 3 cell under set 0: paired with an equal cell."""
    cells, sets = [], []
    for base in STUDY_BASES:
        for q in STUDY_SETS:
            cells.append(dict(base, **q))
            sets.append(q)
    cells.append(dict(STUDY_BASES[1], **STUDY_SETS[0]))
    sets.append(STUDY_SETS[0])
    return cells, sets


def bare(c):
    """The cell without its parameter keys."""
    return {k: v for k, v in c.items() if k not in PARAM_KEYS}


def replay(c, T, scaled_tol=0.1, **params):
    """Cell c's trajectory on the host, as tests/test_sim_gpu.py replays one: generate_host, the C
    oracle with the carried reputation and these consensus parameters, numpy metrics."""
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd.simulate import generate_host

    rep, ms, ss = None, [], []
    for t in range(T):
        g = generate_host(c["rounds"], c["reporters"], c["events"], t=t, seed=c["seed"], **W.rates(c))
        o = OC.batched(g["reports"], g["scaled"], g["lo"], g["hi"], rep, threads=4,
                       want=("old_rep", "smooth_rep", "outcomes_final"), **params)
        m = W.np_metrics(g["scaled"], g["lo"], g["hi"], g["truth"], g["liar"], o["old_rep"], o["smooth_rep"],
                         o["outcomes_final"], scaled_tol)
        ms.append(m)
        ss.append(W.np_summary(m))
        rep = o["smooth_rep"]
    return {"metrics": np.stack(ms), "summary": np.stack(ss), "reputation": rep}
