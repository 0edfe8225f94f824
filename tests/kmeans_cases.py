"""Cases and helpers of k-means in ragged batches and in the simulator, shared
by test_kmeans_ragged_cpu.py, test_kmeans_ragged_gpu.py and test_kmeans_sim_gpu.py.  Needs no GPU.
No test here."""
import functools

import numpy as np

import sim_sweep_cases as W

same_bits = W.same_bits
cell = W.cell

# Shapes at the code-book boundaries N = k^2 and k^2 + 1 (the rule's k steps there), and the
# degenerate edges: one reporter, one event, the kernels' limits.
WAVE_SHAPES = [(1, 1), (2, 1), (4, 3), (5, 3), (9, 2), (10, 4), (16, 5), (17, 5), (25, 1), (26, 6), (36, 8), (37, 8),
               (49, 20), (50, 20), (64, 1), (64, 32), (3, 32)]
WG_SHAPES = [(65, 2), (81, 3), (82, 7), (100, 50), (144, 9), (145, 9), (225, 4), (226, 16), (256, 1), (256, 64)]
WAVE_PER, WG_PER = 3, 2
RESTARTS = (1, 3, 20)


def rule(N):
    return int(np.ceil(np.sqrt(N)))


@functools.lru_cache(maxsize=None)
def shape_rounds(N, E, n, seed):
    """n rounds of N x E of the simulator's kind (missing reports, scaled events) and a raw reputation:
    (reports (n,N,E), reputation (n,N), scaled, lo, hi (n,E))."""
    from pyconsensus_amd.simulate import generate_host

    g = generate_host(n, N, E, t=0, seed=seed, na_frac=0.15, scaled_frac=0.3)
    rep = np.random.default_rng(seed).uniform(0.5, 2.0, size=(n, N))
    return g["reports"], rep, g["scaled"], g["lo"], g["hi"]


@functools.lru_cache(maxsize=None)
def batch(kind):
    """The test rounds of ``kind`` ("wave", "wg" or "wide" = both) in a fixed shuffled order: a list of
    (shape, index inside the shape's rounds)."""
    shapes = {"wave": [(s, WAVE_PER) for s in WAVE_SHAPES], "wg": [(s, WG_PER) for s in WG_SHAPES]}
    shapes["wide"] = shapes["wave"] + shapes["wg"]
    rounds = [(s, i) for s, per in shapes[kind] for i in range(per)]
    order = np.random.default_rng(len(rounds)).permutation(len(rounds))
    return [rounds[i] for i in order]


def per_shape(shape):
    return WAVE_PER if shape in WAVE_SHAPES else WG_PER


def shape_seed(shape):
    return 7000 + 300 * shape[0] + shape[1]


def round_inputs(kind):
    """The ragged call's five lists over batch(kind)."""
    out = [[] for _ in range(5)]
    for shape, i in batch(kind):
        src = shape_rounds(shape[0], shape[1], per_shape(shape), shape_seed(shape))
        for dst, a in zip(out, src):
            dst.append(a[i])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def books(kind, restarts, seed=0, k=None):
    """One book (restarts, k_b) per round of batch(kind), replaying the reference's draws on a
    RandomState of its own.  k: None (the rule), or a tuple of code-book sizes."""
    from pyconsensus_amd.batched import kmeans_draws_ragged

    ns = [s[0] for s, _ in batch(kind)]
    return kmeans_draws_ragged(ns, restarts, np.random.RandomState(1000 * restarts + seed), k=k)


def shape_batches(kind, the_books):
    """{shape: (round indices in batch(kind), in the order of the shape's own rounds; their books
    stacked (n, restarts, k))} -- what one equal-shape call per shape takes.  Only for books of one k
    per shape."""
    by = {}
    for b, (shape, i) in enumerate(batch(kind)):
        by.setdefault(shape, {})[i] = b
    return {shape: ([idx[i] for i in sorted(idx)], np.stack([the_books[idx[i]] for i in sorted(idx)]))
            for shape, idx in by.items()}


def spec_shape(shape, book3, **params):
    """The C SPEC on every round of ``shape`` with its books (n, restarts, k)."""
    from oracle import pcx_oracle_c as OC

    R, rep, sc, lo, hi = shape_rounds(shape[0], shape[1], per_shape(shape), shape_seed(shape))
    return OC.batched(R, sc, lo, hi, rep, algorithm="k-means", kmeans_init=book3, threads=4, **params)


OUTPUTS_N = ("old_rep", "this_rep", "smooth_rep", "scores", "na_row", "participation_rows", "relative_part",
             "reporter_bonus")
OUTPUTS_E = ("adj_first_loadings", "outcomes_raw", "outcomes_adjusted", "outcomes_final", "certainty",
             "consensus_reward", "nas_filled", "participation_columns", "author_bonus")
OUTPUTS_1 = ("participation", "avg_certainty", "branch", "flags", "pi_iters", "components")
