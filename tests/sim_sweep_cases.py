"""Shared cases and helpers of the simulator sweep tests (test_sim_sweep_cpu.py, test_sim_sweep_gpu.py,
test_sim_sweep_cli.py): the sweeps, the slicing of flat arrays by cell, and the numpy restatement of
DESIGN.md 5.4's metrics and summary order.  No test here."""
import numpy as np

RATES = ("liar_frac", "collude_frac", "distort", "na_frac", "scaled_frac")
ROUNDS = ("reports", "scaled", "lo", "hi", "truth", "liar")
# which per-cell starts slice which flat array
OFFSET_OF = {"reports": "cells", "scaled": "events", "lo": "events", "hi": "events", "truth": "events",
             "liar": "reporters", "old_rep": "reporters", "smooth_rep": "reporters", "outcomes_final": "events"}


def cell(rounds, reporters, events, seed, liar_frac=0.3, collude_frac=0.5, distort=0.1, na_frac=0.1, scaled_frac=0.25):
    return dict(rounds=rounds, reporters=reporters, events=events, seed=seed, liar_frac=liar_frac,
                collude_frac=collude_frac, distort=distort, na_frac=na_frac, scaled_frac=scaled_frac)


# the host generator's sweep: a 1 x 1 cell, an odd small one, the one-wave limit, just past it, the largest
HOST_SWEEP = [cell(3, 1, 1, 20261019),
              cell(2, 7, 5, (0xC0FFEE << 32) | 0x1234567, liar_frac=0.5, na_frac=0.2),
              cell(4, 64, 32, 3, collude_frac=0.9, scaled_frac=0.5),
              cell(2, 65, 33, 4, distort=0.3),
              cell(1, 256, 64, 5, liar_frac=0.1, scaled_frac=0.75)]
# E that divides 256, E that does not, a round smaller than one wave, many 1 x 1 rounds, and more rounds
# than one pass of the generator's grid takes (4,096 workgroups of four rounds): the grid-stride step
SMALL_SWEEP = [cell(2, 3, 64, 11), cell(3, 5, 3, 12, na_frac=0.3), cell(2, 256, 1, 13), cell(300, 1, 1, 14),
               cell(16500, 1, 2, 15)]
# the contract's sweep: the wave route, a workgroup round, a 1 x 1 cell without NaNs, classes 3 and 1
CONTRACT_SWEEP = [cell(257, 50, 20, 42, liar_frac=0.2),
                  cell(9, 65, 33, 43, collude_frac=0.8),
                  cell(3, 1, 1, 44, na_frac=0.0),
                  cell(5, 100, 50, 45, distort=0.25, scaled_frac=0.5),
                  cell(2, 256, 64, 46, liar_frac=0.4, na_frac=0.05)]
ALGORITHM_CASES = {
    "hierarchical": {},
    "clusterfeck": {"cluster_threshold": 0.6},
    "big-five": {"max_components": 5},   # with the 6 x 3 cell below the cap applies
    "fixed-variance": {},
    "absolute": {},
}
CAP_CELL = cell(4, 6, 3, 47)


def rates(c):
    return {k: c[k] for k in RATES}


def cell_slice(flat, offsets, kind, c):
    return flat[int(offsets[kind][c]):int(offsets[kind][c + 1])]


def same_bits(a, b):
    """Equal bit for bit, NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a.view(np.uint64)[~nan] == b.view(np.uint64)[~nan]).all())


# ------------------------------------------------------------------ numpy restatement
def np_metrics(scaled, lo, hi, truth, liar, old_rep, smooth_rep, outcomes_final, scaled_tol):
    """[B][6] of B rounds of one shape: correct, liar_rep_before, liar_rep_after, liars_bonus, beats, n_liars."""
    B, E = truth.shape
    with np.errstate(invalid="ignore"):
        ok = np.where(scaled != 0, np.abs(outcomes_final - truth) <= scaled_tol * (hi - lo),
                      outcomes_final == truth)  # a NaN outcome compares false
    lies = (liar & 1) == 1
    before, after = np.zeros(B), np.zeros(B)
    for i in range(liar.shape[1]):  # sequentially, in increasing i
        before = np.where(lies[:, i], before + old_rep[:, i], before)
        after = np.where(lies[:, i], after + smooth_rep[:, i], after)
    with np.errstate(invalid="ignore"):
        beats = (after > before).astype(np.float64)
    return np.stack([ok.sum(axis=1).astype(np.float64) / float(E), before, after, after - before, beats,
                     lies.sum(axis=1).astype(np.float64)], axis=1)


def np_summary(m):
    """Mean over a cell's rounds in the library's order: thread tau of 256 adds rounds tau, tau + 256,
    ... from 0.0; a tree with strides 128 .. 1 (s[tau] += s[tau + stride]); then / R."""
    R = m.shape[0]
    s = np.zeros((256, m.shape[1]))
    for b0 in range(0, R, 256):
        chunk = m[b0:b0 + 256]
        s[:len(chunk)] = s[:len(chunk)] + chunk
    stride = 128
    while stride >= 1:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        stride //= 2
    return s[0] / float(R)
