"""Shared inputs and helpers of the simulator study tests (test_sim_study_cpu.py, test_sim_study_gpu.py):
hand-made flat rounds that reach every branch of the detail metrics, value arrays for the per-cell
statistics, and the numpy restatements of DESIGN.md 5.4.2 (written from its tables, not from the
library's code).  No test here."""
import numpy as np

import sim_sweep_cases as W

cell = W.cell
same_bits = W.same_bits

NDETAIL, NVALUES = 12, 18
TOL = 0.25  # the hand-made rounds' scaled_tol: 0.25 * (4 - -4) = 2 exactly, so an outcome can sit on the bound

# ------------------------------------------------------------------ hand-made rounds for the detail metrics
HAND_CELLS = [cell(14, 1, 1, 0), cell(14, 2, 1, 0), cell(14, 5, 3, 0), cell(14, 65, 33, 0)]


def _hand_cell(rng, R, N, E):
    """R >= 12 rounds of N x E; the first twelve are forced into one special case each, the rest is random."""
    d = {"scaled": rng.integers(0, 2, (R, E)).astype(np.uint8)}
    d["liar"] = rng.integers(0, 4, (R, N)).astype(np.uint8)
    d["scaled"][0], d["scaled"][1] = 0, 1                    # no scaled event / no binary event
    d["liar"][2], d["liar"][3] = 0, 1                        # no liar / only liars, none of whom colludes
    d["scaled"][[7, 9, 10], 0] = 0
    d["scaled"][[8, 11], 0] = 1
    sc = d["scaled"] != 0
    d["lo"] = np.where(sc, rng.integers(-50, 0, (R, E)), 1).astype(np.float64)
    d["hi"] = np.where(sc, rng.integers(1, 50, (R, E)), 2).astype(np.float64)
    d["truth"] = np.where(sc, rng.integers(-50, 50, (R, E)) / 4.0, rng.integers(1, 3, (R, E))).astype(np.float64)
    pick = rng.integers(0, 6, (R, E))
    width = d["hi"] - d["lo"]
    d["outcomes"] = np.select(
        [pick == 0, pick == 1, pick == 2, pick == 3, pick == 4],
        [d["truth"], d["truth"] + 0.05 * width, d["truth"] + 0.5 * width,
         np.where(sc, d["truth"], 1.5), np.where(sc, d["truth"], 3.0 - d["truth"])], np.nan)
    d["old"] = rng.random((R, N)) * np.exp(rng.normal(0, 6, (R, N)))  # magnitudes apart: the order shows
    d["smooth"] = d["old"] * rng.choice([0.5, 1.0, 2.0], (R, N))
    d["smooth"][4] = d["old"][4] * 0.5                       # everyone punished
    d["smooth"][5] = d["old"][5] * 2.0                       # nobody punished
    d["smooth"][6, 0] = np.nan
    d["outcomes"][7, 0] = d["outcomes"][8, 0] = np.nan       # a NaN outcome on a binary and on a scaled event
    d["outcomes"][9, 0] = 1.5
    d["outcomes"][10, 0] = 3.0 - d["truth"][10, 0]
    d["lo"][11, 0], d["hi"][11, 0], d["truth"][11, 0], d["outcomes"][11, 0] = -4.0, 4.0, 1.0, 3.0  # on the bound
    return d


def hand_rounds(cells=HAND_CELLS, seed=20261020):
    """(flat, per_cell): flat arrays in the sweep's layout and the same per cell as (R, ...) arrays."""
    rng = np.random.default_rng(seed)
    per_cell = [_hand_cell(rng, c["rounds"], c["reporters"], c["events"]) for c in cells]
    flat = {k: np.concatenate([d[k].reshape(-1) for d in per_cell]) for k in per_cell[0]}
    return flat, per_cell


def rounds_of(flat):
    return {k: flat[k] for k in ("scaled", "lo", "hi", "truth", "liar")}


# ------------------------------------------------------------------ numpy restatement: detail metrics
def _ratio(a, b):
    return np.float64(a) / np.float64(b) if b != 0 else np.float64("nan")


def np_detail_round(scaled, lo, hi, truth, liar, old_rep, smooth_rep, out, tol):
    """The twelve detail metrics of one round, from the table of DESIGN.md 5.4.2."""
    E, N = len(truth), len(liar)
    binary = [j for j in range(E) if not scaled[j]]
    scal = [j for j in range(E) if scaled[j]]
    with np.errstate(invalid="ignore"):
        d = np.empty(NDETAIL)
        d[0] = _ratio(sum(out[j] == truth[j] for j in binary), len(binary))
        d[1] = _ratio(sum(np.abs(out[j] - truth[j]) <= np.float64(tol) * (hi[j] - lo[j]) for j in scal), len(scal))
        d[2] = _ratio(sum(out[j] == 1.5 for j in binary), len(binary))
        d[3] = _ratio(sum(out[j] == 3.0 - truth[j] for j in binary), len(binary))
        d[4] = _ratio(sum(np.isnan(out[j]) for j in range(E)), E)
        err, cnt = np.float64(0.0), 0
        for j in scal:  # sequentially, in increasing j
            if not np.isnan(out[j]):
                err = err + np.abs(out[j] - truth[j]) / (hi[j] - lo[j])
                cnt += 1
        d[5] = _ratio(err, cnt)
        punished = [bool(smooth_rep[i] < old_rep[i]) for i in range(N)]
    lies = [bool(liar[i] & 1) for i in range(N)]
    tp = sum(p and l for p, l in zip(punished, lies))
    fn = sum((not p) and l for p, l in zip(punished, lies))
    fp = sum(p and not l for p, l in zip(punished, lies))
    tn = sum((not p) and not l for p, l in zip(punished, lies))
    d[6:10] = tp, fn, fp, tn
    tp, fn, fp, tn = (np.float64(x) for x in (tp, fn, fp, tn))
    d[10] = _ratio(tp * tn - fp * fn, np.sqrt(((tp + fp) * (tp + fn)) * ((tn + fp) * (tn + fn))))
    acc = np.float64(0.0)
    for i in range(N):  # sequentially, in increasing i
        if (liar[i] & 3) == 3:
            acc = acc + smooth_rep[i]
    d[11] = acc
    return d


def np_detail_cell(d, tol):
    """[R][12] of one cell's (R, ...) arrays."""
    return np.stack([np_detail_round(d["scaled"][r], d["lo"][r], d["hi"][r], d["truth"][r], d["liar"][r],
                                     d["old"][r], d["smooth"][r], d["outcomes"][r], tol)
                     for r in range(len(d["truth"]))])


# ------------------------------------------------------------------ numpy restatement: statistics
def _tree(s, op):
    s = s.copy()
    stride = 128
    while stride >= 1:
        s[:stride] = op(s[:stride], s[stride:2 * stride])
        stride //= 2
    return s[0]


def _lanes(x, ok, start, op):
    """Lane tau of 256 folds the values tau, tau + 256, ... (where ok) into `start` with op."""
    s = np.full(256, start, dtype=np.float64)
    for b0 in range(0, len(x), 256):
        chunk, use = x[b0:b0 + 256], ok[b0:b0 + 256]
        k = len(chunk)
        s[:k] = np.where(use, op(s[:k], chunk), s[:k])
    return s


def _add(a, b):
    return a + b


def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(b > a, b, a)


def np_stats_column(v, w=None):
    """{n, mean, var, min, max} of the non-NaN values of v, or with w of v - w where neither is NaN, in the
    library's order: 256 strided lanes from 0.0, the tree with strides 128 .. 1, then a second pass over
    (x - mean)^2 in the same order."""
    ok = ~np.isnan(v) if w is None else ~np.isnan(v) & ~np.isnan(w)
    with np.errstate(invalid="ignore"):
        x = np.where(ok, v if w is None else v - w, 0.0)
    nan = np.float64("nan")
    n = _tree(_lanes(np.ones(len(x)), ok, 0.0, _add), _add)
    total = _tree(_lanes(x, ok, 0.0, _add), _add)
    mn = _tree(_lanes(x, ok, np.inf, _min), _min)
    mx = _tree(_lanes(x, ok, -np.inf, _max), _max)
    if n == 0:
        return np.array([0.0, nan, nan, nan, nan])
    mean = total / n
    d = x - mean
    squares = _tree(_lanes(d * d, ok, 0.0, _add), _add)
    return np.array([n, mean, squares / (n - 1.0) if n >= 2 else nan, mn, mx])


def np_stats(cells, metrics, detail, pair_base=None):
    """(stats (T,C,18,5), paired (T,C,18,3) or None)."""
    T = metrics.shape[0]
    values = np.concatenate([metrics, detail], axis=2)
    starts = np.concatenate([[0], np.cumsum([c["rounds"] for c in cells])])
    stats = np.empty((T, len(cells), NVALUES, 5))
    paired = None if pair_base is None else np.empty((T, len(cells), NVALUES, 3))
    for t in range(T):
        for c in range(len(cells)):
            mine = values[t, starts[c]:starts[c + 1]]
            for v in range(NVALUES):
                stats[t, c, v] = np_stats_column(mine[:, v])
                if paired is None:
                    continue
                if pair_base[c] < 0:
                    paired[t, c, v] = 0.0, np.nan, np.nan
                else:
                    b = pair_base[c]
                    paired[t, c, v] = np_stats_column(mine[:, v], values[t, starts[b]:starts[b + 1], v])[:3]
    return stats, paired


# cells of 1, 2, 255, 256, 257 and 600 rounds; cell 4 is the base of two cells, cells 0 to 5 have none
STATS_CELLS = [cell(R, 3, 2, 0) for R in (1, 2, 255, 256, 257, 600, 257, 257, 600, 2, 1)]
STATS_BASE = np.array([-1, -1, -1, -1, -1, -1, 4, 4, 5, 1, 0], dtype=np.int32)
STATS_T = 2


def stats_values(seed=7):
    """metrics (T,B,6) without NaNs and detail (T,B,12) with: a whole column of cell 2, one side of a
    pair only (cell 6 against its base 4, both ways), and a sprinkle."""
    rng = np.random.default_rng(seed)
    B = sum(c["rounds"] for c in STATS_CELLS)
    starts = np.concatenate([[0], np.cumsum([c["rounds"] for c in STATS_CELLS])])
    metrics = rng.normal(0, 1, (STATS_T, B, 6)) * np.exp(rng.normal(0, 6, (STATS_T, B, 6)))
    detail = rng.normal(0, 1, (STATS_T, B, NDETAIL)) * np.exp(rng.normal(0, 6, (STATS_T, B, NDETAIL)))
    detail[:, :, 6:10] = rng.integers(0, 9, (STATS_T, B, 4))  # counts: exact sums, ties in min / max
    detail[:, starts[2]:starts[3], 1] = np.nan
    detail[:, starts[6] + 5, 3] = np.nan
    detail[:, starts[4] + 9, 3] = np.nan
    detail[:, :, 0] = np.where(rng.random((STATS_T, B)) < 0.2, np.nan, detail[:, :, 0])
    return metrics, detail
