"""Crafted batches for the batched kernel's interpolation-median prescreen (csrc/pcx_batched.hip,
wave_wmedian_screen; csrc/pcx_batched_round.inc, the block after stamp 13) and a numpy restatement of
it.  Builders only: the tests are test_interp_prescreen_cpu.py and test_interp_prescreen_gpu.py.

Every batch is B = 32 rounds of N x E.  Eight kinds are median_shortcut_cases.build's as they are
(plain, ties, exact_half, dominant, negative, zero_rows, all_missing_column, no_missing).  The crafted
kinds start from synthetic.rounds and rewrite column 0: scaled, bounds (0, 1) so that the rescale is
the identity, with max(1, N // 10) missing rows (N = 2 has room for one present row only, N = 3 for
two: there a kind keeps the parts that fit):

(collision and near_half also fill the other scaled columns' missing cells, so column 0's medians are the
batch's only interpolation medians and the kernel's prescreen counter must be zero)

* collision: two present values 0.5 and 0.5 (1 + 2^-30), equal in the top 32 bits of their keys, the
  rows below them and the first holding less than half the weight, with the second more: the median is
  the second, and the prescreen, which sees one group, must refuse;
* near_half: integer reputations: the rows below the crossing row sum to 2^20, the crossing row has 2,
  the rows above 2^20, the missing rows 0.  The crossing row's below-sum is 2^-21 T under half: inside
  the prescreen's margin of 2^-16 T (refused), yet the fp64 scan decides it;
* uniform: reputation = None; one missing row in the even rounds and two in the odd ones, so both an
  even and an odd count of present rows occur.  The kernel does not prescreen such a batch (an even
  count puts a running sum exactly on half), so its counter must be zero; the
  restatement without that rule still has to agree with the oracle wherever it decides;
* zero_weight: present rows of reputation 0 below the crossing, above it and at the crossing value;
* signed: column 0's bounds are (0, 2^600) and its present reports negative, 2^-440 u (subnormal after
  the rescale), 2^600 u and 2^800 u (2^200 u after it): the keys' order over signs and exponents;
* one_present: a single present row;
* equal: uniform's column 0 with a reputation of 1.0 given to every reporter: this batch is prescreened,
  and with an even count of present rows a running sum lies exactly on half.

restate(c, scaled, scale) restates the prescreen on the C oracle's own outputs (`original`, `old_rep`)
with row-order fp64 sums against a margin of `scale` x 2^-16 T.  The kernel's single-precision sums are
within 2^-17 T of those, so a median the restatement decides at scale 2 the kernel decides too, and one
the kernel decides the restatement decides at scale 0.5: the two counts bound the kernel's counter.

The seeds below were chosen on the CPU (the C oracle and restate(), no GPU) so that at 50 x 20 each
kind takes its path in at least 8 of its 32 rounds and plain is decided in at least 90 % of its medians
at scale 2 (the first seed tried held); test_interp_prescreen_cpu.py asserts it again.
"""
import functools

import numpy as np

import median_shortcut_cases as MC

B = MC.B
SHARED = ("plain", "ties", "exact_half", "dominant", "negative", "zero_rows", "all_missing_column", "no_missing")
CRAFTED = ("collision", "near_half", "uniform", "zero_weight", "signed", "one_present", "equal")
KINDS = SHARED + CRAFTED
SHAPES = [(50, 20), (50, 21), (2, 3), (3, 4), (9, 5), (64, 32)]
SEED = 7300  # (+ 64 N + E + 1000 * index of the kind)


def _ints(rng, n, total):
    """n positive integers summing to total."""
    return 1 + rng.multinomial(total - n, np.full(n, 1.0 / n)) if n else np.zeros(0, dtype=np.int64)


def build(kind, N, E):
    """(reports, keyword arguments of OC.batched / consensus_batched) of one batch."""
    if kind in SHARED:
        return MC.build(kind, N, E)
    from pyconsensus_amd import synthetic

    k = CRAFTED.index(kind)
    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=SEED + 64 * N + E + 1000 * k)
    sc, lo, hi, rep = sc.copy(), lo.copy(), hi.copy(), rep.copy()
    rng = np.random.default_rng(47 + 64 * N + E + 1000 * k)
    sc[:, 0], lo[:, 0], hi[:, 0] = True, 0.0, 1.0
    if kind in ("collision", "near_half"):  # column 0's are the batch's only interpolation medians
        for j in range(1, E):
            fresh = MC._scaled_values(rng, lo[:, j], hi[:, j], (B, N))
            R[:, :, j] = np.where(sc[:, j][:, None] & np.isnan(R[:, :, j]), fresh, R[:, :, j])
    for b in range(B):
        n_miss = min(N - 1, max(1, N // 10))
        if kind in ("uniform", "equal"):
            n_miss = min(N - 1, 1 + b % 2)
        if kind == "one_present":
            n_miss = N - 1
        order = rng.permutation(N)
        r_miss, pres = order[:n_miss], order[n_miss:]
        P = len(pres)
        x = rng.permutation(P) / (4.0 * P) + rng.uniform(0.3, 0.5)  # distinct, in (0.3, 0.75)
        w = rng.integers(1, 10, P).astype(np.float64)
        if kind == "collision":
            n_lo = max(0, (P - 2) // 2)
            n_hi = max(0, P - 2 - n_lo)
            x[:n_lo] = rng.uniform(0.1, 0.3, n_lo)
            x[n_lo] = 0.5
            if P > 1:
                x[n_lo + 1] = 0.5 * (1.0 + 2.0 ** -30)
                x[n_lo + 2:] = rng.uniform(0.7, 0.9, n_hi)
                w[n_lo + 1] = abs(w[:n_lo + 1].sum() - w[n_lo + 2:].sum()) + 4.0
        elif kind == "near_half":
            n_lo = max(1, (P - 1) // 2) if P > 1 else 0
            n_hi = max(0, P - 1 - n_lo)
            x[:n_lo] = rng.uniform(0.1, 0.3, n_lo)
            x[n_lo] = 0.5
            x[n_lo + 1:] = rng.uniform(0.7, 0.9, n_hi)
            w[:n_lo] = _ints(rng, n_lo, 2 ** 20)
            w[n_lo] = 2.0
            w[n_lo + 1:] = _ints(rng, n_hi, 2 ** 20)
        elif kind == "zero_weight":
            n_lo = max(0, (P - 2) // 2)
            n_hi = max(0, P - 2 - n_lo)
            x[:n_lo] = rng.uniform(0.1, 0.3, n_lo)
            x[n_lo] = 0.5
            if P > 1:
                x[n_lo + 1] = 0.5  # the crossing value's second row: reputation 0
                x[n_lo + 2:] = rng.uniform(0.7, 0.9, n_hi)
                w[n_lo + 1] = 0.0
            if n_lo > 1:
                w[0] = 0.0
            if n_hi > 1:
                w[P - 1] = 0.0
            w[n_lo] = abs(w[:n_lo].sum() - w[n_lo + 2:].sum()) + 4.0
        elif kind == "signed":
            hi[b, 0] = 2.0 ** 600
            u = rng.uniform(0.5, 1.0, P)
            cls = rng.integers(0, 4, P)
            x = np.where(cls == 0, -u * 2.0 ** 599, np.where(cls == 1, u * 2.0 ** -440,
                                                            np.where(cls == 2, u * 2.0 ** 600, u * 2.0 ** 800)))
        R[b, pres, 0] = x
        R[b, r_miss, 0] = np.nan
        rep[b, pres] = w
        if kind == "equal":
            rep[b, :] = 1.0
        if kind == "near_half":
            rep[b, r_miss] = 0.0
    kw = dict(reputation=None if kind == "uniform" else rep, scaled=sc, lo=lo, hi=hi)
    return R, kw


@functools.lru_cache(maxsize=None)
def batch(kind, N, E):
    """(reports, keyword arguments, the C oracle's outputs) of a batch, computed once."""
    if kind in SHARED:
        return MC.batch(kind, N, E)
    from oracle import pcx_oracle_c as OC

    R, kw = build(kind, N, E)
    return R, kw, OC.batched(R, **kw, threads=4)


def key_hi32(x):
    """Top 32 bits of the order-preserving key of each double (-0.0 folded onto +0.0)."""
    u = np.where(x == 0.0, 0.0, x).astype(np.float64).view(np.uint64)
    u = np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))
    return (u >> np.uint64(32)).astype(np.uint32)


def screen_decides(x, rep, scale):
    """The prescreen of one rescaled column x (NaN or 0.0 = missing) under the round's normalised
    reputations, at `scale` times its margin: (decided, median)."""
    present = ~(np.isnan(x) | (x == 0.0))
    if not np.all(rep >= 0.0) or not present.any():  # (a NaN reputation fails the first)
        return False, None
    T = MC._seq_sum(rep[present])
    if not 2.0 ** -100 <= T <= 2.0 ** 100:
        return False, None
    half, M = 0.5 * T, scale * 2.0 ** -16 * T
    if np.any(rep[present] >= half - M):
        return False, None
    key = np.where(present, key_hi32(np.where(present, x, 1.0)), np.uint32(0xffffffff))
    bl = np.array([MC._seq_sum(rep[present & (key < key[i])]) for i in range(len(x))])
    if np.any(np.abs(bl[present] - half) <= M):
        return False, None
    vk = key[present & (bl < half - M)].max()  # (the lowest key always qualifies)
    group = x[present & (key == vk)]
    v = group[0]
    if np.any(group != v) or not (v != 0.0 and abs(v) < 2.0 ** 1023):
        return False, None
    return True, v


def restate(c, scaled, scale, bypass=False):
    """Per (round, scaled column with a missing report) of the oracle's outputs c: has [B][E] bool (the
    column has an interpolation median), decided [B][E] bool, median [B][E].  bypass: the kernel's rule
    for a batch without reputations (reputation=None), which does not prescreen: nothing is decided."""
    orig, rep = c["original"], c["old_rep"]
    nb, _, E = orig.shape
    has, decided, med = np.zeros((nb, E), dtype=bool), np.zeros((nb, E), dtype=bool), np.full((nb, E), np.nan)
    for b in range(nb):
        for j in np.flatnonzero(scaled[b]):
            x = orig[b, :, j]
            if not np.any(np.isnan(x) | (x == 0.0)):
                continue
            has[b, j] = True
            d, v = screen_decides(x, rep[b], scale)
            if d and not bypass:
                decided[b, j], med[b, j] = True, v
    return has, decided, med


def counter_bounds(kind, N=50, E=20):
    """(lower, upper, total) of the kernel's prescreen counter over the batch: the medians the
    restatement decides at twice the margin, those it decides at half of it, all of them."""
    _, kw, c = batch(kind, N, E)
    sc = np.asarray(kw["scaled"]).astype(bool)
    bypass = kw["reputation"] is None
    has, d2, _ = restate(c, sc, 2.0, bypass)
    _, dh, _ = restate(c, sc, 0.5, bypass)
    return int(np.count_nonzero(d2)), int(np.count_nonzero(dh)), int(np.count_nonzero(has))
