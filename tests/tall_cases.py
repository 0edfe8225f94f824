"""Inputs and SPEC runs of the tall batched rounds (256 < N <= 1024 reporters on the workgroup-per-round
kernel, csrc/pcx_tall.hip), shared by test_tall_cpu.py (the SPEC built for 1024 reporters against the
256 build, the route and the LDS plan, the generators' coverage) and test_tall_gpu.py (the kernel
against that SPEC, bit for bit).  Needs no GPU.

The SPEC is oracle/pcx_oracle_batched.c built with oracle/Makefile's CFLAGS plus -DNMAX=1024 into
tests/_spec/libpcx_oracle1024.so, on first use.  Its cost counts in a test's time: a weighted median
over 1024 reporters per scaled column and round is what makes it slow, so the crafted batches whose
columns are (nearly) all scaled run one round of each of their eight patterns, not six.
"""
import ctypes as C
import functools
import os
import re
import shlex
import subprocess

import numpy as np

from oracle import pcx_oracle_c as OC
from pyconsensus_amd import _abi, synthetic
from pyconsensus_amd._abi import BATCH_OUTPUTS, Batch, BatchResult, out_shape
from pyconsensus_amd.batched import clusterfeck_threshold
from medium_edges import MEDIAN_GROUPS, _algorithm_kw, median_rounds
from test_batched_masks_gpu import B as MASK_B, CONFIGS, GROUP as MASK_GROUP, crafted_rounds
from test_batched_pi_gpu import side_rounds

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = os.path.join(os.path.dirname(HERE), "oracle")
SPEC_LIB = os.path.join(HERE, "_spec", "libpcx_oracle1024.so")
ZERO_COV, SVD_FAIL, PI_MAXIT = _abi.FLAG_ZERO_COV, _abi.FLAG_SVD_FAIL, _abi.FLAG_PI_MAXIT
WAVE, WORKGROUP, SCHEDULER, TALL = 0, 1, 2, 3
LDS_LIMIT = 160 * 1024
PLAIN = ("PCA", "absolute", "big-five", "fixed-variance", "cokurtosis")
MUST = ("flags", "pi_iters", "branch", "components", "smooth_rep", "outcomes_final")

_spec = None


def spec_lib():
    """The SPEC built with NMAX = 1024 (built on first use; an error, never a skip, if it cannot be)."""
    global _spec
    if _spec is None:
        src = os.path.join(ORACLE, "pcx_oracle_batched.c")
        if not os.path.exists(SPEC_LIB) or os.path.getmtime(SPEC_LIB) < os.path.getmtime(src):
            with open(os.path.join(ORACLE, "Makefile")) as f:
                m = re.search(r"^CFLAGS\s*=\s*(.*)$", f.read(), re.M)
            assert m, "oracle/Makefile has no CFLAGS line"
            os.makedirs(os.path.dirname(SPEC_LIB), exist_ok=True)
            tmp = "%s.%d.tmp" % (SPEC_LIB, os.getpid())
            subprocess.check_call([os.environ.get("CC", "gcc")] + shlex.split(m.group(1)) +
                                  ["-DNMAX=1024", "-shared", "-o", tmp, src, "-lm"])
            os.replace(tmp, SPEC_LIB)
        h = C.CDLL(SPEC_LIB)
        h.pcxo_consensus_batched_f64.argtypes = [C.POINTER(Batch), C.POINTER(BatchResult), C.c_int]
        h.pcxo_consensus_batched_f64.restype = C.c_int
        _spec = h
    return _spec


def spec(reports, scaled=None, lo=None, hi=None, reputation=None, catch_tolerance=0.1, alpha=0.1, int_dtype=False,
         algorithm="PCA", threads=8, want=None, max_components=5, variance_threshold=0.9, aux_scores=None,
         hierarchy_threshold=0.5, cluster_threshold=None):
    """OC.batched on the 1024-reporter build: {name: array} of every output in ``want`` (default all)."""
    R = np.ascontiguousarray(reports, dtype=np.float64)
    B, N, E = R.shape
    shared = scaled is not None and np.ndim(scaled) == 1
    cont = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
    ptr = lambda a: None if a is None else a.ctypes.data
    sc, lo_, hi_ = cont(scaled, np.uint8), cont(lo, np.float64), cont(hi, np.float64)
    rp, ax = cont(reputation, np.float64), cont(aux_scores, np.float64)
    cthr = clusterfeck_threshold(E) if cluster_threshold is None else float(cluster_threshold)
    inp = Batch(B, N, E, ptr(R), ptr(rp), ptr(sc), ptr(lo_), ptr(hi_), int(shared), int(bool(int_dtype)),
                float(catch_tolerance), float(alpha), _abi.ALGORITHMS[algorithm], int(min(max_components, E)),
                float(variance_threshold), ptr(ax), float(hierarchy_threshold), cthr, 0, 0, None)
    outs, res = {}, BatchResult()
    for name, kind, dt in BATCH_OUTPUTS:
        if want is None or name in want:
            outs[name] = np.empty(out_shape(kind, B, N, E), dtype=dt)
            setattr(res, name, outs[name].ctypes.data)
    rc = spec_lib().pcxo_consensus_batched_f64(C.byref(inp), C.byref(res), int(threads))
    if rc != 0:
        raise ValueError("the 1024-reporter SPEC rejected the batch (rc=%d)" % rc)
    return outs


def take(R, kw, idx):
    """Rounds ``idx`` of a batch: the inputs and every per-round keyword array alike."""
    nb = len(R)
    return R[idx], {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == nb else v)
                    for k, v in kw.items()}


def bits_equal(a, b):
    """Bit for bit, NaNs matching NaNs."""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)


def plan(N, E, alg="PCA"):
    """pcx_tall_plan as a tuple (median waves, rows per np.dot chunk, np.dot chunks, threads), or None."""
    from pyconsensus_amd import _lib

    out = (C.c_int32 * 4)()
    return tuple(out) if _lib.lib().pcx_tall_plan(N, E, _abi.ALGORITHMS[alg], out) == 0 else None


def lds_from_plan(N, E, alg, p):
    """The launch's dynamic LDS restated from the plan (include/pcx.h, pcx_tall_plan)."""
    waves, rows = p[0], p[1]
    E4 = 0 if E == 1 else E & ~3
    pn = 2
    while pn < N:
        pn <<= 1
    mt = (2 if alg in ("big-five", "fixed-variance") else 1) * E * (E + 1)
    region = max(mt, waves * (2 * N + 2 * pn + pn // 2), rows // 4 * E4 + (E - E4) * N)
    return (region + 11 * N + 22 * E) * 8 + ((N * E + 15) >> 4) * 4 + 16


def bigfive_capacity():
    """The largest N that the plan allows for big-five at E = 64 (from pcx_tall_route)."""
    from pyconsensus_amd.batched import route

    return max(N for N in range(257, 1025) if route(N, 64, "big-five", tall=True) == "tall")


# ---------------------------------------------------------------- the GPU test's cases
# 257 x 5: one row past the old limit (a sort network of 512 slots, nq = 5 in the NaN rank path, four
# median waves); 513 x 33: a network of 1024 slots, E odd, two median waves; 1024 x 64: capacity -- one
# median wave, the np.dot partials in four row chunks with a shorter last one, mpw's deepest trees;
# 1024 x 1: the E == 1 ddot and pairwise sums over 1024 terms; 640 x 62: np.dot's tail columns past
# E & ~3 beside chunked partials (two chunks, the last shorter); 1023 x 7: the pairwise sum's deepest
# tree (1023 splits four times) and a row tail of three in np.dot
SYNTH_B = 6
SYNTH_SHAPES = [(257, 5), (513, 33), (1024, 64), (1024, 1), (640, 62), (1023, 7)]
BATTERY_SHAPES = [(257, 5), (513, 33), (1024, 64)]
ALG_CASES = [((513, 33), "absolute"), ((513, 33), "cokurtosis"), ((300, 64), "big-five"), ((300, 40), "fixed-variance"),
             ("capacity", "big-five")]
SLOW_MASKS = ("allscaled", "bounds")  # the SPEC's seconds per round at 1024 reporters (module docstring)


def sid(shape):
    return "%dx%d" % tuple(shape)


def gpu_shapes():
    """Every (N, E, algorithm) that test_tall_gpu.py runs on the tall kernel."""
    cap = (bigfive_capacity(), 64)
    out = [(N, E, "PCA") for N, E in SYNTH_SHAPES]
    out += [((cap if s == "capacity" else s) + (alg,)) for s, alg in ALG_CASES]
    return out + [(513, 33, "absolute"), (300, 20, "PCA")]


@functools.lru_cache(maxsize=None)
def synth_inputs(shape, alg="PCA"):
    N, E = bigfive_capacity() if shape == "capacity" else shape[0], 64 if shape == "capacity" else shape[1]
    R, sc, lo, hi, rep = synthetic.rounds(SYNTH_B, N, E, seed=700 + N + E)
    kw = dict(reputation=rep, scaled=sc, lo=lo, hi=hi)
    kw.update(_algorithm_kw(alg, SYNTH_B, N, E))
    return R, kw


def _frozen(c):
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def synth_spec(shape, alg="PCA"):
    R, kw = synth_inputs(shape, alg)
    return _frozen(spec(R, **kw))


@functools.lru_cache(maxsize=None)
def mask_inputs(shape, config):
    """A crafted mask batch (test_batched_masks_gpu.crafted_rounds); the slow configurations above 512
    reporters as one round of each of the eight patterns."""
    N, E = shape
    R, kw = crafted_rounds(N, E, config)
    if config in SLOW_MASKS and N > 512:
        R, kw = take(R, kw, np.arange(0, MASK_B, MASK_GROUP))
    return R, kw


@functools.lru_cache(maxsize=None)
def mask_spec(shape, config):
    R, kw = mask_inputs(shape, config)
    return _frozen(spec(R, **kw))


SIDE_NB, SIDE_TAKE = 96, 4


@functools.lru_cache(maxsize=None)
def side_inputs(shape):
    """The side battery (test_batched_pi_gpu.side_rounds, 96 rounds): the first four identical-reporter
    rounds, the first four overflowing-bounds rounds and every fourth degenerate-eigenvalue round (eight
    of them: both halves of their reputations), with the kinds' indices in the slice."""
    N, E = shape
    R, kw, kinds = side_rounds(N, E, seed=11, nb=SIDE_NB)
    idx = np.concatenate([kinds["ident"][:SIDE_TAKE], kinds["wide"][:SIDE_TAKE], kinds["degen"][::4]])
    R, kw = take(R, kw, idx)
    nd = len(kinds["degen"][::4])
    return R, kw, dict(ident=np.arange(SIDE_TAKE), wide=np.arange(SIDE_TAKE, 2 * SIDE_TAKE),
                       degen=np.arange(2 * SIDE_TAKE, 2 * SIDE_TAKE + nd))


@functools.lru_cache(maxsize=None)
def side_spec(shape):
    R, kw, _ = side_inputs(shape)
    return _frozen(spec(R, **kw))


def side_preconditions(shape, c, kinds):
    """The SPEC itself took the exits the rounds were made for."""
    f = c["flags"]
    assert np.all(f[kinds["ident"]] & ZERO_COV) and np.all(c["pi_iters"][kinds["ident"]] == 0)
    assert np.all(f[kinds["wide"]] & SVD_FAIL)
    assert np.all(f[kinds["degen"]] & (ZERO_COV | SVD_FAIL) == 0)
    assert np.all(c["pi_iters"][kinds["degen"]] > 0)
    if shape == (1024, 64):
        assert np.count_nonzero(f & PI_MAXIT) >= 1, "no round stops at the iteration cap"
    N = shape[0]
    assert np.all(c["this_rep"][kinds["ident"]] == 1.0 / N)
    assert np.isnan(c["this_rep"][kinds["wide"]]).all() and np.all(c["participation_columns"][kinds["wide"]] == 1.0)


def mask_preconditions(shape, config, R, kw, c):
    """The crafted entries are in the batch the SPEC ran: a fully NaN row (masked in the reference: its
    relative participation is |participation_rows|) and, with bounds, a scaled crafted column."""
    N, E = shape
    full = MASK_B if not (config in SLOW_MASKS and N > 512) else MASK_B // MASK_GROUP
    assert len(R) == len(c["flags"]) == full
    if config != "int":
        assert np.isnan(R[0]).all(axis=1).any()
    if kw.get("scaled") is not None and config != "noscaled":
        assert kw["scaled"][:, E - 1].any()


NAN_SHAPE = (513, 33)  # nq = 9 in the NaN rank path


@functools.lru_cache(maxsize=None)
def nan_inputs():
    """medium_edges.median_rounds under "absolute": the groups whose scaled column fills with NaN keep
    finite reputations there, so the outcome median ranks NaN values among numbers (the NaN rank
    path), here with nine elements per lane."""
    N, E = NAN_SHAPE
    R, kw, groups = median_rounds(N, E)
    kw.update(_algorithm_kw("absolute", len(R), N, E))
    return R, kw, groups


@functools.lru_cache(maxsize=None)
def nan_spec():
    R, kw, _ = nan_inputs()
    return _frozen(spec(R, **kw))


def nan_preconditions(R, c, groups):
    js = NAN_SHAPE[1] - 1
    n = 0
    for name in MEDIAN_GROUPS:
        for b in groups[name]:
            col = c["filled"][b, :, js]
            n += bool(np.isnan(col).any() and not np.isnan(col).all() and np.isfinite(c["smooth_rep"][b]).all())
    assert n >= 8, n  # a column of NaN and numbers beside finite weights: the rank path, not an early exit
