"""What pcx_consensus_batched_f64 and pcx_consensus_ragged_f64 refuse, and in which words.

Every case hands one of the two entries a refused input at a 4 x 3 round shape (65 x 3 and up where
the k-means bound of the larger routes matters) and asserts PCX_EINVAL and the exact message.  The
expected strings are those of the entries before their option checks were shared (libpcx at commit
e9159b0); the cases with two faults at once pin the order of the checks, which is what sharing them
could change.  Every case is refused before anything reaches the stream: no kernel is launched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
PCA, BIG_FIVE, FIXED_VARIANCE, COKURTOSIS, KMEANS, HIERARCHICAL = 0, 2, 3, 4, 5, 6
PTR = 4096  # a non-NULL address for a pointer that is only tested, never followed: each case is refused first

KMEANS_MSG = "k-means needs kmeans_init and 1 <= kmeans_k <= min(N, 8; 1024 above 64 x 32), restarts >= 1"
BIG_FIVE_MSG = "big-five needs 1 <= max_components <= n_events"
ALG_MSG = "algorithm must be an enum pcx_algorithm value (0..7)"
SCALED_MSG = "scaled given without lo/hi"
FINITE_MSG = "catch_tolerance/alpha must be finite"
COKURT_MSG = 'cokurtosis needs aux_scores (aux["cokurt"])'
KM = dict(algorithm=KMEANS, kmeans_k=2, kmeans_restarts=1, kmeans_init=PTR)  # a k-means call that passes

# (case, fields changed from a valid PCA call on 4 x 3 rounds, the message after "batched: ")
BATCHED = [
    ("n_rounds<0", dict(n_rounds=-1), "n_rounds must be in [0, 2^31)"),
    ("n_rounds=2^31", dict(n_rounds=1 << 31), "n_rounds must be in [0, 2^31)"),
    ("n_reporters=0", dict(n_reporters=0), "n_reporters must be in [1, 2^31)"),
    ("n_reporters=2^31", dict(n_reporters=1 << 31), "n_reporters must be in [1, 2^31)"),
    ("n_events=0", dict(n_events=0), "n_events must be in [1, 65536]"),
    ("n_events=65537", dict(n_events=65537), "n_events must be in [1, 65536]"),
    ("reports", dict(reports=None), "reports is NULL"),
    ("scaled,no-lo", dict(scaled=PTR, hi=PTR), SCALED_MSG),
    ("scaled,no-hi", dict(scaled=PTR, lo=PTR), SCALED_MSG),
    ("algorithm=-1", dict(algorithm=-1), ALG_MSG),
    ("algorithm=8", dict(algorithm=8), ALG_MSG),
    ("kmeans,no-init", dict(KM, kmeans_init=None), KMEANS_MSG),
    ("kmeans,k=0", dict(KM, kmeans_k=0), KMEANS_MSG),
    ("kmeans,k>N", dict(KM, kmeans_k=5), KMEANS_MSG),
    ("kmeans,k>8", dict(KM, n_reporters=9, kmeans_k=9), KMEANS_MSG),
    ("kmeans,restarts=0", dict(KM, kmeans_restarts=0), KMEANS_MSG),
    ("kmeans,large,k>N", dict(KM, n_reporters=65, kmeans_k=66), KMEANS_MSG),
    ("kmeans,large,k>1024", dict(KM, n_reporters=65, kmeans_k=1025), KMEANS_MSG),
    ("kmeans,large,k>1024,k<=N", dict(KM, n_reporters=1025, kmeans_k=1025), KMEANS_MSG),
    ("hierarchy=nan", dict(algorithm=HIERARCHICAL, hierarchy_threshold=NAN), "hierarchy_threshold is NaN"),
    ("big-five,0", dict(algorithm=BIG_FIVE, max_components=0), BIG_FIVE_MSG),
    ("big-five,>E", dict(algorithm=BIG_FIVE, max_components=4), BIG_FIVE_MSG),
    ("variance=inf", dict(algorithm=FIXED_VARIANCE, variance_threshold=INF), "variance_threshold must be finite"),
    ("variance=nan", dict(algorithm=FIXED_VARIANCE, variance_threshold=NAN), "variance_threshold must be finite"),
    ("cokurtosis,no-aux", dict(algorithm=COKURTOSIS), COKURT_MSG),
    ("catch=nan", dict(catch_tolerance=NAN), FINITE_MSG),
    ("alpha=inf", dict(alpha=INF), FINITE_MSG),
    # two faults at once: the earlier check of the entry speaks
    ("2:n_events,reports", dict(n_events=0, reports=None), "n_events must be in [1, 65536]"),
    ("2:reports,algorithm", dict(reports=None, algorithm=8), "reports is NULL"),
    ("2:scaled,kmeans", dict(KM, scaled=PTR, kmeans_k=0), SCALED_MSG),
    ("2:algorithm,catch", dict(algorithm=8, catch_tolerance=NAN), ALG_MSG),
    ("2:kmeans,alpha", dict(KM, kmeans_init=None, alpha=NAN), KMEANS_MSG),
    ("2:hierarchy,alpha", dict(algorithm=HIERARCHICAL, hierarchy_threshold=NAN, alpha=NAN), "hierarchy_threshold is NaN"),
    ("2:big-five,alpha", dict(algorithm=BIG_FIVE, max_components=0, alpha=NAN), BIG_FIVE_MSG),
    ("2:variance,catch", dict(algorithm=FIXED_VARIANCE, variance_threshold=INF, catch_tolerance=INF),
     "variance_threshold must be finite"),
    ("2:cokurtosis,alpha", dict(algorithm=COKURTOSIS, alpha=NAN), COKURT_MSG),
]

# (case, fields changed from a valid PCA call on two 4 x 3 rounds, per-round (N, E) or None for NULL shape
# arrays, the message after "ragged: ")
TWO = [(4, 3), (4, 3)]
RAGGED = [
    ("n_rounds<0", dict(n_rounds=-1), TWO, "n_rounds must be in [0, 2^31)"),
    ("algorithm=8", dict(algorithm=8), TWO, ALG_MSG),
    ("kmeans", dict(algorithm=KMEANS), TWO, "k-means is not supported (its code-book size depends on each round's N)"),
    ("shapes", dict(), None, "n_reporters / n_events is NULL"),
    ("round,65x3", dict(), [(4, 3), (65, 3)], "round 1 is 65 x 3; a round must be within [1, 64] x [1, 32]"),
    ("round,4x33", dict(), [(4, 33), (4, 3)], "round 0 is 4 x 33; a round must be within [1, 64] x [1, 32]"),
    ("round,0x3", dict(), [(0, 3), (4, 3)], "round 0 is 0 x 3; a round must be within [1, 64] x [1, 32]"),
    ("reports", dict(reports=None), TWO, "reports is NULL"),
    ("scaled,no-lo", dict(scaled=PTR, hi=PTR), TWO, SCALED_MSG),
    ("scaled,no-hi", dict(scaled=PTR, lo=PTR), TWO, SCALED_MSG),
    ("hierarchy=nan", dict(algorithm=HIERARCHICAL, hierarchy_threshold=NAN), TWO, "hierarchy_threshold is NaN"),
    ("big-five,0", dict(algorithm=BIG_FIVE, max_components=0), TWO, "big-five needs max_components >= 1"),
    ("variance=inf", dict(algorithm=FIXED_VARIANCE, variance_threshold=INF), TWO, "variance_threshold must be finite"),
    ("variance=nan", dict(algorithm=FIXED_VARIANCE, variance_threshold=NAN), TWO, "variance_threshold must be finite"),
    ("cokurtosis,no-aux", dict(algorithm=COKURTOSIS), TWO, COKURT_MSG),
    ("catch=inf", dict(catch_tolerance=INF), TWO, FINITE_MSG),
    ("alpha=nan", dict(alpha=NAN), TWO, FINITE_MSG),
    # two faults at once
    ("2:kmeans,round", dict(algorithm=KMEANS), [(65, 3)], "k-means is not supported (its code-book size depends on "
                                                         "each round's N)"),
    ("2:round,reports", dict(reports=None), [(4, 3), (65, 3)], "round 1 is 65 x 3; a round must be within [1, 64] x "
                                                              "[1, 32]"),
    ("2:reports,catch", dict(reports=None, catch_tolerance=NAN), TWO, "reports is NULL"),
    ("2:scaled,hierarchy", dict(scaled=PTR, algorithm=HIERARCHICAL, hierarchy_threshold=NAN), TWO, SCALED_MSG),
    ("2:hierarchy,alpha", dict(algorithm=HIERARCHICAL, hierarchy_threshold=NAN, alpha=NAN), TWO,
     "hierarchy_threshold is NaN"),
    ("2:big-five,alpha", dict(algorithm=BIG_FIVE, max_components=0, alpha=NAN), TWO, "big-five needs max_components >= 1"),
    ("2:variance,alpha", dict(algorithm=FIXED_VARIANCE, variance_threshold=NAN, alpha=NAN), TWO,
     "variance_threshold must be finite"),
    ("2:cokurtosis,catch", dict(algorithm=COKURTOSIS, catch_tolerance=NAN), TWO, COKURT_MSG),
]


def _context():
    import torch

    from pyconsensus_amd import _device, _lib

    dev = torch.device("cuda", torch.cuda.current_device())
    return _lib.bind_stream(dev.index, _device.current_stream_handle(dev))


def refused_batched(lib, ctx, fields):
    from pyconsensus_amd import _abi

    base = dict(n_rounds=2, n_reporters=4, n_events=3, reports=PTR, catch_tolerance=0.1, alpha=0.1, algorithm=PCA,
                max_components=3, variance_threshold=0.9, hierarchy_threshold=0.5)
    inp = _abi.Batch(**dict(base, **fields))
    rc = lib.pcx_consensus_batched_f64(ctx, C.byref(inp), C.byref(_abi.BatchResult()))
    return rc, lib.pcx_last_error().decode()


def refused_ragged(lib, ctx, fields, shapes):
    from pyconsensus_amd import _abi

    base = dict(n_rounds=2 if shapes is None else len(shapes), reports=PTR, catch_tolerance=0.1, alpha=0.1,
                algorithm=PCA, max_components=3, variance_threshold=0.9, hierarchy_threshold=0.5)
    if shapes is not None:
        n = np.array([s[0] for s in shapes], dtype=np.int32)
        e = np.array([s[1] for s in shapes], dtype=np.int32)
        base.update(n_reporters=n.ctypes.data, n_events=e.ctypes.data)
    inp = _abi.Ragged(**dict(base, **fields))
    rc = lib.pcx_consensus_ragged_f64(ctx, C.byref(inp), C.byref(_abi.BatchResult()))
    return rc, lib.pcx_last_error().decode()


@pytest.mark.parametrize("fields,want", [pytest.param(f, w, id=i) for i, f, w in BATCHED])
def test_batched_refuses(gpu_lib, fields, want):
    from pyconsensus_amd import _abi

    assert refused_batched(gpu_lib, _context(), fields) == (_abi.EINVAL, "batched: " + want)


@pytest.mark.parametrize("fields,shapes,want", [pytest.param(f, s, w, id=i) for i, f, s, w in RAGGED])
def test_ragged_refuses(gpu_lib, fields, shapes, want):
    from pyconsensus_amd import _abi

    assert refused_ragged(gpu_lib, _context(), fields, shapes) == (_abi.EINVAL, "ragged: " + want)
