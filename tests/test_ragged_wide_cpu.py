"""Wide ragged batches without a GPU: the pure planning call (pcx_ragged_plan_wide) with its launch
classes, the Python argument errors under ``wide=True``, and the preconditions of the GPU suite's
inputs (test_ragged_wide_gpu.py), asserted on the C SPEC and the numpy restatement alone."""
import ctypes as C

import numpy as np
import pytest

import golden_cases as G
import parity as P
import ragged_wide_cases as W

ALGS = {"PCA": 0, "absolute": 1, "big-five": 2, "fixed-variance": 3, "cokurtosis": 4, "hierarchical": 6,
        "clusterfeck": 7}
# a hand-written mix: three wave rounds, and workgroup rounds on both sides of a class boundary
HAND = [(3, 4), (100, 50), (64, 32), (256, 64), (65, 1), (1, 33), (50, 20), (200, 34), (100, 50), (256, 64)]


def _plan(shapes, alg):
    from pyconsensus_amd import _lib

    n = np.ascontiguousarray([s[0] for s in shapes], dtype=np.int32)
    e = np.ascontiguousarray([s[1] for s in shapes], dtype=np.int32)
    totals, counts, lds, bad = (C.c_int64 * 3)(-7, -7, -7), (C.c_int64 * 4)(-7, -7, -7, -7), \
        (C.c_int64 * 4)(-7, -7, -7, -7), C.c_int64(-7)
    rc = _lib.lib().pcx_ragged_plan_wide(len(shapes), n.ctypes.data, e.ctypes.data, alg, totals, counts, lds,
                                         C.byref(bad))
    return rc, [int(x) for x in totals], [int(x) for x in counts], [int(x) for x in lds], int(bad.value)


@pytest.mark.parametrize("name", sorted(ALGS))
@pytest.mark.parametrize("shapes", [HAND, W.MIX_SHAPES], ids=["hand", "mix"])
def test_plan_totals_counts_and_lds(name, shapes):
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import ragged_plan

    h = _lib.lib()
    rc, totals, counts, lds, bad = _plan(shapes, ALGS[name])
    assert rc == 0 and bad == -1
    assert totals == [sum(n for n, _ in shapes), sum(e for _, e in shapes), sum(n * e for n, e in shapes)]
    wave = [s for s in shapes if W.is_wave(*s)]
    assert counts[0] == len(wave) and lds[0] == ragged_plan(wave, name)[1]
    for c in (1, 2, 3):  # membership by the formula, computed here from pcx_medium_lds_bytes
        members = [s for s in shapes if not W.is_wave(*s) and W.launch_class(*s, name) == c]
        assert counts[c] == len(members), (c, counts, members)
        assert lds[c] == max([h.pcx_medium_lds_bytes(n, e, ALGS[name]) for n, e in members], default=0)
    assert sum(counts) == len(shapes)
    assert ragged_plan(shapes, name, wide=True) == (tuple(totals), tuple(counts), tuple(lds))


def test_hand_mix_counts_by_hand():
    """PCA: 100 x 50 asks 39,268 bytes (+ 4,288 static -> 35 units of 1,280: three per CU), 256 x 64
    asks 74,768 (62 units: two per CU); 200 x 34 is in the class of two, 65 x 1 and 1 x 33 of three."""
    rc, _, counts, _, _ = _plan(HAND, 0)
    assert rc == 0 and counts == [3, 0, 3, 4]
    assert W.launch_class(100, 50, "PCA") == 3 and W.launch_class(256, 64, "PCA") == 2
    for name in ALGS:
        assert W.launch_class(100, 50, name) != W.launch_class(256, 64, name), name
    assert W.launch_class(256, 64, "big-five") == 1  # (the eigenvectors double the work region)


@pytest.mark.parametrize("shape", [(257, 4), (4, 65), (0, 4), (4, 0)])
def test_plan_names_the_first_bad_round(shape):
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import ragged_plan

    rc, _, _, _, bad = _plan([(3, 3), (256, 64), shape, (300, 70)], 0)
    assert rc == -1 and bad == 2
    msg = _lib.lib().pcx_last_error()
    assert b"round 2 is %d x %d" % shape in msg and b"[1, 256] x [1, 64]" in msg
    with pytest.raises(_lib.PcxError, match="round 1 is %d x %d" % shape):
        ragged_plan([(3, 4), shape], wide=True)


def test_plan_refuses_kmeans_unknown_algorithms_and_null_shapes():
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import ragged_plan

    h = _lib.lib()
    for alg in (5, 8, -1):
        rc, _, _, _, bad = _plan([(3, 3)], alg)
        assert rc == -1 and bad == -1
    _plan([(100, 50)], 5)
    assert b"k-means" in h.pcx_last_error()
    with pytest.raises(_lib.PcxError, match="k-means"):
        ragged_plan([(100, 50)], "k-means", wide=True)
    n = np.array([3], dtype=np.int32)
    for a, b in ((None, n.ctypes.data), (n.ctypes.data, None), (None, None)):
        assert h.pcx_ragged_plan_wide(1, a, b, 0, None, None, None, None) == -1
        assert b"NULL" in h.pcx_last_error()
    assert h.pcx_ragged_plan_wide(-1, n.ctypes.data, n.ctypes.data, 0, None, None, None, None) == -1


def test_plan_accepts_an_empty_batch_and_null_outputs():
    from pyconsensus_amd import _lib

    h = _lib.lib()
    totals, counts, lds, bad = (C.c_int64 * 3)(1, 1, 1), (C.c_int64 * 4)(1, 1, 1, 1), (C.c_int64 * 4)(1, 1, 1, 1), \
        C.c_int64(1)
    assert h.pcx_ragged_plan_wide(0, None, None, 0, totals, counts, lds, C.byref(bad)) == 0
    assert list(totals) == [0, 0, 0] and list(counts) == [0] * 4 and list(lds) == [0] * 4 and bad.value == -1
    n, e = np.array([100], dtype=np.int32), np.array([50], dtype=np.int32)
    none4 = (None, None, None, None)  # every output is optional
    assert h.pcx_ragged_plan_wide(1, n.ctypes.data, e.ctypes.data, 0, *none4) == 0
    assert h.pcx_ragged_plan_wide(1, n.ctypes.data, n.ctypes.data, 0, *none4) == -1  # 100 x 100


def test_exports():
    from pyconsensus_amd import _abi, _lib

    h = _lib.lib()
    assert h.pcx_abi_version() == 9 == _abi.ABI_VERSION
    for name in ("pcx_ragged_plan_wide", "pcx_consensus_ragged_wide_f64", "pcx_test_scratch_cap"):
        assert hasattr(h, name), name


@pytest.fixture
def no_library(monkeypatch):
    """Any libpcx call fails the test: the argument errors come first."""
    from pyconsensus_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "bind_stream", boom)


def test_wide_argument_errors_come_before_any_library_call(no_library):
    """The messages of test_ragged_cpu.py, with rounds above one wave."""
    from pyconsensus_amd.batched import consensus_ragged

    a, b = np.ones((100, 2)), np.ones((4, 50))
    with pytest.raises(ValueError, match=r"reports\[1\]"):
        consensus_ragged([a, np.ones((2, 3, 4))], wide=True)
    with pytest.raises(ValueError, match=r"reports\[0\]"):
        consensus_ragged([np.ones(100)], wide=True)
    with pytest.raises(ValueError, match="one vector per round"):
        consensus_ragged([a, b], reputation=[np.ones(100)], wide=True)
    with pytest.raises(ValueError, match=r"reputation\[1\]"):
        consensus_ragged([a, b], reputation=[np.ones(100), np.ones(5)], wide=True)
    with pytest.raises(ValueError, match=r"lo\[0\]"):
        consensus_ragged([a, b], scaled=[np.zeros(2), np.zeros(50)], lo=[np.zeros(3), np.zeros(50)],
                         hi=[np.ones(2), np.ones(50)], wide=True)
    with pytest.raises(ValueError, match="together"):
        consensus_ragged([a, b], scaled=[np.zeros(2), np.zeros(50)], wide=True)
    with pytest.raises(ValueError, match="aux_scores"):
        consensus_ragged([a, b], algorithm="cokurtosis", wide=True)
    with pytest.raises(ValueError, match=r"aux_scores\[1\]"):
        consensus_ragged([a, b], algorithm="cokurtosis", aux_scores=[np.ones(100), np.ones(5)], wide=True)
    with pytest.raises(NotImplementedError):
        consensus_ragged([a, b], algorithm="no-such", wide=True)


# ---------------------------------------------------------------- preconditions of the GPU inputs
def test_mix_holds_every_shape_and_every_launch_class():
    from pyconsensus_amd.batched import ragged_plan

    per, order = W.mix()
    assert len(order) == W.MIX_ROUNDS and {k for k, _ in order} == set(range(len(W.MIX_SHAPES)))
    shapes = [W.MIX_SHAPES[k] for k, _ in order]
    _, counts, _ = ragged_plan(shapes, "PCA", wide=True)
    assert counts[0] >= 3 and counts[2] >= 3 and counts[3] >= 3, counts
    _, counts, _ = ragged_plan(shapes, "big-five", wide=True)
    assert min(counts) >= 3, counts  # big-five: all three workgroup classes in one call
    assert sum(1 for n, e in W.MIX_SHAPES if e < 5) >= 4  # max_components = 5 is capped per round


@pytest.mark.parametrize("alg", W.SIDE_ALGS)
def test_side_and_median_rounds_take_their_branches_on_the_spec(alg):
    per, order = W.side_inputs()
    assert len(order) == len(W.SIDE_SHAPES) * (3 * W.SIDE_TAKE + len(W.M.MEDIAN_GROUPS) * W.M.MEDIAN_GROUP)
    W.side_preconditions(alg)


def test_consensus_many_problems_spec_agrees_with_the_restatement():
    """Every problem of the GPU suite's consensus_many test: the C SPEC (what the ragged path
    computes, bit for bit) and the numpy restatement of the reference agree under tests/parity.py,
    so the GPU test compares with Oracle with no exemption."""
    from oracle import pcx_oracle_c as OC
    from oracle.pcx_oracle import OracleCPU
    from pyconsensus_amd import Oracle

    ps, qs = W.many_problems(), W.many_problems()
    shapes = [np.asarray(p["reports"]).shape for p in ps]
    assert shapes[0] == (6, 4) and shapes[-3:] == [(70, 5), (100, 50), (256, 64)] and len(ps) == 10
    for i, (p, q) in enumerate(zip(ps, qs)):
        ref = G.flat_result(OracleCPU(**p).consensus())
        o = Oracle(**q)  # (the argument handling only: no GPU is touched before consensus())
        kw = {}
        if o.event_bounds is not None:
            sc, lo, hi = o._bounds_arrays()
            kw.update(scaled=sc[None], lo=lo[None], hi=hi[None])
        if o._rep_raw is not None:
            kw["reputation"] = np.asarray(o._rep_raw, dtype=np.float64)[None]
        c = OC.batched(np.asarray(o._data, dtype=np.float64)[None], int_dtype=o._int_dtype,
                       catch_tolerance=o.catch_tolerance, alpha=o.alpha, **kw)
        bad, _ = P.compare(ref, {k: v[0] for k, v in c.items()})
        assert not bad, (i, shapes[i], bad)
