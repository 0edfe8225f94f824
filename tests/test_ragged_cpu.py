"""Ragged batches without a GPU: the pure planning call (pcx_ragged_plan), the pcx_ragged ctypes
mirror against the C compiler's layout of include/pcx.h, and the argument errors consensus_ragged
raises before it touches the library."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every shape kind of the GPU suite but 50 x 20 (whose equal-shape launch has a compiled instance with
# a smaller carve; a ragged launch runs it on the generic instance, checked on its own below)
SHAPES = [(1, 1), (1, 6), (30, 1), (2, 2), (7, 13), (63, 31), (64, 1), (1, 32), (64, 32), (48, 20), (7, 13)]
ALGS = {"PCA": 0, "absolute": 1, "big-five": 2, "fixed-variance": 3, "cokurtosis": 4, "hierarchical": 6,
        "clusterfeck": 7}


def _plan(shapes, alg):
    from pyconsensus_amd import _lib

    n = np.ascontiguousarray([s[0] for s in shapes], dtype=np.int32)
    e = np.ascontiguousarray([s[1] for s in shapes], dtype=np.int32)
    totals, lds, bad = (C.c_int64 * 3)(-7, -7, -7), C.c_int64(-7), C.c_int64(-7)
    rc = _lib.lib().pcx_ragged_plan(len(shapes), n.ctypes.data, e.ctypes.data, alg, totals, C.byref(lds),
                                    C.byref(bad))
    return rc, [int(x) for x in totals], int(lds.value), int(bad.value)


@pytest.mark.parametrize("name", sorted(ALGS))
def test_plan_totals_and_lds(name):
    from pyconsensus_amd import _lib

    h = _lib.lib()
    rc, totals, lds, bad = _plan(SHAPES, ALGS[name])
    assert rc == 0 and bad == -1
    assert totals == [sum(n for n, _ in SHAPES), sum(e for _, e in SHAPES), sum(n * e for n, e in SHAPES)]
    most = max(h.pcx_batched_lds_bytes(n, e, ALGS[name]) for n, e in SHAPES)
    if ALGS[name] < 5:
        assert lds == most  # the launch allocates the largest round's carve
    else:  # the clusterings' own region comes on top (pcx_batched_lds_bytes leaves it out)
        assert most < lds <= 64 * 1024
    assert lds % 8 == 0


def test_plan_50x20_takes_the_generic_carve():
    """An equal-shape 50 x 20 launch runs a compiled instance (even pitch, 50 median rows); in a
    ragged launch the round runs the generic instance: odd pitch, 64 median rows -- a larger carve,
    the one every other 50-reporter shape of the neighbourhood is allotted."""
    from pyconsensus_amd import _lib

    h = _lib.lib()
    _, _, lds, _ = _plan([(50, 20)], 0)
    assert lds > h.pcx_batched_lds_bytes(50, 20, 0)
    assert h.pcx_batched_lds_bytes(50, 19, 0) <= lds <= h.pcx_batched_lds_bytes(50, 21, 0)
    assert _plan([(50, 20)], 2)[2] > h.pcx_batched_lds_bytes(50, 20, 2)


@pytest.mark.parametrize("shape", [(0, 4), (65, 4), (4, 33), (4, 0), (-1, 4)])
def test_plan_names_the_first_bad_round(shape):
    from pyconsensus_amd import _lib

    rc, _, _, bad = _plan([(3, 3), (64, 32), shape, (70, 70)], 0)
    assert rc == -1 and bad == 2
    assert b"round 2" in _lib.lib().pcx_last_error()


def test_plan_refuses_kmeans_and_unknown_algorithms():
    from pyconsensus_amd import _lib

    for alg in (5, 8, -1):
        rc, _, _, bad = _plan([(3, 3)], alg)
        assert rc == -1 and bad == -1
    _plan([(3, 3)], 5)
    assert b"k-means" in _lib.lib().pcx_last_error()


def test_plan_accepts_an_empty_batch():
    from pyconsensus_amd import _lib

    totals, lds, bad = (C.c_int64 * 3)(1, 1, 1), C.c_int64(1), C.c_int64(1)
    assert _lib.lib().pcx_ragged_plan(0, None, None, 0, totals, C.byref(lds), C.byref(bad)) == 0
    assert list(totals) == [0, 0, 0] and lds.value == 0 and bad.value == -1
    # every output is optional
    n = np.array([3], dtype=np.int32)
    assert _lib.lib().pcx_ragged_plan(1, n.ctypes.data, n.ctypes.data, 0, None, None, None) == 0


def test_python_plan():
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import ragged_plan

    totals, lds = ragged_plan([(3, 4), (64, 32)])
    assert totals == (67, 36, 12 + 2048) and lds == _lib.lib().pcx_batched_lds_bytes(64, 32, 0)
    with pytest.raises(_lib.PcxError, match="round 1"):
        ragged_plan([(3, 4), (65, 2)])
    with pytest.raises(_lib.PcxError, match="k-means"):
        ragged_plan([(3, 4)], "k-means")


def test_abi_version_and_exports():
    from pyconsensus_amd import _abi, _lib

    h = _lib.lib()
    assert h.pcx_abi_version() == 9 == _abi.ABI_VERSION
    assert hasattr(h, "pcx_ragged_plan") and hasattr(h, "pcx_consensus_ragged_f64")
    import pyconsensus_amd

    assert callable(pyconsensus_amd.consensus_ragged) and callable(pyconsensus_amd.consensus_many)


def test_ragged_struct_size_and_offsets_match_c():
    """pcx_ragged as gcc lays it out from include/pcx.h equals the ctypes mirror, and the structs
    the call shares with the batched regime kept their sizes."""
    from pyconsensus_amd import _abi

    structs = {"pcx_ragged": _abi.Ragged, "pcx_batch_result": _abi.BatchResult, "pcx_batch": _abi.Batch}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pcx.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    for cname, py in structs.items():
        assert int(out["%s size" % cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)


@pytest.fixture
def no_library(monkeypatch):
    """Any libpcx call fails the test: the argument errors come first."""
    from pyconsensus_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "bind_stream", boom)


def test_argument_errors_come_before_any_library_call(no_library):
    from pyconsensus_amd.batched import consensus_ragged

    a, b = np.ones((3, 2)), np.ones((4, 5))
    with pytest.raises(ValueError, match=r"reports\[1\]"):
        consensus_ragged([a, np.ones((2, 3, 4))])  # a 3-D entry
    with pytest.raises(ValueError, match=r"reports\[0\]"):
        consensus_ragged([np.ones(3)])
    with pytest.raises(ValueError, match="one vector per round"):
        consensus_ragged([a, b], reputation=[np.ones(3)])
    with pytest.raises(ValueError, match=r"reputation\[1\]"):
        consensus_ragged([a, b], reputation=[np.ones(3), np.ones(5)])
    with pytest.raises(ValueError, match=r"lo\[0\]"):
        consensus_ragged([a, b], scaled=[np.zeros(2), np.zeros(5)], lo=[np.zeros(3), np.zeros(5)],
                         hi=[np.ones(2), np.ones(5)])
    with pytest.raises(ValueError, match="together"):
        consensus_ragged([a, b], scaled=[np.zeros(2), np.zeros(5)])
    with pytest.raises(ValueError, match="aux_scores"):
        consensus_ragged([a, b], algorithm="cokurtosis")
    with pytest.raises(ValueError, match=r"aux_scores\[1\]"):
        consensus_ragged([a, b], algorithm="cokurtosis", aux_scores=[np.ones(3), np.ones(5)])
    with pytest.raises(NotImplementedError):
        consensus_ragged([a, b], algorithm="no-such")
