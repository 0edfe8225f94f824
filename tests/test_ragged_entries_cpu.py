"""The four ragged plan entries agree where they describe the same rounds (pcx_ragged.cpp: one plan
pass for the shared-parameter entries, one table plan for the parameter-set and k-means entries).
Needs no GPU."""
import ctypes as C

import numpy as np

# one-wave rounds and workgroup rounds of two launch classes, in six rounds
SHAPES = [(1, 1), (5, 3), (64, 32), (65, 3), (256, 64), (100, 50)]
WAVE = [s for s in SHAPES if s[0] <= 64 and s[1] <= 32]
DEFAULTS = dict(algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
                hierarchy_threshold=0.5, cluster_threshold=None)


def test_the_plan_entries_report_the_same_totals_and_launches():
    from pyconsensus_amd.batched import ragged_plan, ragged_plan_kmeans, ragged_plan_params

    assert WAVE == SHAPES[:3]
    for shapes in (SHAPES, WAVE):
        of = np.zeros(len(shapes), dtype=np.int32)
        for algorithm in ("PCA", "hierarchical", "big-five"):
            sets = [dict(DEFAULTS, algorithm=algorithm)]
            totals, counts, lds4 = ragged_plan(shapes, algorithm, wide=True)
            t_params, n_params = ragged_plan_params(shapes, sets, of)
            t_kmeans, n_kmeans, offsets = ragged_plan_kmeans(shapes, sets, of, 0)  # no k-means set: books unread
            assert totals == t_params == t_kmeans
            assert totals == (sum(n for n, _ in shapes), sum(e for _, e in shapes), sum(n * e for n, e in shapes))
            assert n_params == n_kmeans == sum(c > 0 for c in counts)  # one algorithm: a launch per class in use
            assert offsets.tolist() == [0] * (len(shapes) + 1)
            assert sum(counts) == len(shapes) and counts[0] == len(WAVE)
    # the one-wave kernel and two launch classes of the workgroup kernel (256 x 64 alone in its class)
    assert ragged_plan(SHAPES, "PCA", wide=True)[1] == (3, 0, 1, 2)
    # under big-five the three workgroup rounds need the LDS of three classes: every class is reached
    assert ragged_plan(SHAPES, "big-five", wide=True)[1] == (3, 1, 1, 1)


def test_the_narrow_plan_is_the_wide_plan_of_wave_sized_rounds():
    from pyconsensus_amd.batched import ragged_plan

    for algorithm in ("PCA", "hierarchical", "big-five"):
        totals, lds = ragged_plan(WAVE, algorithm)
        w_totals, counts, lds4 = ragged_plan(WAVE, algorithm, wide=True)
        assert totals == w_totals and lds == lds4[0] and counts == (len(WAVE), 0, 0, 0) and lds4[1:] == (0, 0, 0)


def test_the_entries_take_null_books_and_null_sizes():
    """pcx_ragged_plan_kmeans with books NULL where no set is k-means, and pcx_kmeans_plan with k NULL:
    restarts * ceil(sqrt(N)) prefix sums."""
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import _params_array

    n = np.array([s[0] for s in SHAPES], dtype=np.int32)
    e = np.array([s[1] for s in SHAPES], dtype=np.int32)
    of = np.zeros(len(SHAPES), dtype=np.int32)
    arr = _params_array([DEFAULTS])
    totals, nl, bad_r, bad_p = (C.c_int64 * 3)(), C.c_int64(-1), C.c_int64(-2), C.c_int64(-2)
    offsets = np.full(len(SHAPES) + 1, -1, dtype=np.int64)
    _lib.check(_lib.lib().pcx_ragged_plan_kmeans(len(SHAPES), n.ctypes.data, e.ctypes.data, 1, C.cast(arr, C.c_void_p),
                                                 of.ctypes.data, None, totals, C.byref(nl), offsets.ctypes.data,
                                                 C.byref(bad_r), C.byref(bad_p)))
    assert tuple(totals) == (int(n.sum()), int(e.sum()), int((n.astype(np.int64) * e).sum()))
    assert nl.value == 3 and bad_r.value == -1 and bad_p.value == -1 and offsets.tolist() == [0] * 7
    for restarts in (1, 2, 20):
        off = np.full(len(SHAPES) + 1, -1, dtype=np.int64)
        _lib.check(_lib.lib().pcx_kmeans_plan(len(SHAPES), n.ctypes.data, e.ctypes.data, None, restarts, off.ctypes.data,
                                              C.byref(bad_r)))
        ks = [int(np.ceil(np.sqrt(N))) for N, _ in SHAPES]
        assert ks == [1, 3, 8, 9, 16, 10]
        assert off.tolist() == [0] + list(np.cumsum([restarts * k for k in ks])) and bad_r.value == -1
