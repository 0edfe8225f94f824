"""k-means in ragged batches and the simulator, the parts that need no GPU:
the code-book layout and its refusals, the structs, the host twin of the books kernel, and the
precondition that makes the GPU comparisons on bits meaningful."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import kmeans_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401

    return sys.modules["pyconsensus_amd.simulate"]


# ------------------------------------------------------------------ the plan
def test_kmeans_plan_offsets_and_the_empty_batch():
    from pyconsensus_amd.batched import kmeans_plan

    shapes = [(10, 3), (100, 5), (4, 3), (64, 32), (65, 1), (256, 64), (1, 1)]
    off = kmeans_plan(shapes, 3)
    ks = [4, 10, 2, 8, 9, 16, 1]
    assert off.dtype == np.int64 and off.tolist() == [0] + list(np.cumsum([3 * k for k in ks]))
    assert [K.rule(n) for n, _ in shapes] == ks
    off = kmeans_plan(shapes, 20, k=[1, 16, 4, 8, 16, 1, 1])  # the caller's sizes, up to the bounds
    assert off.tolist() == [0] + list(np.cumsum([20 * k for k in (1, 16, 4, 8, 16, 1, 1)]))
    assert kmeans_plan([], 5).tolist() == [0]


@pytest.mark.parametrize("shape, k, bound", [((10, 3), 0, 8), ((10, 3), 11, 8), ((10, 3), 9, 8), ((100, 5), 17, 16),
                                             ((5, 3), 6, 5), ((3, 64), 4, 3), ((64, 33), 17, 16)])
def test_kmeans_plan_refuses_a_code_book_size_with_the_round_named(shape, k, bound):
    from pyconsensus_amd import _lib

    n = np.array([7, shape[0]], dtype=np.int32)
    e = np.array([2, shape[1]], dtype=np.int32)
    kk = np.array([3, k], dtype=np.int32)
    bad, off = C.c_int64(-5), np.full(3, -1, dtype=np.int64)
    rc = _lib.lib().pcx_kmeans_plan(2, n.ctypes.data, e.ctypes.data, kk.ctypes.data, 3, off.ctypes.data, C.byref(bad))
    assert rc == -1 and bad.value == 1
    msg = _lib.lib().pcx_last_error().decode()
    assert "round 1" in msg and "%d rows" % k in msg and "[1, %d]" % bound in msg


def test_kmeans_plan_refuses_restarts_and_shapes():
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import kmeans_plan

    with pytest.raises(_lib.PcxError, match="restarts must be >= 1"):
        kmeans_plan([(10, 3)], 0)
    with pytest.raises(_lib.PcxError, match="round 1 is 257 x 3"):
        kmeans_plan([(10, 3), (257, 3)], 2)
    with pytest.raises(_lib.PcxError, match="round 0 is 3 x 65"):
        kmeans_plan([(3, 65)], 2)


def test_ragged_plan_kmeans_counts_only_the_kmeans_rounds():
    from pyconsensus_amd import _lib
    from pyconsensus_amd.batched import param_sets, ragged_plan, ragged_plan_kmeans, ragged_plan_params

    defaults = dict(algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
                    hierarchy_threshold=0.5, cluster_threshold=None)
    shapes = [(10, 3), (100, 5), (17, 5), (65, 2), (4, 3)]
    per_round = [{"algorithm": "k-means"}, {}, {"algorithm": "k-means", "alpha": 0.3}, {"algorithm": "k-means"},
                 {"algorithm": "hierarchical"}]
    sets, of = param_sets(per_round, defaults, "per_round")
    totals, launches, off = ragged_plan_kmeans(shapes, sets, of, 3)
    assert totals == (196, 18, 10 * 3 + 100 * 5 + 17 * 5 + 65 * 2 + 4 * 3)
    assert off.tolist() == [0, 12, 12, 27, 54, 54]
    # k-means rounds are clustering rounds: they add no launch to the hierarchical round's
    plain = [dict(q, algorithm="hierarchical") if q["algorithm"] == "k-means" else q for q in sets]
    assert launches == ragged_plan_params(shapes, plain, of)[1] == 3
    # the shared opt-in of ragged_plan
    t2, n2, off2 = ragged_plan(shapes, "k-means", wide=True, kmeans_restarts=2)
    assert t2 == totals and n2 == 2 and off2.tolist() == [0, 8, 28, 38, 56, 60]
    with pytest.raises(_lib.PcxError, match="round 1 is 100 x 5"):
        ragged_plan(shapes, "k-means", kmeans_restarts=2)
    with pytest.raises(_lib.PcxError, match=r"round 2 \(17 x 5\) has a code book of 9 rows"):
        ragged_plan_kmeans(shapes, sets, of, 3, k=[4, 0, 9, 9, 0])
    with pytest.raises(_lib.PcxError, match="restarts must be >= 1"):
        ragged_plan_kmeans(shapes, sets, of, 0)
    # a batch without a k-means round reads no book
    assert ragged_plan_kmeans(shapes, [defaults], np.zeros(5, dtype=np.int32), 0)[2].tolist() == [0] * 6
    # and what pcx_ragged_plan_params refuses of a set is refused in its words
    with pytest.raises(_lib.PcxError, match="parameter set 0: big-five needs max_components >= 1"):
        ragged_plan_kmeans(shapes, [dict(defaults, algorithm="big-five", max_components=0)], np.zeros(5, np.int32), 3)


def test_the_old_refusals_still_stand():
    """One assertion per old entry's pure plan function: without the new entries k-means is refused in
    the old words."""
    from pyconsensus_amd import _abi, _lib
    from pyconsensus_amd.batched import ragged_plan, ragged_plan_params

    S = _sim()
    assert _lib.lib().pcx_abi_version() == 9
    with pytest.raises(_lib.PcxError, match="k-means is not supported"):
        ragged_plan([(3, 4)], "k-means")
    with pytest.raises(_lib.PcxError, match="k-means is not supported"):
        ragged_plan([(3, 4)], "k-means", wide=True)
    q = dict(algorithm="k-means", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
             hierarchy_threshold=0.5, cluster_threshold=None)
    with pytest.raises(_lib.PcxError, match="parameter set 0: k-means is not supported"):
        ragged_plan_params([(3, 4)], [q], [0])
    with pytest.raises(_lib.PcxError, match="k-means is not simulated"):
        S.sweep_plan([K.cell(2, 5, 3, 1)], algorithm="k-means")
    with pytest.raises(_lib.PcxError, match="cell 0: k-means is not simulated"):
        S.sweep_plan([dict(K.cell(2, 5, 3, 1), algorithm="k-means")])
    with pytest.raises(_lib.PcxError, match="k-means is not simulated"):
        S.study_check([K.cell(2, 5, 3, 1)], algorithm="k-means")
    s = S._sim(2, 5, 3, 1, 0, 0.3, 0.5, 0.1, 0.1, 0.25, algorithm="k-means")
    rounds = _abi.SimRounds()
    assert _lib.lib().pcx_sim_generate_host(C.byref(s), 0, C.byref(rounds)) == -1
    assert "k-means is not simulated" in _lib.lib().pcx_last_error().decode()
    # the new pure check lets it through, and keeps cokurtosis out
    sw, arr, _, _ = S._sweep([K.cell(2, 5, 3, 1)], 1, algorithm="k-means")
    bad = C.c_int64(-2)
    assert _lib.lib().pcx_sim_study_kmeans_check(C.byref(sw), None, None, 20, C.byref(bad)) == 0
    assert _lib.lib().pcx_sim_study_kmeans_check(C.byref(sw), None, None, 0, C.byref(bad)) == -1
    sw, arr, _, _ = S._sweep([K.cell(2, 5, 3, 1)], 1, algorithm="cokurtosis")
    assert _lib.lib().pcx_sim_study_kmeans_check(C.byref(sw), None, None, 20, C.byref(bad)) == -1
    assert "cokurtosis is not simulated" in _lib.lib().pcx_last_error().decode()


def test_new_struct_size_and_offsets_match_c():
    """pcx_kmeans_books as gcc lays it out from include/pcx.h equals the ctypes mirror; the structs
    the new entries share with the old ones kept their sizes."""
    from pyconsensus_amd import _abi

    structs = {"pcx_kmeans_books": _abi.KmeansBooks, "pcx_round_params": _abi.RoundParams, "pcx_ragged": _abi.Ragged,
               "pcx_sim": _abi.Sim, "pcx_sim_sweep": _abi.SimSweep}
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
    assert C.sizeof(_abi.KmeansBooks) == 24


# ------------------------------------------------------------------ the host draws
def test_kmeans_draws_ragged_consumes_the_state_as_kmeans_draws_round_by_round():
    from pyconsensus_amd.batched import kmeans_draws, kmeans_draws_ragged

    ns = [10, 17, 4, 100, 1, 64]
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    got = kmeans_draws_ragged(ns, 3, a)
    want = [kmeans_draws(1, n, 3, b)[0] for n in ns]
    assert [g.shape for g in got] == [(3, K.rule(n)) for n in ns]
    assert all(g.dtype == np.int32 and (g == w).all() for g, w in zip(got, want))
    assert a.randint(1 << 30) == b.randint(1 << 30)  # both states stand where the other does
    # the global state by default, and the caller's k
    np.random.seed(5)
    g1 = kmeans_draws_ragged([9, 30], 2, k=[2, 7])
    after = np.random.get_state()[1].copy()
    rs = np.random.RandomState(5)
    assert (g1[0] == [rs.choice(9, 2, replace=False) for _ in range(2)]).all()
    assert (g1[1] == [rs.choice(30, 7, replace=False) for _ in range(2)]).all()
    assert (after == rs.get_state()[1]).all()


# ------------------------------------------------------------------ the device source's host twin
NK = sorted({(N, K.rule(N)) for N, _ in K.WAVE_SHAPES + K.WG_SHAPES})


def test_host_books_are_in_range_and_distinct():
    S = _sim()
    for N, k in NK:
        b = S.kmeans_books_host(40, N, t=2, seed=99, restarts=5)
        assert b.shape == (40, 5, k) and b.dtype == np.int32
        assert b.min() >= 0 and b.max() < N
        assert all(len(set(row)) == k for row in b.reshape(-1, k).tolist()), (N, k)


def test_host_books_depend_on_seed_round_restart_and_timestep_alone():
    S = _sim()
    a = S.kmeans_books_host(6, 50, t=3, seed=7, restarts=4)
    assert (a == S.kmeans_books_host(6, 50, t=3, seed=7, restarts=4)).all()
    assert (a[:3, :2] == S.kmeans_books_host(3, 50, t=3, seed=7, restarts=2)).all()  # no launch geometry in a draw
    assert all((a[:, r] != a[:, r + 1]).any() for r in range(3))      # across restarts
    assert (a != S.kmeans_books_host(6, 50, t=4, seed=7, restarts=4)).any()  # across timesteps
    assert (a != S.kmeans_books_host(6, 50, t=3, seed=8, restarts=4)).any()
    assert (a[0] != a[1]).any()


def test_host_books_are_uniform_over_the_rows():
    """N = 10, k = 4 over 20,000 (round, restart) draws: every row's frequency lies within five
    binomial standard errors of k / N."""
    S = _sim()
    b = S.kmeans_books_host(1000, 10, t=0, seed=20261020, restarts=20)
    n, p = 20000, 4 / 10
    freq = np.bincount(b.ravel(), minlength=10) / n
    assert b.shape == (1000, 20, 4) and np.abs(freq - p).max() <= 5 * np.sqrt(p * (1 - p) / n), freq


def test_a_sweeps_books_are_its_cells_own():
    S = _sim()
    cells = [K.cell(3, 10, 3, 5), K.cell(2, 100, 5, 7), K.cell(4, 1, 1, 5), K.cell(2, 256, 64, 5), K.cell(3, 10, 3, 5)]
    books, off = S.sweep_kmeans_books_host(cells, t=1, restarts=3)
    assert off.tolist() == [0] + list(np.cumsum([3 * K.rule(c["reporters"]) for c in cells for _ in range(c["rounds"])]))
    b = 0
    for c in cells:
        k = K.rule(c["reporters"])
        mine = books[off[b]:off[b + c["rounds"]]].reshape(c["rounds"], 3, k)
        assert (mine == S.kmeans_books_host(c["rounds"], c["reporters"], t=1, seed=c["seed"], restarts=3)).all()
        b += c["rounds"]
    # cells that share seed, shape and rounds draw the same books: the common random numbers of a pair
    assert (books[off[0]:off[3]] == books[off[11]:off[14]]).all()


def test_the_generators_other_streams_are_untouched():
    """generate_host for one fixed seed equals a recording made before the KMEANS stream existed."""
    S = _sim()
    want = np.load(os.path.join(ROOT, "tests", "golden", "sim_streams_2x3x4.npz"))
    got = S.generate_host(2, 3, 4, t=1, seed=20261020, liar_frac=0.4, collude_frac=0.5, distort=0.2, na_frac=0.2,
                          scaled_frac=0.5)
    assert set(got) == set(want.files)
    for name in want.files:
        assert K.same_bits(got[name], want[name]), name


# ------------------------------------------------------------------ the precondition of the GPU tests
def test_a_rounds_result_depends_on_its_own_book():
    """A kernel that read another round's book must not pass the GPU comparisons: under the C SPEC, at
    one restart, exchanging a round's book for a second draw changes this_rep's bits in at least half
    of the test rounds with N >= 17 and E >= 5.  And the test rounds reach both ends: a NaN this_rep
    (no finite distortion, or equal cluster sizes) in at least one, finite values in at least half."""
    changed = total = nan_rounds = finite_rounds = rounds = 0
    first, second = K.books("wide", 1), K.books("wide", 1, seed=1)
    for shape, (idx, b1) in K.shape_batches("wide", first).items():
        a = K.spec_shape(shape, b1)["this_rep"]
        rounds += len(idx)
        nan_rounds += int(np.isnan(a).any(axis=1).sum())
        finite_rounds += int(np.isfinite(a).all(axis=1).sum())
        if shape[0] >= 17 and shape[1] >= 5:
            b2 = np.stack([second[b] for b in idx])
            c = K.spec_shape(shape, b2)["this_rep"]
            assert (b1 != b2).any()
            total += len(idx)
            changed += sum(not K.same_bits(a[r], c[r]) for r in range(len(idx)))
    print("rounds whose this_rep changes with the book: %d of %d; NaN rounds %d, finite rounds %d of %d"
          % (changed, total, nan_rounds, finite_rounds, rounds))
    assert total >= 20 and 2 * changed >= total
    assert nan_rounds >= 1 and 2 * finite_rounds >= rounds
