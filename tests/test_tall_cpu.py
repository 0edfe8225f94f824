"""Tall batched rounds without a GPU: the SPEC built for 1024 reporters against the 256 build, the
tall route and its LDS plan (pcx_tall_route, pcx_tall_lds_bytes, pcx_tall_plan -- pure functions), the
coverage of the inputs that test_tall_gpu.py runs, checked on the SPEC alone, and the refusal without
a GPU."""
import numpy as np
import pytest

import tall_cases as T
from oracle import pcx_oracle_c as OC
from pyconsensus_amd import _abi, synthetic

ALGS = _abi.ALGORITHMS


def _lib():
    from pyconsensus_amd import _lib

    return _lib.lib()


@pytest.mark.parametrize("shape", [(65, 33), (256, 64), (200, 34)], ids=T.sid)
def test_spec_1024_equals_spec_256(shape):
    """The reporter limit is a build parameter of the SPEC and nothing else: every output of the two
    builds agrees bit for bit where both run."""
    N, E = shape
    R, sc, lo, hi, rep = synthetic.rounds(8, N, E, seed=5 + N)
    batches = [(R, dict(reputation=rep, scaled=sc, lo=lo, hi=hi))]
    Rc, kwc = T.crafted_rounds(N, E, "bounds")
    batches.append(T.take(Rc, kwc, np.arange(0, T.MASK_B, T.MASK_GROUP)))
    for Rb, kw in batches:
        for alg in ("PCA", "big-five"):
            more = T._algorithm_kw(alg, len(Rb), N, E)
            a, b = OC.batched(Rb, **kw, **more, threads=8), T.spec(Rb, **kw, **more)
            assert set(a) == set(b)
            for k in a:
                assert T.bits_equal(a[k], b[k]).all(), (shape, alg, k)
    with pytest.raises(ValueError):  # (and the 256 build refuses what only the 1024 build takes)
        OC.batched(np.ones((1, 300, 2)))


def test_tall_route_extends_the_batched_route():
    from pyconsensus_amd.batched import kmeans_k, route, tall_plan

    h = _lib()
    for name, alg in ALGS.items():
        for N in list(range(1, 257, 5)) + [64, 65, 255, 256]:
            for E in (1, 2, 31, 32, 33, 63, 64):
                k = kmeans_k(N)
                assert h.pcx_tall_route(N, E, alg, k) == h.pcx_batched_route(N, E, alg, k), (name, N, E)
    for name in ("k-means", "hierarchical", "clusterfeck"):  # the clusterings stay where they are
        for N in (257, 300, 512, 1024, 1025):
            for E in (1, 20, 64, 65):
                k = kmeans_k(N)
                assert h.pcx_tall_route(N, E, ALGS[name], k) == h.pcx_batched_route(N, E, ALGS[name], k) == T.SCHEDULER
    for name in T.PLAIN:
        assert h.pcx_tall_route(1025, 5, ALGS[name], 1) == T.SCHEDULER
        assert h.pcx_tall_route(300, 65, ALGS[name], 1) == T.SCHEDULER
        assert h.pcx_tall_lds_bytes(1025, 5, ALGS[name]) == 0 and h.pcx_tall_lds_bytes(300, 65, ALGS[name]) == 0
        assert h.pcx_tall_lds_bytes(256, 64, ALGS[name]) == 0  # not a tall shape: the workgroup route's
        assert h.pcx_tall_route(257, 10, ALGS[name], 1) == T.TALL
        assert h.pcx_batched_route(257, 10, ALGS[name], 1) == T.SCHEDULER  # the default route is unchanged
    assert h.pcx_tall_route(300, 20, 8, 1) == -1 and h.pcx_tall_route(0, 20, 0, 1) == -1
    assert route(300, 20, "PCA", tall=True) == "tall" and route(300, 20, "PCA") == "scheduler"
    assert route(300, 20, "hierarchical", tall=True) == "scheduler"
    assert route(100, 50, "PCA", tall=True) == "workgroup" and route(50, 20, "PCA", tall=True) == "wave"
    assert tall_plan(100, 50) is None and tall_plan(300, 20)["waves"] == 4


def test_tall_lds_follows_the_plan_everywhere():
    """Every N in 257..1024 and E in 1..64: the route says tall exactly where the LDS figure is in
    (0, 160 KB]; the figure is the plan's, restated; a plan never asks for more rows than there are."""
    import ctypes as C

    h = _lib()
    out = (C.c_int32 * 4)()
    seen = {name: 0 for name in T.PLAIN}
    for name in T.PLAIN:
        alg = ALGS[name]
        for N in range(257, 1025):
            for E in range(1, 65):
                r = h.pcx_tall_route(N, E, alg, 1)
                lds = h.pcx_tall_lds_bytes(N, E, alg)
                assert r in (T.TALL, T.SCHEDULER), (name, N, E, r)
                assert (r == T.TALL) == (0 < lds <= T.LDS_LIMIT), (name, N, E, r, lds)
                rc = h.pcx_tall_plan(N, E, alg, out)
                assert (rc == 0) == (r == T.TALL)
                if r != T.TALL:
                    assert lds == 0 and tuple(out) == (0, 0, 0, 0)
                    continue
                seen[name] += 1
                waves, rows, chunks, threads = tuple(out)
                assert waves in (1, 2, 4) and threads % 64 == 0 and waves <= threads // 64
                assert rows % 4 == 0 and 4 <= rows <= N and chunks >= 1
                nb = N >> 2
                if E > 1:
                    assert (chunks - 1) * (rows // 4) < nb <= chunks * (rows // 4), (name, N, E, tuple(out))
                assert lds == T.lds_from_plan(N, E, name, tuple(out)), (name, N, E, tuple(out))
    # PCA, absolute and cokurtosis fit everywhere; the Jacobi algorithms' second matrix does not
    for name in ("PCA", "absolute", "cokurtosis"):
        assert seen[name] == 768 * 64
    for name in ("big-five", "fixed-variance"):
        assert 0 < seen[name] < 768 * 64
        assert h.pcx_tall_route(1024, 64, ALGS[name], 1) == T.SCHEDULER
    cap = T.bigfive_capacity()
    assert 512 < cap < 1024 and h.pcx_tall_route(cap + 1, 64, ALGS["big-five"], 1) == T.SCHEDULER


def test_gpu_shapes_take_every_plan_branch():
    plans = {s: T.plan(*s) for s in T.gpu_shapes()}
    assert all(p is not None for p in plans.values()), plans
    assert {p[0] for p in plans.values()} == {4, 2, 1}
    assert plans[257, 5, "PCA"][0] == 4 and plans[513, 33, "PCA"][0] == 2 and plans[1024, 64, "PCA"][0] == 1
    one = [s for s, p in plans.items() if p[2] == 1]
    ragged = [s for s, p in plans.items() if p[2] > 1 and (s[0] >> 2) % (p[1] // 4)]
    assert one and ragged, plans
    assert (1024, 64, "PCA") in ragged and plans[1024, 64, "PCA"][2] >= 3  # several chunks, the last shorter
    assert (640, 62, "PCA") in ragged
    assert plans[1024, 1, "PCA"][2] == 1  # E == 1: no block partials


@pytest.mark.parametrize("shape", T.BATTERY_SHAPES, ids=T.sid)
def test_side_battery_reaches_its_exits_on_the_spec(shape):
    R, kw, kinds = T.side_inputs(shape)
    T.side_preconditions(shape, T.side_spec(shape), kinds)


@pytest.mark.parametrize("config", T.CONFIGS)
@pytest.mark.parametrize("shape", T.BATTERY_SHAPES, ids=T.sid)
def test_mask_battery_on_the_spec(shape, config):
    R, kw = T.mask_inputs(shape, config)
    T.mask_preconditions(shape, config, R, kw, T.mask_spec(shape, config))


def test_nan_battery_ranks_nan_values_on_the_spec():
    R, kw, groups = T.nan_inputs()
    T.nan_preconditions(R, T.nan_spec(), groups)


def test_fixed_variance_case_stops_at_different_counts():
    c = T.synth_spec((300, 40), "fixed-variance")
    assert len(set(c["components"].tolist())) > 1


def test_tall_needs_a_gpu_like_the_default(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (the same test where a GPU is visible)
    from pyconsensus_amd.batched import consensus_batched

    R, sc, lo, hi, rep = synthetic.rounds(2, 300, 4, seed=1)
    errs = []
    for tall in (False, True):
        with pytest.raises(Exception) as ei:
            consensus_batched(R, rep, sc, lo, hi, tall=tall)
        errs.append((type(ei.value), str(ei.value)))
    assert errs[0] == errs[1]
