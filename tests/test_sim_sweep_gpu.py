"""Simulator sweeps on the GPU: cells of different shapes, rates and seeds in one call.

The contract is the specification: cell c's slice of every output of a sweep is byte for byte what
``simulate`` gives for that cell alone.  Everything is compared bit for bit, NaNs in the same places:
the device generator against the host generator, the metrics and the per-cell summaries against the
numpy restatement of DESIGN.md 5.4, whole sweeps against per-cell ``simulate`` and against a host
replay that does not go through ``simulate``.
"""
import sys

import numpy as np
import pytest

import sim_sweep_cases as W

pytestmark = pytest.mark.gpu


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401  (the module: the package exports the function of that name)

    return sys.modules["pyconsensus_amd.simulate"]


def _sync():
    import torch

    torch.cuda.synchronize()


def _host(x):
    return x.cpu().numpy()


_REFERENCE = {}


def reference(c, T, algorithm="PCA", **kw):
    """``simulate`` of one cell alone (computed once per cell and parameters, left unchanged)."""
    key = (tuple(sorted(c.items())), T, algorithm, tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        r = _sim().simulate(c["rounds"], c["reporters"], c["events"], T, seed=c["seed"], algorithm=algorithm,
                            keep_rounds=True, keep_outputs=True, **dict(W.rates(c), **kw))
        _sync()
        _REFERENCE[key] = {"metrics": _host(r["metrics"]), "summary": _host(r["summary"]),
                           "reputation": _host(r["reputation"]),
                           "rounds": {k: _host(v) for k, v in r["rounds"].items()},
                           "outputs": {k: _host(r["outputs"][k]) for k in ("old_rep", "smooth_rep", "outcomes_final")}}
    return _REFERENCE[key]


def run_sweep(cells, T, algorithm="PCA", **kw):
    r = _sim().sweep(cells, T, algorithm=algorithm, keep_rounds=True, keep_outputs=True, **kw)
    _sync()
    return {"metrics": _host(r["metrics"]), "summary": _host(r["summary"]), "reputation": _host(r["reputation"]),
            "rounds": {k: _host(v) for k, v in r["rounds"].items()},
            "outputs": {k: _host(v) for k, v in r["outputs"].items()}, "offsets": r["offsets"]}


def assert_cells_equal_simulate(cells, T, algorithm="PCA", **kw):
    got = run_sweep(cells, T, algorithm, **kw)
    off = got["offsets"]
    B = sum(c["rounds"] for c in cells)
    assert got["metrics"].shape == (T, B, 6) and got["summary"].shape == (T, len(cells), 6)
    for c, k in enumerate(cells):
        want = reference(k, T, algorithm, **kw)
        where = (algorithm, c)
        assert W.same_bits(got["metrics"][:, off["rounds"][c]:off["rounds"][c + 1]], want["metrics"]), where
        assert W.same_bits(got["summary"][:, c], want["summary"]), where
        assert W.same_bits(W.cell_slice(got["reputation"], off, "reporters", c), want["reputation"].reshape(-1)), where
        for name in W.ROUNDS:
            assert W.same_bits(W.cell_slice(got["rounds"][name], off, W.OFFSET_OF[name], c),
                               want["rounds"][name].reshape(-1)), where + (name,)
        for name in ("old_rep", "smooth_rep", "outcomes_final"):
            assert W.same_bits(W.cell_slice(got["outputs"][name], off, W.OFFSET_OF[name], c),
                               want["outputs"][name].reshape(-1)), where + (name,)
    return got


# ------------------------------------------------------------------ generation
@pytest.mark.parametrize("cells", [W.HOST_SWEEP, W.SMALL_SWEEP], ids=["host-sweep", "small-rounds"])
@pytest.mark.parametrize("t", [0, 2])
def test_generate_matches_the_host_generator(gpu_lib, cells, t):
    S = _sim()
    dev = S.sweep_generate(cells, t)
    host = S.sweep_generate_host(cells, t)
    for name in W.ROUNDS:
        assert W.same_bits(_host(dev[name]), host[name]), name


def test_generate_skips_null_outputs(gpu_lib):
    S = _sim()
    host = S.sweep_generate_host(W.HOST_SWEEP, 1)
    for fields in (("reports",), ("liar", "truth"), ("scaled", "lo", "hi")):
        dev = S.sweep_generate(W.HOST_SWEEP, 1, fields=fields)
        assert set(dev) == set(fields) | {"offsets"}
        for name in fields:
            assert W.same_bits(_host(dev[name]), host[name]), name


# ------------------------------------------------------------------ metrics and summaries
def _random_rounds(rng, cells):
    """Hand-built flat rounds and consensus outputs (no generator, no consensus), and per cell the same
    as equal-shape arrays."""
    flat = {k: [] for k in ("scaled", "lo", "hi", "truth", "liar", "old", "smooth", "outcomes")}
    per_cell = []
    for k in cells:
        R, N, E = k["rounds"], k["reporters"], k["events"]
        d = {"scaled": rng.integers(0, 2, (R, E)).astype(np.uint8)}
        d["lo"] = np.where(d["scaled"] != 0, rng.integers(-50, 0, (R, E)), 1).astype(np.float64)
        d["hi"] = np.where(d["scaled"] != 0, rng.integers(1, 50, (R, E)), 2).astype(np.float64)
        d["truth"] = np.where(d["scaled"] != 0, rng.integers(-50, 50, (R, E)) / 4.0, rng.integers(1, 3, (R, E)))
        d["truth"] = d["truth"].astype(np.float64)
        # outcomes: the truth, near it, far from it, and NaN
        pick = rng.integers(0, 4, (R, E))
        width = d["hi"] - d["lo"]
        d["outcomes"] = np.select([pick == 0, pick == 1, pick == 2],
                                  [d["truth"], d["truth"] + 0.05 * width, d["truth"] + 0.5 * width], np.nan)
        d["liar"] = rng.integers(0, 4, (R, N)).astype(np.uint8)
        d["old"] = rng.random((R, N)) * np.exp(rng.normal(0, 6, (R, N)))  # magnitudes apart: the order shows
        d["smooth"] = rng.random((R, N)) * np.exp(rng.normal(0, 6, (R, N)))
        per_cell.append(d)
        for name in flat:
            flat[name].append(d[name].reshape(-1))
    return {name: np.concatenate(v) for name, v in flat.items()}, per_cell


def test_metrics_and_per_cell_summaries(gpu_lib):
    """Cells of 1, 255, 256, 257 and 600 rounds of different shapes in one sweep: every round's metrics
    and every cell's means in the summary order, against the numpy restatement applied per cell."""
    S = _sim()
    cells = [W.cell(1, 5, 4, 0), W.cell(255, 6, 3, 0), W.cell(256, 3, 7, 0), W.cell(257, 9, 2, 0), W.cell(600, 4, 5, 0)]
    flat, per_cell = _random_rounds(np.random.default_rng(20261020), cells)
    tol = 0.1
    got = S.sweep_metrics(cells, flat, flat["old"], flat["smooth"], flat["outcomes"], scaled_tol=tol)
    m, s, off = _host(got["metrics"]), _host(got["summary"]), got["offsets"]
    assert m.shape == (sum(c["rounds"] for c in cells), 6) and s.shape == (len(cells), 6)
    for c, d in enumerate(per_cell):
        want = W.np_metrics(d["scaled"], d["lo"], d["hi"], d["truth"], d["liar"], d["old"], d["smooth"],
                            d["outcomes"], tol)
        assert W.same_bits(m[off["rounds"][c]:off["rounds"][c + 1]], want), c
        assert W.same_bits(s[c], W.np_summary(want)), c
        if cells[c]["rounds"] >= 255:  # (the order is observable: another one gives other bits)
            assert not W.same_bits(W.np_summary(want), want.sum(axis=0) / float(len(want)))
    # summary NULL: the metrics alone
    alone = S.sweep_metrics(cells, flat, flat["old"], flat["smooth"], flat["outcomes"], scaled_tol=tol, summary=False)
    assert alone["summary"] is None and W.same_bits(_host(alone["metrics"]), m)


# ------------------------------------------------------------------ the contract
@pytest.fixture(scope="module")
def pca_sweep(gpu_lib):
    return assert_cells_equal_simulate(W.CONTRACT_SWEEP, 3)


def test_contract_pca(pca_sweep):
    """Five cells, T = 3: every cell's metrics, summary, reputation, last rounds and last consensus
    outputs are its own simulate()'s (checked in the fixture); the carried reputation is the last smooth_rep."""
    assert W.same_bits(pca_sweep["outputs"]["smooth_rep"], pca_sweep["reputation"])
    assert 0.5 < pca_sweep["summary"][0, 0, 0] <= 1.0  # the default population mostly finds the truth


@pytest.mark.parametrize("algorithm", list(W.ALGORITHM_CASES))
def test_contract_other_algorithms(gpu_lib, algorithm):
    cells = W.CONTRACT_SWEEP + ([W.CAP_CELL] if algorithm == "big-five" else [])
    assert_cells_equal_simulate(cells, 2, algorithm, **W.ALGORITHM_CASES[algorithm])


def test_contract_clusterfeck_default_threshold(gpu_lib):
    """With no cluster_threshold the device's per-round rule applies: the sweep's last outputs are
    consensus_ragged(wide=True) on its own last rounds with the reputation it carried into them (the
    reputation a sweep of one timestep fewer returns)."""
    from pyconsensus_amd import consensus_ragged

    S = _sim()
    cells = W.CONTRACT_SWEEP
    first = S.sweep(cells, 1, algorithm="clusterfeck")
    both = S.sweep(cells, 2, algorithm="clusterfeck", keep_rounds=True, keep_outputs=True)
    _sync()
    carried, rounds = _host(first["reputation"]), {k: _host(v) for k, v in both["rounds"].items()}
    shapes = [(c["reporters"], c["events"]) for c in cells for _ in range(c["rounds"])]
    r0 = np.cumsum([0] + [n for n, _ in shapes])
    e0 = np.cumsum([0] + [e for _, e in shapes])
    c0 = np.cumsum([0] + [n * e for n, e in shapes])
    B = len(shapes)
    want = consensus_ragged([rounds["reports"][c0[b]:c0[b + 1]].reshape(shapes[b]) for b in range(B)],
                            [carried[r0[b]:r0[b + 1]] for b in range(B)],
                            [rounds["scaled"][e0[b]:e0[b + 1]] for b in range(B)],
                            [rounds["lo"][e0[b]:e0[b + 1]] for b in range(B)],
                            [rounds["hi"][e0[b]:e0[b + 1]] for b in range(B)], algorithm="clusterfeck", wide=True)
    _sync()
    for name, v in both["outputs"].items():
        assert W.same_bits(_host(v), _host(want[name])), name


# ------------------------------------------------------------------ host replay, independent of simulate()
def _replay_cell(host_rounds, c, rep, scaled_tol=0.1):
    from oracle import pcx_oracle_c as OC

    k, off = host_rounds["cells"][c], host_rounds["offsets"]
    R, N, E = k["rounds"], k["reporters"], k["events"]
    g = {name: W.cell_slice(host_rounds[name], off, W.OFFSET_OF[name], c) for name in W.ROUNDS}
    g = {name: v.reshape({"cells": (R, N, E), "events": (R, E), "reporters": (R, N)}[W.OFFSET_OF[name]])
         for name, v in g.items()}
    o = OC.batched(g["reports"], g["scaled"], g["lo"], g["hi"], rep, threads=8,
                   want=("old_rep", "smooth_rep", "outcomes_final"))
    m = W.np_metrics(g["scaled"], g["lo"], g["hi"], g["truth"], g["liar"], o["old_rep"], o["smooth_rep"],
                     o["outcomes_final"], scaled_tol)
    return g, o, m


def test_sweep_matches_host_replay(pca_sweep):
    """The PCA sweep's first two cells (the wave route and a workgroup round) replayed on the host:
    sweep_generate_host, the C oracle's batched consensus per cell with the carried reputation, numpy
    metrics and summaries."""
    S = _sim()
    cells, T, off = W.CONTRACT_SWEEP, 3, pca_sweep["offsets"]
    rep, last = [None, None], [None, None]
    for t in range(T):
        host = S.sweep_generate_host(cells, t)
        host["cells"] = cells
        for c in (0, 1):
            g, o, m = _replay_cell(host, c, rep[c])
            rep[c], last[c] = o["smooth_rep"], (g, o)
            assert W.same_bits(pca_sweep["metrics"][t, off["rounds"][c]:off["rounds"][c + 1]], m), (t, c)
            assert W.same_bits(pca_sweep["summary"][t, c], W.np_summary(m)), (t, c)
    for c in (0, 1):
        g, o = last[c]
        assert W.same_bits(W.cell_slice(pca_sweep["reputation"], off, "reporters", c), rep[c].reshape(-1)), c
        for name in W.ROUNDS:
            assert W.same_bits(W.cell_slice(pca_sweep["rounds"][name], off, W.OFFSET_OF[name], c),
                               g[name].reshape(-1)), (c, name)
        for name in ("old_rep", "smooth_rep", "outcomes_final"):
            assert W.same_bits(W.cell_slice(pca_sweep["outputs"][name], off, W.OFFSET_OF[name], c),
                               o[name].reshape(-1)), (c, name)


def test_sweep_takes_a_flat_starting_reputation(gpu_lib):
    from oracle import pcx_oracle_c as OC

    S = _sim()
    cells = [W.cell(5, 50, 20, 8), W.cell(3, 65, 33, 9)]
    host = S.sweep_generate_host(cells, 0)
    off = host["offsets"]
    rep0 = np.random.default_rng(1).integers(1, 100, int(off["reporters"][-1])).astype(np.float64)
    r = S.sweep(cells, 1, reputation=rep0, keep_outputs=True)
    _sync()
    for c, k in enumerate(cells):
        R, N, E = k["rounds"], k["reporters"], k["events"]
        o = OC.batched(W.cell_slice(host["reports"], off, "cells", c).reshape(R, N, E),
                       W.cell_slice(host["scaled"], off, "events", c).reshape(R, E),
                       W.cell_slice(host["lo"], off, "events", c).reshape(R, E),
                       W.cell_slice(host["hi"], off, "events", c).reshape(R, E),
                       W.cell_slice(rep0, off, "reporters", c).reshape(R, N), want=("old_rep", "smooth_rep"))
        assert W.same_bits(W.cell_slice(_host(r["outputs"]["old_rep"]), off, "reporters", c), o["old_rep"].reshape(-1))
        assert W.same_bits(W.cell_slice(_host(r["reputation"]), off, "reporters", c), o["smooth_rep"].reshape(-1))
    with pytest.raises(ValueError):
        S.sweep(cells, 1, reputation=rep0[:-1])


# ------------------------------------------------------------------ launch classes
def test_wave_route_and_every_launch_class_in_one_call(gpu_lib):
    """Under big-five 65 x 33 is launch class 3, 100 x 50 class 2 and 256 x 64 class 1: with the 50 x 20
    cell the one-wave launch, its scatter and three workgroup launches meet in every timestep."""
    cells = [W.cell(70, 50, 20, 31), W.cell(5, 100, 50, 32), W.cell(2, 256, 64, 33), W.cell(4, 65, 33, 34)]
    counts = _sim().sweep_plan(cells, algorithm="big-five", max_components=5)[1]
    assert counts.tolist() == [70, 2, 5, 4], counts
    assert_cells_equal_simulate(cells, 2, "big-five", max_components=5)


def test_wave_rounds_only_take_the_narrow_ragged_launch(gpu_lib):
    cells = [W.cell(70, 50, 20, 34), W.cell(9, 64, 32, 35, liar_frac=0.1), W.cell(7, 3, 2, 36), W.cell(300, 1, 1, 37)]
    counts = _sim().sweep_plan(cells)[1]
    assert counts[0] == sum(c["rounds"] for c in cells) and not counts[1:].any()
    assert_cells_equal_simulate(cells, 2)


# ------------------------------------------------------------------ asynchrony
def test_sweep_returns_before_the_stream_reaches_it(gpu_lib):
    """No host wait in the call: behind a long-running queue of matrix products on the stream, a T = 6
    sweep with workgroup rounds (descriptor tables, uploaded once) returns while an event recorded BEFORE
    it is still pending."""
    import torch

    S = _sim()
    cells = [W.cell(64, 50, 20, 1), W.cell(4, 100, 50, 2), W.cell(2, 256, 64, 3)]
    S.sweep(cells, 6)  # the work buffers, the staging slots and torch's allocator are warm
    x = torch.randn(4096, 4096, dtype=torch.float64, device="cuda")
    y = x @ x
    _sync()
    ev = torch.cuda.Event()
    for _ in range(40):  # (some hundred milliseconds of fp64 products)
        y = x @ x
    ev.record()
    r = S.sweep(cells, 6)
    returned_early = not ev.query()
    _sync()
    assert returned_early, "sweep() blocked the host until the work queued before it had run"
    warm = S.sweep(cells, 6)
    _sync()
    assert W.same_bits(_host(r["metrics"]), _host(warm["metrics"]))


# ------------------------------------------------------------------ determinism, buffers, simulate()
def test_determinism_and_one_cells_seed(gpu_lib):
    cells = [W.cell(40, 50, 20, 7), W.cell(6, 65, 33, 7), W.cell(30, 20, 10, 7)]
    a, b = run_sweep(cells, 2), run_sweep(cells, 2)
    other = [dict(c) for c in cells]
    other[1]["seed"] = 8
    c = run_sweep(other, 2)
    off = a["offsets"]
    for name in ("metrics", "summary", "reputation"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["rounds"]["reports"].tobytes() == b["rounds"]["reports"].tobytes()
    for k in (0, 1, 2):
        rows = slice(off["rounds"][k], off["rounds"][k + 1])
        same = W.same_bits(a["metrics"][:, rows], c["metrics"][:, rows]) and W.same_bits(
            W.cell_slice(a["rounds"]["reports"], off, "cells", k), W.cell_slice(c["rounds"]["reports"], off, "cells", k))
        assert same == (k != 1), k
        assert W.same_bits(a["summary"][:, k], c["summary"][:, k]) == (k != 1), k


def test_work_buffers_grow_are_shared_with_simulate_and_released(gpu_lib):
    import torch

    from pyconsensus_amd import _lib

    S = _sim()
    small = [W.cell(3, 5, 3, 1), W.cell(2, 65, 33, 2)]
    large = [W.cell(300, 50, 20, 3), W.cell(8, 100, 50, 4), W.cell(3, 5, 3, 5)]

    def run(cells):
        r = S.sweep(cells, 2)
        _sync()
        return _host(r["metrics"]).tobytes() + _host(r["reputation"]).tobytes() + _host(r["summary"]).tobytes()

    def run_simulate():
        r = S.simulate(257, 50, 20, 2, seed=42)
        _sync()
        return _host(r["metrics"]).tobytes() + _host(r["reputation"]).tobytes() + _host(r["summary"]).tobytes()

    sim_before = run_simulate()
    s1 = run(small)
    assert run_simulate() == sim_before          # simulate() unchanged by a sweep on the same context
    l1 = run(large)
    assert run_simulate() == sim_before
    _lib.check(gpu_lib.pcx_release_workspace(_lib.context(torch.cuda.current_device())))
    assert run(large) == l1 and run(small) == s1 and run_simulate() == sim_before


def test_refusals_and_the_empty_sweep(gpu_lib):
    S = _sim()
    for kw in (dict(algorithm="k-means"), dict(algorithm="cokurtosis"), dict(T=0)):
        with pytest.raises(Exception):
            S.sweep([W.cell(2, 5, 3, 1)], **kw)
    with pytest.raises(Exception) as e:
        S.sweep([W.cell(2, 5, 3, 1), W.cell(2, 300, 3, 1)])
    assert "cell 1:" in str(e.value)
    r = S.sweep([], 2)
    _sync()
    assert r["metrics"].shape == (2, 0, 6) and r["summary"].shape == (2, 0, 6) and r["reputation"].shape == (0,)
