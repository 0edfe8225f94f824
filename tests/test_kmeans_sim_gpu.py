"""k-means in the simulator on the GPU: the code books drawn on the device equal
their host twin byte for byte, a trajectory under k-means equals the host-driven loop over the same
books, a sweep's cells equal their own simulate(), and a study pairs a PCA cell with a k-means cell on
the same drawn rounds.  Every comparison is on bits, NaN equal to NaN."""
import sys

import numpy as np
import pytest

import kmeans_cases as K
import sim_sweep_cases as W

pytestmark = pytest.mark.gpu


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401

    return sys.modules["pyconsensus_amd.simulate"]


def _sync():
    import torch

    torch.cuda.synchronize()


def _host(x):
    return x.cpu().numpy()


SWEEP = [K.cell(3, 10, 4, 5), K.cell(2, 100, 50, 7, liar_frac=0.2), K.cell(70, 1, 1, 5), K.cell(2, 256, 64, 9),
         K.cell(5, 17, 5, 11, na_frac=0.2)]


def test_device_books_equal_the_host_books(gpu_lib):
    S = _sim()
    for (N, E), B, t, restarts in (((50, 20), 300, 0, 20), ((64, 32), 33, 2, 3), ((100, 50), 5, 1, 1), ((1, 1), 4, 0, 2)):
        got = S.kmeans_books(B, N, t=t, seed=31 + N, restarts=restarts)
        _sync()
        want = S.kmeans_books_host(B, N, t=t, seed=31 + N, restarts=restarts)
        assert tuple(got.shape) == want.shape == (B, restarts, K.rule(N)) and (_host(got) == want).all(), (N, E)
    for t in (0, 3):
        got, off = S.sweep_kmeans_books(SWEEP, t=t, restarts=3)
        _sync()
        want, off_h = S.sweep_kmeans_books_host(SWEEP, t=t, restarts=3)
        assert (off == off_h).all() and got.numel() == off[-1] == want.size and (_host(got) == want).all()


def host_loop(B, N, E, T, seed, restarts, **rates):
    """The trajectory driven from the host: generate, consensus_batched on the host twin's books,
    metrics, smooth_rep carried."""
    from pyconsensus_amd.batched import consensus_batched

    S = _sim()
    rep, ms, ss = None, [], []
    for t in range(T):
        g = S.generate(B, N, E, t=t, seed=seed, **rates)
        o = consensus_batched(g["reports"], rep, g["scaled"], g["lo"], g["hi"], algorithm="k-means",
                              kmeans_init=S.kmeans_books_host(B, N, t=t, seed=seed, restarts=restarts))
        m = S.metrics(g, o["old_rep"], o["smooth_rep"], o["outcomes_final"])
        _sync()
        ms.append(_host(m["metrics"]))
        ss.append(_host(m["summary"]))
        rep = o["smooth_rep"]
    return {"metrics": np.stack(ms), "summary": np.stack(ss), "reputation": _host(rep),
            "outputs": {k: _host(v) for k, v in o.items() if not k.startswith("_")},
            "rounds": {k: _host(v) for k, v in g.items()}}


_SIMULATE = {}


def simulate(B, N, E, T, seed, restarts, **rates):
    key = (B, N, E, T, seed, restarts, tuple(sorted(rates.items())))
    if key not in _SIMULATE:
        r = _sim().simulate(B, N, E, T, seed=seed, algorithm="k-means", kmeans_restarts=restarts, keep_rounds=True,
                            keep_outputs=True, **rates)
        _sync()
        _SIMULATE[key] = {"metrics": _host(r["metrics"]), "summary": _host(r["summary"]),
                          "reputation": _host(r["reputation"]),
                          "outputs": {k: _host(v) for k, v in r["outputs"].items()},
                          "rounds": {k: _host(v) for k, v in r["rounds"].items()}}
    return _SIMULATE[key]


@pytest.mark.parametrize("B, N, E", [(33, 50, 20), (5, 100, 50)])
def test_simulate_under_kmeans_equals_the_host_driven_loop(gpu_lib, B, N, E):
    got = simulate(B, N, E, 3, 20261020, 3)
    want = host_loop(B, N, E, 3, 20261020, 3)
    for name in ("metrics", "summary", "reputation"):
        assert K.same_bits(got[name], want[name]), name
    assert set(got["outputs"]) == set(want["outputs"]) and len(got["outputs"]) == 23
    for name, v in want["outputs"].items():
        assert K.same_bits(got["outputs"][name], v), name
    for name, v in want["rounds"].items():
        assert K.same_bits(got["rounds"][name], v), name
    assert not K.same_bits(got["metrics"][0], got["metrics"][2])


def _cell_slices(r, offsets, c):
    kind_of = {"N": "reporters", "E": "events", "1": "rounds", "NE": "cells"}
    from pyconsensus_amd import _abi

    kinds = {name: kind_of[kind] for name, kind, _ in _abi.BATCH_OUTPUTS}
    out = {"metrics": r["metrics"][:, int(offsets["rounds"][c]):int(offsets["rounds"][c + 1])],
           "summary": r["summary"][:, c], "reputation": W.cell_slice(r["reputation"], offsets, "reporters", c)}
    out["outputs"] = {k: W.cell_slice(v, offsets, kinds[k], c) for k, v in r["outputs"].items()}
    out["rounds"] = {k: W.cell_slice(v, offsets, W.OFFSET_OF[k], c) for k, v in r["rounds"].items()}
    return out


def assert_cell_is_its_simulate(got, cell, T, restarts, what):
    want = simulate(cell["rounds"], cell["reporters"], cell["events"], T, cell["seed"], restarts, **W.rates(cell))
    for name in ("metrics", "summary", "reputation"):
        assert K.same_bits(got[name], want[name].reshape(got[name].shape)), (what, name)
    for group in ("outputs", "rounds"):
        assert set(got[group]) == set(want[group])
        for name, v in want[group].items():
            assert K.same_bits(got[group][name], v.reshape(-1)), (what, group, name)


def test_a_sweeps_cells_equal_their_own_simulate(gpu_lib):
    S = _sim()
    r = S.sweep(SWEEP, 2, algorithm="k-means", kmeans_restarts=3, keep_rounds=True, keep_outputs=True)
    _sync()
    host = {"metrics": _host(r["metrics"]), "summary": _host(r["summary"]), "reputation": _host(r["reputation"]),
            "outputs": {k: _host(v) for k, v in r["outputs"].items()},
            "rounds": {k: _host(v) for k, v in r["rounds"].items() if k != "offsets"}}
    for c, cell in enumerate(SWEEP):
        assert_cell_is_its_simulate(_cell_slices(host, r["offsets"], c), cell, 2, 3, c)


def test_a_study_pairs_pca_and_kmeans_on_the_same_rounds(gpu_lib):
    S = _sim()
    bases = [K.cell(40, 17, 5, 3, liar_frac=0.4), K.cell(6, 100, 50, 4)]
    cells = [dict(b, algorithm=alg) for b in bases for alg in ("PCA", "k-means")]
    r = S.study(cells, 2, pair_with="first", keep_detail=True, keep_rounds=True, keep_outputs=True, kmeans_restarts=3)
    _sync()
    assert r["pair_base"].tolist() == [-1, 0, -1, 2]
    metrics, detail, off = _host(r["metrics"]), _host(r["detail"]), r["offsets"]
    bare = [{k: v for k, v in c.items() if k != "algorithm"} for c in cells]
    want = S.sweep_stats_host(bare, metrics, detail, pair_with=[-1, 0, -1, 2])
    assert K.same_bits(_host(r["stats"]), want["stats"]) and K.same_bits(_host(r["paired"]), want["paired"])
    host = {"metrics": metrics, "summary": _host(r["summary"]), "reputation": _host(r["reputation"]),
            "outputs": {k: _host(v) for k, v in r["outputs"].items()},
            "rounds": {k: _host(v) for k, v in r["rounds"].items() if k != "offsets"}}
    for c in (0, 2):  # the two cells of a pair see the same drawn rounds
        a, b = _cell_slices(host, off, c), _cell_slices(host, off, c + 1)
        for name in W.ROUNDS:
            assert K.same_bits(a["rounds"][name], b["rounds"][name]), (c, name)
        assert not K.same_bits(a["outputs"]["smooth_rep"], b["outputs"]["smooth_rep"])
        assert_cell_is_its_simulate(b, bare[c + 1], 2, 3, c + 1)  # the k-means cell is its own simulate()
    plain = S.study([bare[0]], 2, keep_rounds=True, keep_outputs=True)  # and the PCA cell the parent's study
    _sync()
    assert K.same_bits(_host(plain["metrics"]), _cell_slices(host, off, 0)["metrics"])


def test_without_the_keyword_kmeans_is_still_refused(gpu_lib):
    from pyconsensus_amd._lib import PcxError
    from pyconsensus_amd.batched import consensus_ragged

    S = _sim()
    mats = [np.ones((5, 3)) + (np.arange(15).reshape(5, 3) % 2), np.ones((4, 3)) + (np.arange(12).reshape(4, 3) % 2)]
    with pytest.raises(PcxError, match="k-means is not supported"):
        consensus_ragged(mats, algorithm="k-means")
    with pytest.raises(PcxError, match="parameter set 1: k-means"):
        consensus_ragged(mats, per_round=[{}, {"algorithm": "k-means"}], wide=True)
    with pytest.raises(PcxError, match="k-means is not simulated"):
        S.simulate(4, 5, 3, algorithm="k-means")
    with pytest.raises(PcxError, match="k-means is not simulated"):
        S.sweep([K.cell(2, 5, 3, 1)], algorithm="k-means")
    with pytest.raises(PcxError, match="cell 0: k-means is not simulated"):
        S.sweep_plan([dict(K.cell(2, 5, 3, 1), algorithm="k-means")])
    with pytest.raises(PcxError, match="cell 0: k-means is not simulated"):
        S.study([dict(K.cell(2, 5, 3, 1), algorithm="k-means")])
    with pytest.raises(PcxError, match="cokurtosis is not simulated"):
        S.sweep([K.cell(2, 5, 3, 1)], algorithm="cokurtosis", kmeans_restarts=3)
    with pytest.raises(PcxError, match="restarts must be >= 1"):
        S.simulate(4, 5, 3, algorithm="k-means", kmeans_restarts=0)
    # another algorithm under the keyword: the same bytes as without it
    a = S.simulate(8, 10, 4, 2, seed=3, kmeans_restarts=5)
    b = S.simulate(8, 10, 4, 2, seed=3)
    _sync()
    assert K.same_bits(_host(a["metrics"]), _host(b["metrics"])) and K.same_bits(_host(a["reputation"]), _host(b["reputation"]))
