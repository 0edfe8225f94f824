"""Tall cells in simulator studies on the GPU (sweep / study / simulate(..., tall=True),
pcx_simulate_study_tall_f64, pcx_simulate_tall_f64): a tall cell's slice against its equal-shape twin
byte for byte, the chain against the C SPEC built for 1024 reporters at T = 1 (its inputs drawn by the
host generator), per-cell algorithms with pairing, the generator's 1024-reporter instantiation against
its CPU twin, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sim_study_cases as S
import tall_cases as T
import tall_ragged_cases as G

pytestmark = pytest.mark.gpu

W = S.W
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_KIND = {"N": "reporters", "E": "events"}


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401  (the module: the package exports the function of that name)

    return sys.modules["pyconsensus_amd.simulate"]


def _host(x):
    return x.cpu().numpy()


def _host_all(r):
    import torch

    torch.cuda.synchronize()
    got = {k: _host(v) for k, v in r.items() if k in ("metrics", "summary", "reputation", "stats", "detail", "paired")}
    for k in ("rounds", "outputs"):
        if k in r:
            got[k] = {n: _host(v) for n, v in r[k].items() if n != "offsets"}
    got["offsets"] = r.get("offsets")
    return got


_RUNS = {}


def _study(T_):
    if T_ not in _RUNS:
        _RUNS[T_] = _host_all(_sim().study(G.STUDY_CELLS, T_, tall=True, pair_with=None, keep_detail=True,
                                           keep_outputs=True, keep_rounds=True))
    return _RUNS[T_]


def _twin(c, T_, **kw):
    k = G.STUDY_CELLS[c]
    return _host_all(_sim().simulate(k["rounds"], k["reporters"], k["events"], T_, seed=k["seed"], **W.rates(k),
                                     keep_outputs=True, keep_rounds=True, **kw))


def _cell_outputs(r, c):
    """{name: the cell's slice} of a study's kept outputs, shaped as the equal-shape call's."""
    from pyconsensus_amd import _abi

    k, off = G.STUDY_CELLS[c], r["offsets"]
    R, N, E = k["rounds"], k["reporters"], k["events"]
    out = {}
    for name, kind, _ in _abi.BATCH_OUTPUTS:
        if name not in r["outputs"]:
            continue
        v = r["outputs"][name]
        if kind in OUT_KIND:
            out[name] = W.cell_slice(v, off, OUT_KIND[kind], c).reshape(R, N if kind == "N" else E)
        else:
            out[name] = W.cell_slice(v, off, "rounds", c)
    return out


@pytest.mark.parametrize("c", [0, 1, 2], ids=["257x5", "513x33", "1024x64"])
def test_tall_cell_is_its_equal_shape_twin(gpu_lib, c):
    M = _sim()
    r, off = _study(G.STUDY_T), _study(G.STUDY_T)["offsets"]
    k = G.STUDY_CELLS[c]
    R, N, E = k["rounds"], k["reporters"], k["events"]
    rows = slice(int(off["rounds"][c]), int(off["rounds"][c + 1]))
    twin, twin0 = _twin(c, G.STUDY_T, tall=True), _twin(c, 1, tall=True)
    assert S.same_bits(r["metrics"][:, rows], twin["metrics"])
    assert S.same_bits(r["summary"][:, c], twin["summary"])
    assert S.same_bits(W.cell_slice(r["reputation"], off, "reporters", c).reshape(R, N), twin["reputation"])
    mine = _cell_outputs(r, c)
    assert set(mine) == set(twin["outputs"])
    for name, v in mine.items():
        assert S.same_bits(v, twin["outputs"][name]), name
    # detail: the equal-shape host entry on the twin's rounds and outputs, timestep by timestep
    for t, tw in ((0, twin0), (G.STUDY_T - 1, twin)):
        o = tw["outputs"]
        want = M.detail_host({n: tw["rounds"][n] for n in ("scaled", "lo", "hi", "truth", "liar")}, o["old_rep"],
                             o["smooth_rep"], o["outcomes_final"])
        assert S.same_bits(r["detail"][t, rows], want), t
    # stats: the stand-alone host entry's arithmetic over the twin's metrics and that detail (it reads
    # the cells' round counts alone: a 1 x 1 stand-in cell of R rounds)
    st = M.sweep_stats_host([G.cell(R, 1, 1, 0)], twin["metrics"], r["detail"][:, rows])
    assert S.same_bits(r["stats"][:, c], st["stats"][:, 0])


def test_small_cells_are_the_existing_studys(gpu_lib):
    small = [3, 4]
    r, off = _study(G.STUDY_T), _study(G.STUDY_T)["offsets"]
    e = _host_all(_sim().study([G.STUDY_CELLS[c] for c in small], G.STUDY_T, keep_detail=True, keep_outputs=True))
    for k, c in enumerate(small):
        rows = slice(int(off["rounds"][c]), int(off["rounds"][c + 1]))
        erows = slice(int(e["offsets"]["rounds"][k]), int(e["offsets"]["rounds"][k + 1]))
        for name in ("metrics", "detail"):
            assert S.same_bits(r[name][:, rows], e[name][:, erows]), (c, name)
        for name in ("summary", "stats"):
            assert S.same_bits(r[name][:, c], e[name][:, k]), (c, name)
        assert S.same_bits(W.cell_slice(r["reputation"], off, "reporters", c),
                           W.cell_slice(e["reputation"], e["offsets"], "reporters", k))
        from pyconsensus_amd import _abi

        for name, kind, _ in _abi.BATCH_OUTPUTS:
            if name in r["outputs"]:
                key = OUT_KIND.get(kind, "rounds")
                assert S.same_bits(W.cell_slice(r["outputs"][name], off, key, c),
                                   W.cell_slice(e["outputs"][name], e["offsets"], key, k)), (c, name)


@pytest.mark.parametrize("c", [0, 1, 2], ids=["257x5", "513x33", "1024x64"])
def test_tall_cell_against_the_spec_at_one_timestep(gpu_lib, c):
    """T = 1: the kept consensus outputs of a tall cell against the SPEC on the host generator's rounds."""
    M = _sim()
    k = G.STUDY_CELLS[c]
    g = M.generate_host(k["rounds"], k["reporters"], k["events"], t=0, seed=k["seed"], **W.rates(k))
    want = T.spec(g["reports"], g["scaled"], g["lo"], g["hi"], None)
    mine = _cell_outputs(_study(1), c)
    assert set(G.EVERY) <= set(mine) <= set(want)
    for name, v in mine.items():
        same = T.bits_equal(v, want[name])
        assert np.all(same), (name, int(np.size(same) - np.count_nonzero(same)))


def test_per_cell_algorithms_with_pairing(gpu_lib):
    """A 512 x 20 cell under PCA and under "absolute", paired: the paired differences recomputed on the
    host from the study's own metrics and detail, in the stand-alone statistics entry's arithmetic."""
    M = _sim()
    r = _host_all(M.study(G.PAIR_CELLS, 2, tall=True, pair_with="first", keep_detail=True))
    R = G.PAIR_CELLS[0]["rounds"]
    st = M.sweep_stats_host([G.cell(R, 1, 1, 0)] * 2, r["metrics"], r["detail"], pair_with=[-1, 0])
    assert S.same_bits(r["stats"], st["stats"]) and S.same_bits(r["paired"], st["paired"])
    values = np.concatenate([r["metrics"], r["detail"]], axis=2)
    ok = ~np.isnan(values[:, R:]) & ~np.isnan(values[:, :R])
    assert np.array_equal(r["paired"][:, 1, :, 0], ok.sum(axis=1))  # n: the rounds where both values exist
    assert (r["paired"][:, 1, :, 0] > 0).any() and (r["stats"][:, 0, :, 1] != r["stats"][:, 1, :, 1]).any()
    for c, alg in enumerate(("PCA", "absolute")):  # each cell is its own equal-shape run
        k = G.PAIR_CELLS[c]
        tw = _host_all(M.simulate(k["rounds"], k["reporters"], k["events"], 2, seed=k["seed"], **W.rates(k),
                                  algorithm=alg, tall=True))
        assert S.same_bits(r["metrics"][:, c * R:(c + 1) * R], tw["metrics"]), alg


def test_generator_1024_against_its_cpu_twin(gpu_lib):
    M = _sim()
    k = G.TWIN_CELL
    r = _host_all(M.sweep([G.cell(2, 7, 5, 3), k], 1, tall=True, keep_rounds=True))
    g = M.generate_host(k["rounds"], k["reporters"], k["events"], t=0, seed=k["seed"], **W.rates(k))
    assert g["liar"].any() and np.isnan(g["reports"]).any() and g["scaled"].any()
    for name in W.ROUNDS:
        assert S.same_bits(W.cell_slice(r["rounds"][name], r["offsets"], W.OFFSET_OF[name], 1), g[name].reshape(-1)), name


def test_command_line_tall(gpu_lib):
    argv = [sys.executable, "-m", "pyconsensus_amd.simulate", "--tall", "--rounds", "3", "--reporters", "50,300",
            "--events", "6", "--seed", "9"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout)
    assert [c["reporters"] for c in got["cells"]] == [50, 300]
    M = _sim()
    cells = M.grid(3, seed=9, reporters=[50, 300], events=[6], liar_frac=[0.3], collude_frac=[0.5], distort=[0.1],
                   na_frac=[0.1], scaled_frac=[0.25])
    want = _host(M.sweep(cells, 1, tall=True)["summary"])
    for c, printed in enumerate(got["cells"]):
        assert [printed["summary"][0][k] for k in M.METRICS] == [float(v) for v in want[0, c]], c
    p = subprocess.run(argv[:3] + argv[4:], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "[1, 256] x [1, 64]" in p.stderr  # without --tall: the old refusal
