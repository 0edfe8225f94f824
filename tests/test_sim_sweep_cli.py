"""``python -m pyconsensus_amd.simulate`` with comma lists: single values print what they always printed,
a list on any shape or rate runs ``sweep(grid(...))`` and prints one JSON object with a ``cells`` list."""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401  (the module: the package exports the function of that name)

    return sys.modules["pyconsensus_amd.simulate"]


def _run(capsys, argv):
    assert _sim().main(argv) == 0
    out = capsys.readouterr().out
    assert out.count("\n") == 1  # one line, one object
    return out


def test_single_values_print_the_equal_shape_summary(gpu_lib, capsys):
    S = _sim()
    out = _run(capsys, ["--rounds", "257", "--reporters", "30", "--events", "12", "--timesteps", "2", "--seed", "5",
                        "--liars", "0.2", "--missing", "0.05"])
    summary = S.simulate(257, 30, 12, 2, seed=5, liar_frac=0.2, na_frac=0.05)["summary"].cpu().numpy()
    want = json.dumps({"rounds": 257, "reporters": 30, "events": 12, "seed": 5, "algorithm": "PCA",
                       "summary": [dict(zip(S.METRICS, (float(v) for v in row)), timestep=t)
                                   for t, row in enumerate(summary)]}) + "\n"
    assert out == want  # byte for byte: the keys, their order and the values
    assert list(json.loads(out)) == ["rounds", "reporters", "events", "seed", "algorithm", "summary"]
    # the defaults are what they were
    got = json.loads(_run(capsys, ["--rounds", "64"]))
    assert (got["reporters"], got["events"], got["seed"], got["algorithm"]) == (50, 20, 0, "PCA")
    want = S.simulate(64)["summary"].cpu().numpy()
    assert [got["summary"][0][k] for k in S.METRICS] == [float(v) for v in want[0]]


def test_lists_run_the_grid(gpu_lib, capsys):
    S = _sim()
    got = json.loads(_run(capsys, ["--rounds", "100", "--timesteps", "2", "--seed", "3", "--liars", "0.1,0.3",
                                   "--reporters", "20,50"]))
    cells = S.grid(100, seed=3, reporters=[20, 50], events=[20], liar_frac=[0.1, 0.3], collude_frac=[0.5],
                   distort=[0.1], na_frac=[0.1], scaled_frac=[0.25])
    want = S.sweep(cells, 2)["summary"].cpu().numpy()
    assert (got["rounds"], got["seed"], got["algorithm"]) == (100, 3, "PCA") and len(got["cells"]) == 4
    assert sorted((c["reporters"], c["liar_frac"]) for c in got["cells"]) == [(20, 0.1), (20, 0.3), (50, 0.1), (50, 0.3)]
    for c, (cell, printed) in enumerate(zip(cells, got["cells"])):
        for k in ("reporters", "events", "liar_frac", "collude_frac", "distort", "na_frac", "scaled_frac"):
            assert printed[k] == cell[k], (c, k)
        assert [s["timestep"] for s in printed["summary"]] == [0, 1]
        for t in range(2):
            assert [printed["summary"][t][k] for k in S.METRICS] == [float(v) for v in want[t, c]], (c, t)
    # every cell of the grid is its own equal-shape run
    one = S.simulate(100, 50, 20, 2, seed=3, liar_frac=0.3)["summary"].cpu().numpy()
    assert np.array_equal(want[:, 3], one)
