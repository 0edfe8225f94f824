"""Simulator studies on the GPU: a sweep that also writes detail metrics every timestep
and reduces every per-round value to per-cell statistics and paired differences on the device.

The kernels are the inline code of the host entries, so everything is compared bit for bit (all NaNs
alike): the device against the host on hand-made inputs and on a study's real rounds, a study against
the sweep it extends, and a study's statistics against the stand-alone entries on its own outputs.
"""
import ctypes as C
import json
import sys

import numpy as np
import pytest

import sim_study_cases as S

pytestmark = pytest.mark.gpu

W = S.W


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401  (the module: the package exports the function of that name)

    return sys.modules["pyconsensus_amd.simulate"]


def _sync():
    import torch

    torch.cuda.synchronize()


def _host(x):
    return x.cpu().numpy()


# 1 x 1, an odd small shape, the one-wave limit and just past it (the workgroup route); liar_frac 0 and 1,
# scaled_frac 0 and 1, and na_frac 1: no report at all, every scaled outcome NaN
STUDY_CELLS = [S.cell(40, 1, 1, 1), S.cell(7, 5, 3, 2, liar_frac=0.0), S.cell(9, 5, 3, 3, liar_frac=1.0),
               S.cell(5, 64, 32, 4, scaled_frac=0.0), S.cell(3, 65, 33, 5, scaled_frac=1.0),
               S.cell(6, 5, 3, 6, na_frac=1.0), S.cell(4, 65, 33, 7)]

_RUNS = {}


def run_study(cells, T, pair_with=None, algorithm="PCA", **kw):
    """A study with everything kept, on the host (computed once per argument set, left unchanged)."""
    key = (json.dumps(cells, sort_keys=True), T, json.dumps(pair_with), algorithm, json.dumps(kw, sort_keys=True))
    if key not in _RUNS:
        r = _sim().study(cells, T, pair_with=pair_with, keep_detail=True, keep_rounds=True, keep_outputs=True,
                         algorithm=algorithm, **kw)
        _sync()
        got = {k: _host(r[k]) for k in ("metrics", "summary", "reputation", "stats", "detail")}
        got["paired"] = _host(r["paired"]) if "paired" in r else None
        got["rounds"] = {k: _host(v) for k, v in r["rounds"].items()}
        got["outputs"] = {k: _host(v) for k, v in r["outputs"].items()}
        got["offsets"] = r["offsets"]
        _RUNS[key] = got
    return _RUNS[key]


def _last_inputs(r):
    return r["rounds"], r["outputs"]["old_rep"], r["outputs"]["smooth_rep"], r["outputs"]["outcomes_final"]


# ------------------------------------------------------------------ detail metrics: device against host
def test_detail_on_hand_made_rounds(gpu_lib):
    M = _sim()
    flat, _ = S.hand_rounds()
    args = (S.HAND_CELLS, S.rounds_of(flat), flat["old"], flat["smooth"], flat["outcomes"])
    dev = M.sweep_detail(*args, scaled_tol=S.TOL)
    assert S.same_bits(_host(dev), M.sweep_detail_host(*args, scaled_tol=S.TOL))


def test_detail_on_a_studys_rounds(gpu_lib):
    """T = 2: the last timestep's real rounds and outputs; the study's own detail[1] is the same bytes."""
    M = _sim()
    r = run_study(STUDY_CELLS, 2)
    rounds, old, smooth, outc = _last_inputs(r)
    off = r["offsets"]
    # na_frac = 1, no report at all: the scaled outcomes are NaN, the binary ones mostly indeterminate
    blank, blank_scaled = (W.cell_slice(x, off, "events", 5) for x in (outc, rounds["scaled"]))
    assert np.isnan(blank[blank_scaled != 0]).all() and (blank_scaled != 0).any() and (blank == 1.5).any()
    host = M.sweep_detail_host(STUDY_CELLS, rounds, old, smooth, outc)
    dev = _host(M.sweep_detail(STUDY_CELLS, rounds, old, smooth, outc))
    assert S.same_bits(dev, host)
    assert S.same_bits(r["detail"][1], host)
    rows = slice(off["rounds"][5], off["rounds"][6])
    assert (host[rows, 4] > 0).any() and np.isnan(host[rows, 5]).all() and (host[rows, 2] > 0).any()
    assert (host[off["rounds"][1]:off["rounds"][2], 6:8] == 0).all()   # liar_frac 0: no liar
    assert (host[off["rounds"][2]:off["rounds"][3], 8:10] == 0).all()  # liar_frac 1: nobody honest
    assert np.isnan(host[off["rounds"][3]:off["rounds"][4], 1]).all()  # scaled_frac 0
    assert np.isnan(host[off["rounds"][4]:off["rounds"][5], 0]).all()  # scaled_frac 1


@pytest.mark.parametrize("c", [2, 6], ids=["5x3", "65x33"])
def test_equal_shape_detail_is_the_cells_slice(gpu_lib, c):
    M = _sim()
    r = run_study(STUDY_CELLS, 2)
    k, off = STUDY_CELLS[c], r["offsets"]
    R, N, E = k["rounds"], k["reporters"], k["events"]
    rounds, old, smooth, outc = _last_inputs(r)
    mine = {name: W.cell_slice(rounds[name], off, W.OFFSET_OF[name], c).reshape(
        (R, N) if name == "liar" else (R, E)) for name in ("scaled", "lo", "hi", "truth", "liar")}
    old, smooth = (W.cell_slice(x, off, "reporters", c).reshape(R, N) for x in (old, smooth))
    outc = W.cell_slice(outc, off, "events", c).reshape(R, E)
    want = r["detail"][1, off["rounds"][c]:off["rounds"][c + 1]]
    assert S.same_bits(_host(M.detail(mine, old, smooth, outc)), want)
    assert S.same_bits(M.detail_host(mine, old, smooth, outc), want)


# ------------------------------------------------------------------ statistics: device against host
def test_stats_on_the_hand_made_values(gpu_lib):
    M = _sim()
    metrics, detail = S.stats_values()
    host = M.sweep_stats_host(S.STATS_CELLS, metrics, detail, pair_with=list(S.STATS_BASE))
    dev = M.sweep_stats(S.STATS_CELLS, metrics, detail, pair_with=list(S.STATS_BASE))
    assert S.same_bits(_host(dev["stats"]), host["stats"]) and S.same_bits(_host(dev["paired"]), host["paired"])
    alone = M.sweep_stats(S.STATS_CELLS, metrics, detail)  # paired and pair_base NULL together
    assert "paired" not in alone and S.same_bits(_host(alone["stats"]), host["stats"])


PAIR_CELLS = [S.cell(1, 5, 3, 11), S.cell(257, 5, 3, 12), S.cell(257, 5, 3, 12, liar_frac=0.4),
              S.cell(1, 5, 3, 11, na_frac=0.3), S.cell(257, 6, 3, 12)]
PAIR_BASE = [-1, -1, 1, 0, 1]


def test_stats_of_a_studys_own_outputs(gpu_lib):
    """R in {1, 257}: the study's stats / paired are sweep_stats on the call's own metrics and detail,
    device and host, and `mean` of the metrics is the sweep's summary."""
    M = _sim()
    r = run_study(PAIR_CELLS, 2, pair_with=PAIR_BASE)
    host = M.sweep_stats_host(PAIR_CELLS, r["metrics"], r["detail"], pair_with=PAIR_BASE)
    dev = M.sweep_stats(PAIR_CELLS, r["metrics"], r["detail"], pair_with=PAIR_BASE)
    for name in ("stats", "paired"):
        assert S.same_bits(r[name], host[name]), name
        assert S.same_bits(_host(dev[name]), host[name]), name
    assert not np.isnan(r["metrics"]).any() and S.same_bits(r["stats"][:, :, :6, 1], r["summary"])
    assert (r["paired"][:, 2, :6, 0] == 257).all() and (r["paired"][:, :2, :, 0] == 0).all()
    assert (r["paired"][:, 2, 5, 1] > 0).all()  # liar_frac 0.4 against 0.3 on one seed: never fewer liars


# ------------------------------------------------------------------ a study is its sweep
@pytest.mark.parametrize("algorithm,kw", [("PCA", {}), ("hierarchical", {}), ("big-five", {"max_components": 5})],
                         ids=["PCA", "hierarchical", "big-five"])
def test_study_writes_the_sweeps_bytes(gpu_lib, algorithm, kw):
    got = run_study(STUDY_CELLS, 2, algorithm=algorithm, **kw)
    r = _sim().sweep(STUDY_CELLS, 2, algorithm=algorithm, keep_rounds=True, keep_outputs=True, **kw)
    _sync()
    for name in ("metrics", "summary", "reputation"):
        assert S.same_bits(got[name], _host(r[name])), name
    for name, v in r["rounds"].items():
        assert S.same_bits(got["rounds"][name], _host(v)), name
    for name, v in r["outputs"].items():
        assert S.same_bits(got["outputs"][name], _host(v)), name


def test_every_timesteps_detail(gpu_lib):
    """T = 3: detail[t] is sweep_detail on the last timestep of a study of t + 1 timesteps."""
    M = _sim()
    whole = run_study(STUDY_CELLS, 3)
    for t in range(3):
        part = run_study(STUDY_CELLS, t + 1)
        rounds, old, smooth, outc = _last_inputs(part)
        assert S.same_bits(whole["detail"][t], _host(M.sweep_detail(STUDY_CELLS, rounds, old, smooth, outc))), t
        assert S.same_bits(whole["metrics"][t], part["metrics"][t]), t


def test_detail_and_metrics_may_stay_in_the_workspace(gpu_lib):
    """Without keep_detail the statistics are the same bytes."""
    r = _sim().study(PAIR_CELLS, 2, pair_with=PAIR_BASE)
    _sync()
    want = run_study(PAIR_CELLS, 2, pair_with=PAIR_BASE)
    assert "detail" not in r
    assert S.same_bits(_host(r["stats"]), want["stats"]) and S.same_bits(_host(r["paired"]), want["paired"])


# ------------------------------------------------------------------ common random numbers
def test_common_random_numbers_show_in_paired(gpu_lib):
    """Two 5 x 3 cells with one seed and the same rates: every paired difference is exactly 0 -- mean 0,
    var 0 -- over all the rounds in which the value exists (n = R for the six metrics, which are never
    NaN here; a ratio without a denominator is NaN in both cells alike, so n is the cell's own count).
    With another seed the differences are not 0."""
    R = 40
    r = run_study([S.cell(R, 5, 3, 21), S.cell(R, 5, 3, 21), S.cell(R, 5, 3, 22)], 2, pair_with=[-1, 0, 0])
    n, mean, var = (r["paired"][:, 1, :, k] for k in range(3))
    assert (n[:, :6] == R).all() and (n == r["stats"][:, 1, :, 0]).all() and (n[:, 12:16] == R).all()
    assert (mean[n >= 1] == 0.0).all() and (var[n >= 2] == 0.0).all() and (n >= 2).sum() >= 2 * 16
    other_mean, other_var = r["paired"][:, 2, :, 1], r["paired"][:, 2, :, 2]
    assert (other_mean[:, :6] != 0.0).any() and (other_var[:, :6] > 0.0).any()


# ------------------------------------------------------------------ asynchrony
def test_study_returns_before_the_stream_reaches_it(gpu_lib):
    """No host wait in the call: behind a long-running queue of matrix products on the stream, a T = 6 study
    with workgroup rounds returns while an event recorded BEFORE it is still pending."""
    import torch

    M = _sim()
    cells = [S.cell(64, 50, 20, 1), S.cell(4, 100, 50, 2), S.cell(64, 50, 20, 1, liar_frac=0.2)]
    M.study(cells, 6, pair_with="first")  # the work buffers, the staging slots and torch's allocator are warm
    x = torch.randn(4096, 4096, dtype=torch.float64, device="cuda")
    y = x @ x
    _sync()
    ev = torch.cuda.Event()
    for _ in range(40):  # (some hundred milliseconds of fp64 products)
        y = x @ x
    ev.record()
    r = M.study(cells, 6, pair_with="first")
    returned_early = not ev.query()
    _sync()
    assert returned_early, "study() blocked the host until the work queued before it had run"
    warm = M.study(cells, 6, pair_with="first")
    _sync()
    assert W.same_bits(_host(r["stats"]), _host(warm["stats"])) and W.same_bits(_host(r["paired"]), _host(warm["paired"]))


# ------------------------------------------------------------------ command line
def _run(capsys, argv):
    assert _sim().main(argv) == 0
    out = capsys.readouterr().out
    assert out.count("\n") == 1  # one line, one object
    return out


def _same_number(a, b):
    return a == b or (a != a and b != b)


def test_cli_stats_and_paired(gpu_lib, capsys):
    M = _sim()
    argv = ["--rounds", "100", "--timesteps", "2", "--seed", "3", "--liars", "0.1,0.3", "--reporters", "20,50"]
    cells = M.grid(100, seed=3, reporters=[20, 50], events=[20], liar_frac=[0.1, 0.3], collude_frac=[0.5],
                   distort=[0.1], na_frac=[0.1], scaled_frac=[0.25])
    want = M.study(cells, 2, pair_with="first")
    summary, stats, paired = (_host(want[k]) for k in ("summary", "stats", "paired"))
    se, pse = M.stderr(stats), M.stderr(paired)
    assert want["pair_base"].tolist() == [-1, 0, -1, 2]
    for flags in (["--stats"], ["--paired"], ["--stats", "--paired"]):
        got = json.loads(_run(capsys, argv + flags))
        assert (got["rounds"], got["seed"], got["algorithm"]) == (100, 3, "PCA") and len(got["cells"]) == 4
        for c, printed in enumerate(got["cells"]):
            assert printed["reporters"] == cells[c]["reporters"] and printed["liar_frac"] == cells[c]["liar_frac"]
            for t, d in enumerate(printed["summary"]):
                assert d["timestep"] == t
                assert [d[k] for k in M.METRICS] == [float(v) for v in summary[t, c]]
                assert list(d["detail"]) == list(M.DETAIL) and list(d["stderr"]) == list(M.VALUES)
                assert all(_same_number(d["detail"][k], float(stats[t, c, 6 + i, 1])) for i, k in enumerate(M.DETAIL))
                assert all(_same_number(d["stderr"][k], float(se[t, c, i])) for i, k in enumerate(M.VALUES))
                if "--paired" in flags and c in (1, 3):
                    assert list(d["vs_first"]) == list(M.VALUES)
                    for i, k in enumerate(M.VALUES):
                        assert _same_number(d["vs_first"][k][0], float(paired[t, c, i, 1])), (c, t, k)
                        assert _same_number(d["vs_first"][k][1], float(pse[t, c, i])), (c, t, k)
                else:
                    assert "vs_first" not in d
    # without the flags: exactly the sweep's object
    plain = M.sweep(cells, 2)["summary"].cpu().numpy()
    expect = json.dumps({"rounds": 100, "seed": 3, "algorithm": "PCA",
                         "cells": [dict({k: v for k, v in cell.items() if k not in ("rounds", "seed")},
                                        summary=[dict(zip(M.METRICS, (float(v) for v in row)), timestep=t)
                                                 for t, row in enumerate(plain[:, c])])
                                   for c, cell in enumerate(cells)]}) + "\n"
    assert _run(capsys, argv) == expect


def test_cli_stats_on_one_cell(gpu_lib, capsys):
    """Single values: the equal-shape call's object, every timestep extended; without the flag byte for
    byte what it always printed."""
    M = _sim()
    argv = ["--rounds", "257", "--reporters", "30", "--events", "12", "--timesteps", "2", "--seed", "5",
            "--liars", "0.2", "--missing", "0.05"]
    one = M.simulate(257, 30, 12, 2, seed=5, liar_frac=0.2, na_frac=0.05)["summary"].cpu().numpy()
    expect = json.dumps({"rounds": 257, "reporters": 30, "events": 12, "seed": 5, "algorithm": "PCA",
                         "summary": [dict(zip(M.METRICS, (float(v) for v in row)), timestep=t)
                                     for t, row in enumerate(one)]}) + "\n"
    assert _run(capsys, argv) == expect
    got = json.loads(_run(capsys, argv + ["--stats"]))
    assert list(got) == ["rounds", "reporters", "events", "seed", "algorithm", "summary"]
    want = M.study([S.cell(257, 30, 12, 5, liar_frac=0.2, na_frac=0.05)], 2)
    stats = _host(want["stats"])
    for t, d in enumerate(got["summary"]):
        assert [d[k] for k in M.METRICS] == [float(v) for v in one[t]]  # one cell of a study is its simulate()
        assert all(_same_number(d["detail"][k], float(stats[t, 0, 6 + i, 1])) for i, k in enumerate(M.DETAIL))
        assert all(_same_number(d["stderr"][k], float(M.stderr(stats)[t, 0, i])) for i, k in enumerate(M.VALUES))
        assert "vs_first" not in d


# ------------------------------------------------------------------ nothing is launched
def test_empty_and_refused_studies_write_nothing(gpu_lib):
    import torch

    from pyconsensus_amd import _abi, _device, _lib

    M = _sim()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    sentinel = -12345.0
    bufs = {k: torch.full((4096,), sentinel, dtype=torch.float64, device=dev)
            for k in ("metrics", "summary", "reputation", "detail", "stats", "paired")}
    res, st = _abi.SimResult(), _abi.SimStudyResult()
    res.metrics, res.summary, res.reputation = (bufs[k].data_ptr() for k in ("metrics", "summary", "reputation"))
    st.detail, st.stats, st.paired = (bufs[k].data_ptr() for k in ("detail", "stats", "paired"))

    def untouched():
        _sync()
        return all(bool((b == sentinel).all()) for b in bufs.values())

    s, arr, _, _ = M._sweep([], 2)
    none = np.zeros(1, dtype=np.int32)  # (paired wants a pair_base, here of no cell)
    assert gpu_lib.pcx_simulate_study_f64(h, C.byref(s), none.ctypes.data, C.byref(res), C.byref(st)) == 0
    assert untouched()
    cells = [S.cell(4, 5, 3, 1), S.cell(4, 5, 3, 1), S.cell(5, 5, 3, 1)]
    s, arr, _, _ = M._sweep(cells, 2)
    for base, bad in (([-1, 3, -1], 1), ([0, -1, -1], 0), ([-1, -1, 0], 2)):
        b = np.asarray(base, dtype=np.int32)
        assert gpu_lib.pcx_simulate_study_f64(h, C.byref(s), b.ctypes.data, C.byref(res), C.byref(st)) == -1
        msg = gpu_lib.pcx_last_error().decode()
        assert msg.startswith("pcx_simulate_study_f64: ") and "cell %d:" % bad in msg, msg
        assert untouched()
        assert gpu_lib.pcx_sim_sweep_stats_f64(h, C.byref(s), bufs["metrics"].data_ptr(), bufs["detail"].data_ptr(),
                                               b.ctypes.data, bufs["stats"].data_ptr(), bufs["paired"].data_ptr()) == -1
        assert untouched()
    with pytest.raises(Exception) as e:
        M.study(cells, 2, pair_with=[-1, -1, 0])
    assert "cell 2:" in str(e.value)
    r = M.study([], 2, pair_with=[])
    _sync()
    assert r["stats"].shape == (2, 0, 18, 5) and r["paired"].shape == (2, 0, 18, 3) and r["metrics"].shape == (2, 0, 6)
