"""Per-round consensus parameters on the GPU: rounds of one ragged call, and cells
of one study, each under its own algorithm and options.

The new kernels are the texts of the kernels they are compared with, so every comparison is bit for
bit (all NaNs alike): a mixed call against the shared-parameter calls of its sets, a study's cells
against their own studies on the existing entry, and one cell against a host replay.
"""
import sys

import numpy as np
import pytest

import round_params_cases as RP

pytestmark = pytest.mark.gpu

W = RP.W
OUTPUTS_N = ("old_rep", "this_rep", "smooth_rep", "scores", "na_row", "participation_rows", "relative_part",
             "reporter_bonus")


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401

    return sys.modules["pyconsensus_amd.simulate"]


def _sync():
    import torch

    torch.cuda.synchronize()


def _host(x):
    return x.cpu().numpy()


# ------------------------------------------------------------------ 1. mixed rounds
_RAGGED = {}


def ragged(key, **kw):
    """A consensus_ragged(wide=True) run of the mixed batch on the host (computed once, left unchanged)."""
    from pyconsensus_amd.batched import consensus_ragged, ragged_to_host

    if key not in _RAGGED:
        R, rep, sc, lo, hi, aux = RP.mix_inputs()
        _RAGGED[key] = ragged_to_host(consensus_ragged(R, rep, sc, lo, hi, aux_scores=aux, wide=True, filled=True,
                                                       original=True, **kw))
    return _RAGGED[key]


def assert_round_equal(got, want, b, what):
    from pyconsensus_amd.batched import ragged_round

    g, w = ragged_round(got, b), ragged_round(want, b)
    assert set(g) == set(w) and {"filled", "original", "branch", "flags", "pi_iters", "components"} <= set(g)
    for name in w:
        assert RP.same_bits(np.asarray(g[name]), np.asarray(w[name])), (what, b, name)


def test_mixed_rounds_equal_their_shared_parameter_runs(gpu_lib):
    per_round = [RP.MIX_SETS[RP.mix_set_index(b)] for b in range(RP.MIX_ROUNDS)]
    mixed = ragged("mixed", per_round=per_round)
    assert len(mixed["_shapes"]) == RP.MIX_ROUNDS
    for q, kw in enumerate(RP.MIX_SETS):
        want = ragged("set%d" % q, **kw)  # the existing entry: the whole batch with the set shared
        for b in range(RP.MIX_ROUNDS):
            if RP.mix_set_index(b) == q:
                assert_round_equal(mixed, want, b, RP.set_name(kw))
    # what the sets are there to reach: a capped big-five round, components of fixed-variance, both PCAs apart
    comps = mixed["components"]
    assert all(comps[b] >= 1 for b in range(RP.MIX_ROUNDS) if RP.mix_set_index(b) == 4)
    assert all(comps[b] == -1 for b in range(RP.MIX_ROUNDS) if RP.mix_set_index(b) != 4)
    assert not RP.same_bits(ragged("set0")["smooth_rep"], ragged("set1", **RP.MIX_SETS[1])["smooth_rep"])


def test_every_round_on_one_set_equals_the_shared_call(gpu_lib):
    one = ragged("all0", per_round=[RP.MIX_SETS[0]] * RP.MIX_ROUNDS)
    want = ragged("set0", **RP.MIX_SETS[0])
    names = [name for name in want if not name.startswith("_")]
    assert len(names) == 25 and set(names) == {name for name in one if not name.startswith("_")}
    for name in names:
        assert RP.same_bits(one[name], want[name]), name


def test_per_round_keeps_the_narrow_limit_and_refuses_by_set(gpu_lib):
    from pyconsensus_amd._lib import PcxError
    from pyconsensus_amd.batched import consensus_ragged

    rng = np.random.default_rng(3)
    mats = [rng.integers(1, 3, (5, 3)).astype(float), rng.integers(1, 3, (65, 3)).astype(float)]
    with pytest.raises(PcxError, match="round 1 is 65 x 3"):
        consensus_ragged(mats, per_round=[{}, {"alpha": 0.3}])
    with pytest.raises(PcxError, match="parameter set 1: k-means"):
        consensus_ragged(mats, per_round=[{}, {"algorithm": "k-means"}], wide=True)
    with pytest.raises(ValueError, match="cokurtosis needs aux_scores"):
        consensus_ragged(mats, per_round=[{}, {"algorithm": "cokurtosis"}], wide=True)
    with pytest.raises(ValueError, match="one entry per round"):
        consensus_ragged(mats, per_round=[{}], wide=True)
    empty = consensus_ragged([], per_round=[], wide=True)
    _sync()
    assert empty["smooth_rep"].numel() == 0


# ------------------------------------------------------------------ 2. a study's cells
_STUDY = {}


def study(cells, pair_with=None, **kw):
    """A study with everything kept, on the host (computed once per argument set, left unchanged)."""
    import json

    key = (json.dumps(cells, sort_keys=True), json.dumps(pair_with), json.dumps(kw, sort_keys=True))
    if key not in _STUDY:
        r = _sim().study(cells, RP.STUDY_T, pair_with=pair_with, keep_detail=True, keep_rounds=True, keep_outputs=True,
                         **kw)
        _sync()
        got = {k: _host(r[k]) for k in ("metrics", "summary", "reputation", "stats", "detail")}
        got["paired"] = _host(r["paired"]) if "paired" in r else None
        got["pair_base"] = r.get("pair_base")
        got["rounds"] = {k: _host(v) for k, v in r["rounds"].items()}
        got["outputs"] = {k: _host(v) for k, v in r["outputs"].items()}
        got["offsets"] = r["offsets"]
        _STUDY[key] = got
    return _STUDY[key]


def mixed_study():
    cells, sets = RP.study_cells()
    return cells, sets, study(cells, pair_with="first")


def test_a_studys_cells_equal_their_own_studies(gpu_lib):
    from pyconsensus_amd import _abi

    cells, sets, r = mixed_study()
    off = r["offsets"]
    kind_of = {name: {"N": "reporters", "E": "events", "1": "rounds"}[kind] for name, kind, _ in _abi.BATCH_OUTPUTS
               if name not in ("original", "filled")}
    for c, (k, q) in enumerate(zip(cells, sets)):
        own = study([RP.bare(k)], **q)  # the existing entry: the cell alone, its set as the keywords
        rows = slice(int(off["rounds"][c]), int(off["rounds"][c + 1]))
        assert RP.same_bits(r["metrics"][:, rows], own["metrics"]), (c, "metrics")
        assert RP.same_bits(r["detail"][:, rows], own["detail"]), (c, "detail")
        assert RP.same_bits(r["summary"][:, c], own["summary"][:, 0]), (c, "summary")
        assert RP.same_bits(r["stats"][:, c], own["stats"][:, 0]), (c, "stats")
        assert RP.same_bits(W.cell_slice(r["reputation"], off, "reporters", c), own["reputation"]), (c, "reputation")
        for name in W.ROUNDS:
            assert RP.same_bits(W.cell_slice(r["rounds"][name], off, W.OFFSET_OF[name], c), own["rounds"][name]), (c, name)
        for name, kind in kind_of.items():
            assert RP.same_bits(W.cell_slice(r["outputs"][name], off, kind, c), own["outputs"][name]), (c, name)


def test_a_studys_paired_differences(gpu_lib):
    M = _sim()
    cells, sets, r = mixed_study()
    n_sets = len(RP.STUDY_SETS)
    base = [-1 if c % n_sets == 0 else c - c % n_sets for c in range(len(cells) - 1)] + [n_sets]
    assert list(r["pair_base"]) == base
    alone = M.sweep_stats(cells, r["metrics"], r["detail"], pair_with="first")  # the existing stand-alone entry
    assert RP.same_bits(_host(alone["paired"]), r["paired"]) and RP.same_bits(_host(alone["stats"]), r["stats"])
    # a cell paired with a copy under the same set: every difference is zero
    copy = r["paired"][:, len(cells) - 1]
    assert (copy[:, :, 1][copy[:, :, 0] > 0] == 0).all() and (copy[:, :, 2][copy[:, :, 0] > 1] == 0).all()
    assert (copy[:, :6, 0] == cells[-1]["rounds"]).all()
    # the alpha = 0.5 cells against their alpha = 0.1 bases: the liars' reputation after the round moves
    # (test_round_params_cpu.py shows the same on the host replay)
    after = M.VALUES.index("liar_rep_after")
    for b in range(1, len(RP.STUDY_BASES)):
        assert (r["paired"][1:, b * n_sets + 1, after, 1] != 0).all(), b
    # and a set that changes the algorithm changes the outcomes somewhere
    assert not RP.same_bits(r["metrics"][:, int(r["offsets"]["rounds"][n_sets + 3]):int(r["offsets"]["rounds"][n_sets + 4])],
                            r["metrics"][:, int(r["offsets"]["rounds"][n_sets]):int(r["offsets"]["rounds"][n_sets + 1])])


# ------------------------------------------------------------------ 3. host replay
def test_a_cell_matches_its_host_replay(gpu_lib):
    """Hierarchical with alpha = 0.3 on the 5 x 3 cell, beside a PCA cell of the same rounds: generate_host,
    the C oracle with the carried reputation, numpy metrics -- tests/test_sim_gpu.py's rules."""
    base = RP.STUDY_BASES[1]
    q = {"algorithm": "hierarchical", "alpha": 0.3}
    cells = [dict(base), dict(base, **q)]
    r = study(cells)
    off = r["offsets"]
    for c, params in enumerate(({}, q)):
        want = RP.replay(base, RP.STUDY_T, **params)
        rows = slice(int(off["rounds"][c]), int(off["rounds"][c + 1]))
        assert RP.same_bits(r["metrics"][:, rows], want["metrics"]), c
        assert RP.same_bits(r["summary"][:, c], want["summary"]), c
        assert RP.same_bits(W.cell_slice(r["reputation"], off, "reporters", c), want["reputation"].reshape(-1)), c


# ------------------------------------------------------------------ 4. asynchrony
def test_params_study_returns_before_the_stream_reaches_it(gpu_lib):
    """tests/test_sim_sweep_gpu.py's method: behind a long queue of matrix products a T = 6 study with
    per-cell parameters returns while an event recorded BEFORE it is still pending."""
    import torch

    S = _sim()
    cells = [dict(W.cell(64, 50, 20, 1), alpha=0.3), dict(W.cell(4, 100, 50, 2), algorithm="hierarchical"),
             dict(W.cell(2, 256, 64, 3), algorithm="big-five"), W.cell(8, 5, 3, 4)]
    S.study(cells, 6, pair_with=[-1, -1, -1, -1])  # the work buffers, the staging slots and the allocator are warm
    x = torch.randn(4096, 4096, dtype=torch.float64, device="cuda")
    y = x @ x
    _sync()
    ev = torch.cuda.Event()
    for _ in range(40):  # (some hundred milliseconds of fp64 products)
        y = x @ x
    ev.record()
    r = S.study(cells, 6, pair_with=[-1, -1, -1, -1])
    returned_early = not ev.query()
    _sync()
    assert returned_early, "study() blocked the host until the work queued before it had run"
    warm = S.study(cells, 6, pair_with=[-1, -1, -1, -1])
    _sync()
    assert RP.same_bits(_host(r["stats"]), _host(warm["stats"]))


# ------------------------------------------------------------------ 5. Python routing
def test_cells_without_parameter_keys_keep_the_sweeps_contract(gpu_lib):
    """No cell carries a parameter: the existing entry, whose documented contract is that cell c's slice
    is simulate() of that cell with the shared parameters."""
    S = _sim()
    cells = [RP.bare(c) for c in RP.STUDY_BASES[1:]]
    kw = dict(algorithm="absolute", alpha=0.3)
    assert S._cell_params(S._cells(cells)[0], **kw) is None
    r = study(cells, **kw)
    for c, k in enumerate(cells):
        one = S.simulate(k["rounds"], k["reporters"], k["events"], RP.STUDY_T, seed=k["seed"], **W.rates(k), **kw)
        _sync()
        rows = slice(int(r["offsets"]["rounds"][c]), int(r["offsets"]["rounds"][c + 1]))
        assert RP.same_bits(r["metrics"][:, rows], _host(one["metrics"])), c
        assert RP.same_bits(r["summary"][:, c], _host(one["summary"])), c
    # ... and a cell that carries the same values as keys gives the same bytes through the new entry
    keyed = study([dict(c, **kw) for c in cells])
    for name in ("metrics", "summary", "reputation", "stats", "detail"):
        assert RP.same_bits(keyed[name], r[name]), name


def test_command_line_lists_of_algorithms_and_alphas(gpu_lib, capsys):
    import json

    S = _sim()
    argv = ["--rounds", "16", "--reporters", "5", "--events", "3", "--timesteps", "2", "--seed", "7"]
    assert S.main(argv + ["--algorithm", "PCA,absolute", "--alpha", "0.1,0.5", "--catch", "0.2", "--paired"]) == 0
    got = json.loads(capsys.readouterr().out)
    assert got["algorithm"] == "PCA,absolute" and len(got["cells"]) == 4
    # each cell's object gains the parameter keys that vary (and only those), in grid order
    assert [(c["algorithm"], c["alpha"]) for c in got["cells"]] == [("PCA", 0.1), ("PCA", 0.5), ("absolute", 0.1),
                                                                    ("absolute", 0.5)]
    assert all("catch_tolerance" not in c for c in got["cells"])
    assert "vs_first" not in got["cells"][0]["summary"][1] and "vs_first" in got["cells"][3]["summary"][1]
    cells = S.grid(16, seed=7, reporters=[5], events=[3], liar_frac=[0.3], collude_frac=[0.5], distort=[0.1],
                   na_frac=[0.1], scaled_frac=[0.25], algorithm=["PCA", "absolute"], alpha=[0.1, 0.5])
    want = study(cells, catch_tolerance=0.2)["summary"]
    for c in range(4):
        assert [got["cells"][c]["summary"][t]["liar_rep_after"] for t in range(2)] == want[:2, c, 2].tolist()
    # a single name and value: the object as before, the value the call's keyword
    assert S.main(argv + ["--algorithm", "absolute", "--alpha", "0.5"]) == 0
    one = json.loads(capsys.readouterr().out)
    assert one["algorithm"] == "absolute" and "cells" not in one
    r = S.simulate(16, 5, 3, 2, seed=7, algorithm="absolute", alpha=0.5)
    _sync()
    assert one["summary"][1]["liar_rep_after"] == float(r["summary"][1, 2])


def test_consensus_ragged_without_per_round_is_unchanged(gpu_lib):
    """Round b of the plain call is consensus_batched of round b (its documented contract)."""
    from pyconsensus_amd.batched import consensus_batched, ragged_round

    R, rep, sc, lo, hi, aux = RP.mix_inputs()
    got = ragged("set0", **RP.MIX_SETS[0])
    for b in (1, 4, 5):  # 3 x 33, 5 x 3, 100 x 50
        one = consensus_batched(R[b][None], rep[b][None], sc[b][None], lo[b][None], hi[b][None])
        _sync()
        g = ragged_round(got, b)
        for name in OUTPUTS_N + ("outcomes_final", "certainty"):
            assert RP.same_bits(np.asarray(g[name]), _host(one[name])[0]), (b, name)
