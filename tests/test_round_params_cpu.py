"""Per-round consensus parameters without a device: the ABI, the pure plan and
check entries with their refusals by index, and the Python cell and grid handling."""
import ctypes as C
import sys

import numpy as np
import pytest

import ragged_wide_cases as RW
import round_params_cases as RP


def _lib():
    from pyconsensus_amd import _lib

    return _lib.lib()


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401

    return sys.modules["pyconsensus_amd.simulate"]


def _err():
    return _lib().pcx_last_error().decode()


DEFAULTS = dict(algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
                hierarchy_threshold=0.5, cluster_threshold=None)


def params_array(sets):
    from pyconsensus_amd import _abi

    return (_abi.RoundParams * max(len(sets), 1))(*[_abi.round_params(dict(DEFAULTS, **q)) for q in sets])


def plan(shapes, sets, param_of, raw=None):
    """(rc, totals, n_launches, bad_round, bad_param) of pcx_ragged_plan_params."""
    sh = np.asarray(shapes, dtype=np.int32).reshape(-1, 2)
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    of = np.ascontiguousarray(param_of, dtype=np.int32)
    arr = raw if raw is not None else params_array(sets)
    totals, nl, br, bp = (C.c_int64 * 3)(), C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    rc = _lib().pcx_ragged_plan_params(len(sh), n.ctypes.data, e.ctypes.data, len(sets), C.cast(arr, C.c_void_p),
                                       of.ctypes.data, totals, C.byref(nl), C.byref(br), C.byref(bp))
    return rc, tuple(totals), nl.value, br.value, bp.value


# ------------------------------------------------------------------ ABI
def test_abi_struct_symbols_and_version():
    from pyconsensus_amd import _abi

    assert C.sizeof(_abi.RoundParams) == 48
    assert _abi.RoundParams.alpha.offset == 16 and _abi.RoundParams.cluster_threshold.offset == 40
    lib = _lib()
    for name in ("pcx_ragged_plan_params", "pcx_consensus_ragged_params_f64", "pcx_sim_study_params_check",
                 "pcx_simulate_study_params_f64"):
        assert hasattr(lib, name), name
    assert lib.pcx_abi_version() == 9


# ------------------------------------------------------------------ plan
def test_plan_totals_and_launches_of_a_hand_made_batch():
    shapes = [(1, 1), (5, 3), (64, 32), (65, 3), (256, 64), (100, 50)]
    sets = [{}, {"algorithm": "big-five"}, {"algorithm": "hierarchical"}]
    # one-wave: PCA, big-five, hierarchical -> three groups; 65 x 3 PCA and 100 x 50 PCA share the
    # plain instantiation (classes by their LDS), 256 x 64 hierarchical is a CLUS launch
    of = [0, 1, 2, 0, 2, 0]
    rc, totals, nl, br, bp = plan(shapes, sets, of)
    assert rc == 0 and (br, bp) == (-1, -1)
    assert totals == (sum(n for n, _ in shapes), sum(e for _, e in shapes), sum(n * e for n, e in shapes))
    classes = {RW.launch_class(65, 3, "PCA"), RW.launch_class(100, 50, "PCA")}
    assert nl == 3 + len(classes) + 1
    # every round on one set of one group: one launch
    assert plan(shapes[:3], sets[:1], [0, 0, 0])[2] == 1
    # the number of launches does not depend on P: sixty-four sets of one group
    many = [{"alpha": 0.01 * k} for k in range(64)]
    assert plan([(5, 3)] * 64, many, list(range(64)))[2] == 1


def test_plan_of_the_mixed_batch_reaches_every_group_and_class():
    """The GPU test's batch: the three one-wave groups, and the three launch classes of the workgroup
    kernel for its plain and for its CLUS instantiation."""
    shapes = RP.mix_shapes()
    wave, plain, clus = set(), set(), set()
    meets = {}
    for b, (N, E) in enumerate(shapes):
        alg = RP.set_name(RP.MIX_SETS[RP.mix_set_index(b)])
        meets.setdefault((N, E), set()).add(RP.mix_set_index(b))
        if RW.is_wave(N, E):
            wave.add("clus" if alg in ("hierarchical", "clusterfeck") else
                     "eigen" if alg in ("big-five", "fixed-variance") else "packed")
        else:
            (clus if alg in ("hierarchical", "clusterfeck") else plain).add(RW.launch_class(N, E, alg))
    assert wave == {"packed", "eigen", "clus"}
    # (no clustering round reaches class 1: the largest round the entry takes, 256 x 64, is of class 2
    # under both clusterings, and a round's LDS grows with N and with E -- so no shape can be added for it)
    assert RW.launch_class(256, 64, "hierarchical") == 2 and RW.launch_class(256, 64, "clusterfeck") == 2
    assert plain == {1, 2, 3} and clus == {2, 3}, (plain, clus)
    assert all(len(v) >= 3 for v in meets.values()), meets
    assert all(RP.mix_set_index(b) != RP.mix_set_index(b + 1) for b in range(RP.MIX_ROUNDS - 1))
    # big-five's max_components = 5 meets E = 3 on both kernels
    five = [shapes[b] for b in range(RP.MIX_ROUNDS) if RP.mix_set_index(b) == 3]
    assert (5, 3) in five and (65, 3) in five, five
    rc, totals, nl, br, bp = plan(shapes, RP.MIX_SETS, [RP.mix_set_index(b) for b in range(RP.MIX_ROUNDS)])
    assert rc == 0 and nl == 3 + 3 + 2
    from pyconsensus_amd.batched import ragged_plan

    assert totals == ragged_plan(shapes, wide=True)[0]


def test_plan_refusals_name_the_round_or_the_set():
    from pyconsensus_amd import _abi

    EINVAL = -1
    shapes, ok = [(5, 3), (6, 4)], [{}, {"algorithm": "absolute"}]
    rc, _, _, br, bp = plan(shapes, ok, [0, 2])
    assert rc == EINVAL and (br, bp) == (1, -1) and "round 1" in _err() and "param_of 2" in _err()
    rc, _, _, br, bp = plan(shapes, ok, [-1, 0])
    assert rc == EINVAL and br == 0 and "round 0" in _err()
    rc, _, _, br, bp = plan(shapes, [], [0, 0])
    assert rc == EINVAL and (br, bp) == (-1, -1) and "n_params" in _err()
    rc, _, _, br, bp = plan([(5, 3), (257, 4)], ok, [0, 1])
    assert rc == EINVAL and br == 1 and "round 1 is 257 x 4" in _err() and "[1, 256] x [1, 64]" in _err()

    def bad_set(why, **fields):
        arr = params_array(ok + [{}])
        for k, v in fields.items():
            setattr(arr[2], k, v)
        rc, _, _, br, bp = plan(shapes, ok + [{}], [0, 2], raw=arr)
        assert rc == EINVAL and (br, bp) == (-1, 2), (fields, rc, br, bp)
        assert "parameter set 2" in _err() and why in _err(), _err()

    bad_set("algorithm must be", algorithm=8)
    bad_set("algorithm must be", algorithm=-1)
    bad_set("k-means", algorithm=_abi.ALG_KMEANS)
    bad_set("alpha must be finite", alpha=float("nan"))
    bad_set("alpha must be finite", catch_tolerance=float("inf"))
    bad_set("big-five needs max_components >= 1", algorithm=_abi.ALG_BIG_FIVE, max_components=0)
    bad_set("hierarchy_threshold is NaN", algorithm=_abi.ALG_HIERARCHICAL, hierarchy_threshold=float("nan"))
    bad_set("variance_threshold must be finite", algorithm=_abi.ALG_FIXED_VARIANCE, variance_threshold=float("inf"))
    # ... only where the set's algorithm reads them
    arr = params_array(ok)
    arr[0].hierarchy_threshold = arr[0].variance_threshold = float("nan")
    arr[0].max_components = 0
    assert plan(shapes, ok, [0, 1], raw=arr)[0] == 0


def test_plan_of_an_empty_batch():
    rc, totals, nl, br, bp = plan([], [], [])
    assert rc == 0 and totals == (0, 0, 0) and nl == 0 and (br, bp) == (-1, -1)
    assert plan([], [{}], [])[0] == 0


# ------------------------------------------------------------------ the simulator's check
def test_study_params_check_refuses_by_cell():
    S = _sim()
    cells = [RP.cell(4, 5, 3, 1), dict(RP.cell(4, 5, 3, 1), algorithm="hierarchical", alpha=0.3),
             dict(RP.cell(4, 65, 33, 1), algorithm="clusterfeck")]
    assert list(S.study_check(cells, "first", 3)) == [-1, 0, -1]
    totals, counts, lds = S.sweep_plan(cells, 3)
    assert totals[0] == 12 and counts[0] == 8 and counts[1:].sum() == 4
    from pyconsensus_amd._lib import PcxError

    for key, value, why in (("algorithm", "cokurtosis", "cokurtosis is not simulated"),
                            ("algorithm", "k-means", "k-means is not simulated"),
                            ("alpha", float("nan"), "alpha must be finite"),
                            ("max_components", 0, None)):
        bad = [dict(c) for c in cells]
        bad[2][key] = value
        if why is None:  # max_components is read by big-five alone
            S.study_check(bad, None, 1)
            bad[2]["algorithm"] = "big-five"
            why = "big-five needs max_components >= 1"
        with pytest.raises(PcxError, match="cell 2: .*" + why):
            S.study_check(bad, None, 1)
    # the sweep's shared parameters are not read when the cells carry their own: a cell's key wins
    S.study_check([dict(c, algorithm="absolute") for c in cells], None, 1, algorithm="cokurtosis")
    with pytest.raises(PcxError, match="cokurtosis is not simulated"):
        S.study_check([RP.bare(c) for c in cells], None, 1, algorithm="cokurtosis")


# ------------------------------------------------------------------ Python: cells and grids
def test_cells_accept_the_parameter_keys():
    S = _sim()
    full = dict(RP.cell(3, 5, 3, 9), algorithm="absolute", catch_tolerance=0.2, alpha=0.3, max_components=2,
                variance_threshold=0.8, hierarchy_threshold=0.6, cluster_threshold=0.4)
    norm, arr, offsets = S._cells([full, (3, 5, 3, 9)])
    assert all(norm[0][k] == full[k] for k in RP.PARAM_KEYS)
    assert set(norm[1]) == set(S.CELL_FIELDS)  # a tuple cell fills CELL_FIELDS alone
    assert S.CELL_FIELDS == ("rounds", "reporters", "events", "seed", "liar_frac", "collude_frac", "distort",
                             "na_frac", "scaled_frac")
    assert arr[0].n_rounds == 3 and arr[1].n_reporters == 5
    with pytest.raises(ValueError, match="unknown field"):
        S._cells([dict(full, alhpa=0.3)])
    with pytest.raises(ValueError, match="a tuple cell is"):
        S._cells([(3, 5, 3, 9, 0.3, 0.5, 0.1, 0.1, 0.25, "absolute")])
    cp = S._cell_params(norm, alpha=0.7)
    assert cp[0].alpha == 0.3 and cp[1].alpha == 0.7 and cp[0].algorithm == 1 and cp[1].algorithm == 0
    assert S._cell_params(S._cells([(3, 5, 3, 9)])[0]) is None


def test_grid_takes_parameter_axes():
    S = _sim()
    g = S.grid(4, alpha=[0.1, 0.3], algorithm=["PCA", "absolute"])
    assert g == [{"rounds": 4, "seed": 0, "alpha": 0.1, "algorithm": "PCA"},
                 {"rounds": 4, "seed": 0, "alpha": 0.1, "algorithm": "absolute"},
                 {"rounds": 4, "seed": 0, "alpha": 0.3, "algorithm": "PCA"},
                 {"rounds": 4, "seed": 0, "alpha": 0.3, "algorithm": "absolute"}]
    assert list(S.pair_base(g, "first")) == [-1, 0, 0, 0]
    with pytest.raises(ValueError, match="unknown axis"):
        S.grid(4, alhpa=[0.1])


def test_param_sets_are_deduplicated():
    from pyconsensus_amd.batched import param_sets

    sets, of = param_sets([None, {"alpha": 0.3}, {}, {"alpha": 0.3}, {"algorithm": "absolute"}], DEFAULTS, "per_round")
    assert list(of) == [0, 1, 0, 1, 2] and len(sets) == 3 and sets[1]["alpha"] == 0.3 and sets[1]["algorithm"] == "PCA"
    with pytest.raises(ValueError, match=r"per_round\[1\]: unknown parameter"):
        param_sets([None, {"alhpa": 0.3}], DEFAULTS, "per_round")


def test_alpha_acts_on_the_liars_reputation_in_the_host_replay():
    """What the GPU test asserts of the alpha = 0.5 cell's paired difference, on the host: the liars'
    reputation after the round differs from the alpha = 0.1 run's at every timestep."""
    for base in RP.STUDY_BASES[1:]:
        a = RP.replay(base, RP.STUDY_T, alpha=0.1)["metrics"][:, :, 2]
        b = RP.replay(base, RP.STUDY_T, alpha=0.5)["metrics"][:, :, 2]
        assert (np.abs((b - a).mean(axis=1)) > 1e-6).all(), base
