"""Ragged batches on the GPU: rounds of different shapes in one launch of the one-wave round kernel
(batched.consensus_ragged, pcx_consensus_ragged_f64) and consensus_many on top of it.  Every output is
compared as bits, NaN equal to NaN: a round in a ragged launch is that round's own equal-shape launch."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import golden_cases as G
import parity as P

pytestmark = pytest.mark.gpu

ALGORITHMS = ["PCA", "absolute", "big-five", "fixed-variance", "cokurtosis", "hierarchical", "clusterfeck"]
# the sizes at which an offset, a pitch (odd / even E) or a carve error shows; the 50 x 20 rounds pin the
# generic instance against the compiled one
MIX_SHAPES = [(1, 1), (1, 6), (30, 1), (2, 2), (7, 13), (50, 20), (63, 31), (64, 1), (1, 32), (64, 32)]
MIX_ROUNDS = 512


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    same = _bits(a) == _bits(b)
    if a.dtype.kind == "f":
        same = same | (np.isnan(a) & np.isnan(b))
    assert np.all(same), (what, int(np.size(same) - np.count_nonzero(same)))


def _host(out):
    from pyconsensus_amd.batched import ragged_to_host

    return ragged_to_host(out)


@functools.lru_cache(maxsize=None)
def _mix():
    """The seeded mix: per shape its rounds (synthetic.rounds) and, per round of the shuffled
    order, (shape index, index among that shape's rounds)."""
    from pyconsensus_amd import synthetic

    rng = np.random.default_rng(20261019)
    which = np.concatenate([np.arange(len(MIX_SHAPES)), rng.integers(0, len(MIX_SHAPES), MIX_ROUNDS - len(MIX_SHAPES))])
    rng.shuffle(which)
    per, order, seen = [], [], [0] * len(MIX_SHAPES)
    for k, (N, E) in enumerate(MIX_SHAPES):
        R, sc, lo, hi, rep = synthetic.rounds(int(np.sum(which == k)), N, E, seed=700 + k)
        aux = np.random.default_rng(900 + k).normal(size=(R.shape[0], N))
        per.append(dict(R=R, scaled=sc, lo=lo, hi=hi, reputation=rep, aux=aux))
    for k in which:
        order.append((int(k), seen[k]))
        seen[k] += 1
    return per, order


def _alg_kw(alg):
    kw = dict(algorithm=alg)
    if alg in ("big-five", "fixed-variance"):
        kw.update(max_components=5, variance_threshold=0.75)  # (5 > E for five of the shapes: capped per round)
    return kw


def _run_mix(order, alg, **extra):
    from pyconsensus_amd.batched import consensus_ragged

    per, _ = _mix()
    pick = lambda key: [per[k][key][i] for k, i in order]
    kw = _alg_kw(alg)
    if alg == "cokurtosis":
        kw["aux_scores"] = pick("aux")
    return consensus_ragged(pick("R"), pick("reputation"), pick("scaled"), pick("lo"), pick("hi"), filled=True,
                            original=True, **kw, **extra)


@functools.lru_cache(maxsize=None)
def _spec(alg):
    """The C SPEC's outputs of the mix's rounds, one run per shape."""
    from oracle import pcx_oracle_c as OC

    per, _ = _mix()
    ref = []
    for d in per:
        kw = _alg_kw(alg)
        if alg == "cokurtosis":
            kw["aux_scores"] = d["aux"]
        ref.append(OC.batched(d["R"], d["scaled"], d["lo"], d["hi"], d["reputation"], threads=8, **kw))
    return ref


def _check_against_spec(host, order, alg, what):
    from pyconsensus_amd.batched import ragged_round

    ref = _spec(alg)
    names = [k for k in host if not k.startswith("_")]
    assert {"original", "filled", "smooth_rep", "outcomes_final", "branch", "components"} <= set(names)
    for b, (k, i) in enumerate(order):
        g = ragged_round(host, b)
        for name in names:
            assert_same_bits(g[name], ref[k][name][i], (what, alg, b, MIX_SHAPES[k], name))


@pytest.mark.parametrize("alg", ALGORITHMS)
def test_seeded_mix_bitexact_vs_spec(gpu_lib, alg):
    """512 rounds of ten shapes in shuffled order, one launch: every output of every round, `original`
    and `filled` included, equals the C SPEC run on that round's shape."""
    _, order = _mix()
    assert len(order) == MIX_ROUNDS and {k for k, _ in order} == set(range(len(MIX_SHAPES)))
    out = _run_mix(order, alg)
    assert out["_shapes"].shape == (MIX_ROUNDS, 2)
    for key in ("_reporter_offsets", "_event_offsets", "_cell_offsets"):
        assert out[key].dtype == np.int64 and out[key].shape == (MIX_ROUNDS + 1,) and out[key][0] == 0
    assert out["smooth_rep"].is_cuda and out["smooth_rep"].shape == (int(out["_reporter_offsets"][-1]),)
    assert out["filled"].shape == (int(out["_cell_offsets"][-1]),) and out["branch"].shape == (MIX_ROUNDS,)
    _check_against_spec(_host(out), order, alg, "mix")


@pytest.mark.parametrize("alg", ["PCA", "clusterfeck"])
def test_reversed_order_gives_reversed_outputs(gpu_lib, alg):
    """The same rounds in reversed order give the reversed outputs, bit for bit (a write outside a
    round's own ranges would land in another round's)."""
    from pyconsensus_amd.batched import ragged_round

    _, order = _mix()
    order = order[:192]
    fwd, rev = _host(_run_mix(order, alg)), _host(_run_mix(order[::-1], alg))
    B = len(order)
    for b in range(B):
        f, r = ragged_round(fwd, b), ragged_round(rev, B - 1 - b)
        for name in f:
            assert_same_bits(f[name], r[name], (alg, b, name))


def test_back_to_back_calls(gpu_lib):
    """Calls with different shape lists and no synchronisation between them -- more calls than the
    library has descriptor staging slots -- are all correct after one sync, and the same call twice
    gives identical bits."""
    import torch

    _, order = _mix()
    lists = [order[:200], order[200:260], order[100:400], order[:200], order[300:]]
    outs = [_run_mix(o, "PCA") for o in lists]
    torch.cuda.synchronize()
    hosts = [_host(o) for o in outs]
    for h, o in zip(hosts, lists):
        _check_against_spec(h, o, "PCA", "back-to-back")
    for name in (k for k in hosts[0] if not k.startswith("_")):
        assert_same_bits(hosts[0][name], hosts[3][name], ("twice", name))


def _golden_groups():
    groups = {}
    for name, case in list(G.kat().items()) + list(G.mixed().items()):
        N, E = case["in_reports"].shape
        if name in P.EXCLUDED or N > 64 or E > 32:
            continue
        key = (bool(case["in_has_bounds"]), bool(case["in_has_rep"]), float(case["in_catch_tolerance"]),
               float(case["in_alpha"]), bool(case["in_int_dtype"]))
        groups.setdefault(key, []).append((name, case))
    return groups


def test_goldens_one_launch_per_group(gpu_lib):
    """Every KAT and mixed golden round of at most 64 x 32 -- the case set of
    test_batched_gpu.test_golden_kat_and_mixed -- in one ragged launch per (bounds, reputation,
    catch_tolerance, alpha, int dtype) group: the known-mismatch list holds unchanged, and every
    output equals the case's own consensus_batched run."""
    from pyconsensus_amd.batched import consensus_batched, consensus_ragged, ragged_round

    groups = _golden_groups()
    assert sum(len(v) for v in groups.values()) >= 20 and len({c["in_reports"].shape for v in groups.values()
                                                               for _, c in v}) >= 5
    observed, ran = {}, []
    for (bounds, has_rep, tol, alpha, ints), cases in groups.items():
        kw = {}
        if bounds:
            kw.update(scaled=[c["in_scaled"] for _, c in cases], lo=[c["in_lo"] for _, c in cases],
                      hi=[c["in_hi"] for _, c in cases])
        if has_rep:
            kw["reputation"] = [c["in_reputation"] for _, c in cases]
        host = _host(consensus_ragged([c["in_reports"] for _, c in cases], catch_tolerance=tol, alpha=alpha,
                                      int_dtype=ints, filled=True, original=True, **kw))
        for b, (name, c) in enumerate(cases):
            g = ragged_round(host, b)
            ran.append(name)
            kind, _ = P.mismatch_kind(c, g)
            if kind:
                observed[name] = kind
            one = {}
            if bounds:
                one.update(scaled=c["in_scaled"][None], lo=c["in_lo"][None], hi=c["in_hi"][None])
            if has_rep:
                one["reputation"] = c["in_reputation"][None]
            own = consensus_batched(c["in_reports"][None], catch_tolerance=tol, alpha=alpha, int_dtype=ints,
                                    filled=True, original=True, **one)
            for k, v in g.items():
                assert_same_bits(v, own[k].cpu().numpy()[0], (name, k))
    P.assert_known("exact", observed, ran)


def test_refusals_launch_nothing(gpu_lib):
    """k-means, a 65 x 4 round and a 4 x 33 round are refused with the round named; nothing is
    launched (the outputs keep their bytes); a valid call afterwards succeeds."""
    import torch

    from pyconsensus_amd import _abi, _device, _lib
    from pyconsensus_amd.batched import consensus_ragged

    ok = [np.full((3, 4), 1.0), np.full((5, 2), 2.0)]
    with pytest.raises(_lib.PcxError, match="k-means"):
        consensus_ragged(ok, algorithm="k-means")
    with pytest.raises(_lib.PcxError, match="round 2 is 65 x 4"):
        consensus_ragged(ok + [np.ones((65, 4))])
    with pytest.raises(_lib.PcxError, match="round 1 is 4 x 33"):
        consensus_ragged([ok[0], np.ones((4, 33)), ok[1]])
    # the C call itself: refused before anything reaches the stream
    dev = torch.device("cuda", torch.cuda.current_device())
    n, e = np.array([3, 65], dtype=np.int32), np.array([4, 4], dtype=np.int32)
    R = torch.ones(3 * 4 + 65 * 4, dtype=torch.float64, device=dev)
    sentinel = torch.full((68,), -7.0, dtype=torch.float64, device=dev)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    for alg, shapes_n in ((_abi.ALG_PCA, n), (_abi.ALG_KMEANS, np.array([3, 5], dtype=np.int32))):
        inp = _abi.Ragged(2, shapes_n.ctypes.data, e.ctypes.data, R.data_ptr(), None, None, None, None, 0, alg,
                          0.1, 0.1, 5, 0.9, None, 0.5, 0.0)
        res = _abi.BatchResult()
        res.smooth_rep = sentinel.data_ptr()
        assert gpu_lib.pcx_consensus_ragged_f64(h, C.byref(inp), C.byref(res)) == _abi.EINVAL
    msg = gpu_lib.pcx_last_error()
    assert b"k-means" in msg
    torch.cuda.synchronize()
    assert bool((sentinel == -7.0).all())
    # an empty batch succeeds and launches nothing
    inp = _abi.Ragged(0, None, None, None, None, None, None, None, 0, 0, 0.1, 0.1, 5, 0.9, None, 0.5, 0.0)
    assert gpu_lib.pcx_consensus_ragged_f64(h, C.byref(inp), C.byref(_abi.BatchResult())) == 0
    empty = consensus_ragged([])
    assert empty["smooth_rep"].numel() == 0 and empty["_cell_offsets"].tolist() == [0]
    out = _host(consensus_ragged(ok))
    assert out["outcomes_final"].tolist() == [1.0] * 4 + [2.0] * 2


# ---------------------------------------------------------------- consensus_many
README = dict(reports=[[0.2, 0.7, 1, 1], [0.3, 0.5, 1, 1], [0.1, 0.7, 1, 1],
                       [0.5, 0.7, 2, 1], [0.1, 0.2, 2, 2], [0.1, 0.2, 2, 2]],
              reputation=[1, 2, 10, 9, 4, 2],
              event_bounds=[{"scaled": True, "min": 0.1, "max": 0.5}, {"scaled": True, "min": 0.2, "max": 0.7},
                            {"scaled": False, "min": 1, "max": 2}, {"scaled": False, "min": 1, "max": 2}])


def _problems():
    from pyconsensus_amd import synthetic

    ps = [copy.deepcopy(README)]
    kinds = {}  # (bounds, reputation, int dtype) -> its cases; a dozen taken kind by kind in turn
    for name, case in sorted(list(G.kat().items()) + list(G.mixed().items())):
        N, E = case["in_reports"].shape
        if name not in P.EXCLUDED and N <= 64 and E <= 32:
            kinds.setdefault((bool(case["in_has_bounds"]), bool(case["in_has_rep"]), bool(case["in_int_dtype"])),
                             []).append(case)
    assert len(kinds) >= 3 and sum(len(v) for v in kinds.values()) >= 12, {k: len(v) for k, v in kinds.items()}
    picked = [v[i] for i in range(12) for _, v in sorted(kinds.items()) if i < len(v)][:12]
    for case in picked:
        kw = G.oracle_args(case)
        kw.pop("algorithm")
        ps.append(kw)
    R, sc, lo, hi, rep = synthetic.matrix(70, 5, seed=11)  # above one wave: through Oracle itself
    ps.append(dict(reports=R, event_bounds=synthetic.bounds_list(sc, lo, hi), reputation=rep))
    return ps


def _same_value(a, b, path):
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), (path, list(a), list(b))
        for k in a:
            _same_value(a[k], b[k], path + (k,))
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_value(x, y, path + (i,))
    elif isinstance(a, np.ma.MaskedArray):
        assert np.array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b)), path
        assert_same_bits(np.ma.getdata(a), np.ma.getdata(b), path)
    elif isinstance(a, np.ndarray):
        assert_same_bits(a, b, path)
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("alg", ["PCA", "big-five"])
def test_consensus_many_equals_the_oracle_loop(gpu_lib, alg):
    """The README's 6 x 4 example, a dozen goldens of mixed kinds and a 70 x 5 problem (the fallback):
    each result dict equals Oracle(...).consensus() of the same problem in keys, container types and
    values; under big-five max_components = 5 exceeds E for some problems and is capped per round."""
    from pyconsensus_amd import Oracle, consensus_many

    a, b = _problems(), _problems()  # (Oracle rescales a caller's float matrix in place: one copy each)
    assert any(np.asarray(p["reports"]).shape[1] < 5 for p in a)
    many = consensus_many(a, algorithm=alg)
    assert isinstance(many, list) and len(many) == len(b)
    for i, p in enumerate(b):
        _same_value(many[i], Oracle(**p, algorithm=alg).consensus(), (alg, i))
        assert_same_bits(np.asarray(a[i]["reports"], dtype=np.float64),
                         np.asarray(p["reports"], dtype=np.float64), (alg, i, "caller's matrix"))
