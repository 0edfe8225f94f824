"""Wide ragged batches on the GPU: rounds up to 256 x 64 in one call (batched.consensus_ragged with
wide=True, pcx_consensus_ragged_wide_f64) -- the one-wave kernel for the rounds of at most 64 x 32 with
the scatter of their per-round outputs, the ragged form of the workgroup kernel for the others, one
launch per launch class -- and consensus_many(wide=True) on top.  Every output is compared as bits, NaN
equal to NaN, against the C SPEC run on each round's own shape.  The inputs' preconditions are
asserted in test_ragged_wide_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import golden_cases as G
import parity as P
import ragged_wide_cases as W
from test_ragged_gpu import assert_same_bits

pytestmark = pytest.mark.gpu

PER_ROUND = ("participation", "avg_certainty", "branch", "flags", "pi_iters", "components")


def _host(out):
    from pyconsensus_amd.batched import ragged_to_host

    return ragged_to_host(out)


def _run_mix(order, alg, wide=True, filled=True, original=True):
    from pyconsensus_amd.batched import consensus_ragged

    args, kw = W.mix_call(order, alg)
    return consensus_ragged(*args, filled=filled, original=original, wide=wide, **kw)


def _check_against_spec(host, order, alg, what, must=("original", "filled")):
    from pyconsensus_amd.batched import ragged_round

    ref = W.mix_spec(alg)
    names = [k for k in host if not k.startswith("_")]
    assert set(must + PER_ROUND + ("smooth_rep", "outcomes_final")) <= set(names)
    for b, (k, i) in enumerate(order):
        g = ragged_round(host, b)
        for name in names:
            assert_same_bits(g[name], ref[k][name][i], (what, alg, b, W.MIX_SHAPES[k], name))


@pytest.mark.parametrize("alg", W.ALGORITHMS)
def test_seeded_mix_bitexact_vs_spec(gpu_lib, alg):
    """256 rounds of fourteen shapes in shuffled order, one call: every output of every round --
    `original`, `filled` and the six per-round outputs (a wrong scatter or round index shows there)
    included -- equals the C SPEC run on that round's shape."""
    _, order = W.mix()
    out = _run_mix(order, alg)
    assert out["_shapes"].shape == (W.MIX_ROUNDS, 2) and out["branch"].shape == (W.MIX_ROUNDS,)
    assert out["smooth_rep"].is_cuda and out["smooth_rep"].shape == (int(out["_reporter_offsets"][-1]),)
    assert out["filled"].shape == (int(out["_cell_offsets"][-1]),)
    _check_against_spec(_host(out), order, alg, "mix")


@pytest.mark.parametrize("alg", ["PCA", "clusterfeck"])
def test_mix_without_filled_and_original(gpu_lib, alg):
    """filled=False, original=False: the filled matrices live in the kernel's scratch, at the slot
    strides of the launch's largest round; both outputs are null."""
    _, order = W.mix()
    host = _host(_run_mix(order, alg, filled=False, original=False))
    assert "filled" not in host and "original" not in host
    _check_against_spec(host, order, alg, "no filled / original", must=())


def _workgroup_rounds(n):
    """n rounds of the mix above one wave, of two launch classes (100 x 50 and 256 x 64 among them)."""
    _, order = W.mix()
    take = [o for o in order if not W.is_wave(*W.MIX_SHAPES[o[0]])]
    big = [o for o in take if W.MIX_SHAPES[o[0]] == (256, 64)][:3]
    rest = [o for o in take if o not in big][:n - len(big)]
    picked = rest[:5] + big[:1] + rest[5:12] + big[1:] + rest[12:]
    assert len(picked) == n and len({W.launch_class(*W.MIX_SHAPES[k], "PCA") for k, _ in picked}) == 2
    return picked


def test_chunked_scratch_equals_one_chunk(gpu_lib):
    """A scratch cap that holds three 256 x 64 rounds: 20 workgroup rounds of two classes run in
    chunks and give the bits of the uncapped call; with the cap back at its default, so does the
    next call."""
    import torch

    from pyconsensus_amd import _lib

    order = _workgroup_rounds(20)
    ctx = _lib.context(torch.cuda.current_device())
    whole = _host(_run_mix(order, "PCA", filled=False, original=False))
    per_round = (256 * 64 + 64 * 64) * 8  # the filled matrix and the covariance of a 256 x 64 round
    _lib.check(gpu_lib.pcx_test_scratch_cap(ctx, 3 * per_round))
    try:
        capped = _host(_run_mix(order, "PCA", filled=False, original=False))
    finally:
        _lib.check(gpu_lib.pcx_test_scratch_cap(ctx, 0))
    again = _host(_run_mix(order, "PCA", filled=False, original=False))
    for name in (k for k in whole if not k.startswith("_")):
        assert_same_bits(capped[name], whole[name], ("capped", name))
        assert_same_bits(again[name], whole[name], ("cap cleared", name))
    _check_against_spec(whole, order, "PCA", "uncapped", must=())


@pytest.mark.parametrize("alg", W.SIDE_ALGS)
def test_side_and_median_rounds_in_one_wide_launch(gpu_lib, alg):
    """The covariance / power-iteration exits and the weighted-median paths of medium_edges at three
    workgroup shapes and two one-wave shapes, shuffled into one call: every output equals the SPEC."""
    from pyconsensus_amd.batched import consensus_ragged, ragged_round

    per, order = W.side_inputs()
    ref = W.side_spec(alg)
    rounds = [(per[k][bat][0][b], {name: v[b] for name, v in per[k][bat][1].items()}) for k, bat, b in order]
    pick = lambda name: [kw[name] for _, kw in rounds]
    host = _host(consensus_ragged([r for r, _ in rounds], pick("reputation"), pick("scaled"), pick("lo"), pick("hi"),
                                  filled=True, original=True, wide=True, **W.side_alg_kw(alg)))
    names = [k for k in host if not k.startswith("_")]
    assert set(PER_ROUND + ("filled", "original", "smooth_rep", "outcomes_final")) <= set(names) <= set(ref[0]["side"])
    for i, (k, bat, b) in enumerate(order):
        g = ragged_round(host, i)
        for name in names:
            assert_same_bits(g[name], ref[k][bat][name][b], (alg, i, W.SIDE_SHAPES[k], bat, b, name))


def test_wave_rounds_only_equal_the_narrow_call(gpu_lib):
    _, order = W.mix()
    order = [o for o in order if W.is_wave(*W.MIX_SHAPES[o[0]])]
    assert len(order) >= 30
    wide, narrow = _host(_run_mix(order, "PCA")), _host(_run_mix(order, "PCA", wide=False))
    for name in (k for k in narrow if not k.startswith("_")):
        assert_same_bits(wide[name], narrow[name], name)


def test_equal_shapes_equal_consensus_batched(gpu_lib):
    """64 rounds of 100 x 50 through the descriptor route equal consensus_batched on the same data."""
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched, consensus_ragged

    R, sc, lo, hi, rep = synthetic.rounds(64, 100, 50, seed=4)
    host = _host(consensus_ragged(list(R), list(rep), list(sc), list(lo), list(hi), filled=True, original=True,
                                  wide=True))
    own = consensus_batched(R, rep, sc, lo, hi, filled=True, original=True)
    for name in (k for k in host if not k.startswith("_")):
        assert_same_bits(host[name], own[name].cpu().numpy().reshape(-1), name)


@pytest.mark.parametrize("alg", ["PCA", "clusterfeck"])
def test_reversed_order_gives_reversed_outputs(gpu_lib, alg):
    from pyconsensus_amd.batched import ragged_round

    _, order = W.mix()
    order = order[:96]
    fwd, rev = _host(_run_mix(order, alg)), _host(_run_mix(order[::-1], alg))
    B = len(order)
    for b in range(B):
        f, r = ragged_round(fwd, b), ragged_round(rev, B - 1 - b)
        for name in f:
            assert_same_bits(f[name], r[name], (alg, b, name))


def test_refusals_launch_nothing(gpu_lib):
    """k-means, a 257 x 4 and a 4 x 65 round are refused with the round named, and nothing is
    launched (the outputs keep their bytes); an empty batch succeeds; a valid call afterwards works."""
    import torch

    from pyconsensus_amd import _abi, _device, _lib
    from pyconsensus_amd.batched import consensus_ragged

    ok = [np.full((3, 4), 1.0), np.full((70, 2), 2.0)]
    with pytest.raises(_lib.PcxError, match="k-means"):
        consensus_ragged(ok, algorithm="k-means", wide=True)
    with pytest.raises(_lib.PcxError, match="round 2 is 257 x 4"):
        consensus_ragged(ok + [np.ones((257, 4))], wide=True)
    with pytest.raises(_lib.PcxError, match="round 1 is 4 x 65"):
        consensus_ragged([ok[0], np.ones((4, 65)), ok[1]], wide=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    n, e = np.array([70, 257], dtype=np.int32), np.array([4, 4], dtype=np.int32)
    R = torch.ones(70 * 4 + 257 * 4, dtype=torch.float64, device=dev)
    sentinel = torch.full((70 + 257,), -7.0, dtype=torch.float64, device=dev)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    for alg, shapes_n in ((_abi.ALG_PCA, n), (_abi.ALG_KMEANS, np.array([70, 5], dtype=np.int32))):
        inp = _abi.Ragged(2, shapes_n.ctypes.data, e.ctypes.data, R.data_ptr(), None, None, None, None, 0, alg,
                          0.1, 0.1, 5, 0.9, None, 0.5, 0.0)
        res = _abi.BatchResult()
        res.smooth_rep = sentinel.data_ptr()
        assert gpu_lib.pcx_consensus_ragged_wide_f64(h, C.byref(inp), C.byref(res)) == _abi.EINVAL
    assert b"k-means" in gpu_lib.pcx_last_error()
    # a valid shape list with an option the shared checks refuse: nothing reaches the stream either
    ok_n = np.array([70, 5], dtype=np.int32)
    inp = _abi.Ragged(2, ok_n.ctypes.data, e.ctypes.data, None, None, None, None, None, 0, 0, 0.1, 0.1, 5, 0.9, None,
                      0.5, 0.0)
    res = _abi.BatchResult()
    res.smooth_rep = sentinel.data_ptr()
    assert gpu_lib.pcx_consensus_ragged_wide_f64(h, C.byref(inp), C.byref(res)) == _abi.EINVAL
    assert b"ragged: reports is NULL" in gpu_lib.pcx_last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == -7.0).all())
    inp = _abi.Ragged(0, None, None, None, None, None, None, None, 0, 0, 0.1, 0.1, 5, 0.9, None, 0.5, 0.0)
    assert gpu_lib.pcx_consensus_ragged_wide_f64(h, C.byref(inp), C.byref(_abi.BatchResult())) == 0
    empty = consensus_ragged([], wide=True)
    assert empty["smooth_rep"].numel() == 0 and empty["_cell_offsets"].tolist() == [0]
    out = _host(consensus_ragged(ok, wide=True))
    assert out["outcomes_final"].tolist() == [1.0] * 4 + [2.0] * 2


def test_back_to_back_calls(gpu_lib):
    """Three calls with different mixes and no synchronisation between them: after one sync each
    equals its own single call."""
    import torch

    _, order = W.mix()
    lists = [order[:80], order[60:130], order[100:]]
    outs = [_run_mix(o, "PCA") for o in lists]
    torch.cuda.synchronize()
    hosts = [_host(o) for o in outs]
    for h, o in zip(hosts, lists):
        single = _host(_run_mix(o, "PCA"))
        for name in (k for k in h if not k.startswith("_")):
            assert_same_bits(h[name], single[name], ("back-to-back", name))
        _check_against_spec(h, o, "PCA", "back-to-back")


# ---------------------------------------------------------------- consensus_many(wide=True)
def _same_layout(a, b, path):
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), (path, list(a), list(b))
        for k in a:
            _same_layout(a[k], b[k], path + (k,))
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_layout(x, y, path + (i,))
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype, (path, a.shape, b.shape, a.dtype, b.dtype)
        if isinstance(a, np.ma.MaskedArray):
            assert np.array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b)), path


def test_consensus_many_wide(gpu_lib):
    """The README's example, six goldens, a 70 x 5, a 100 x 50 and a 256 x 64 problem in one
    consensus_many(wide=True): keys and container types of Oracle(...).consensus(), the ragged path
    for all of them, values by the parity rules, the caller's matrices rescaled in place alike."""
    from pyconsensus_amd import Oracle, consensus_many
    from pyconsensus_amd import many as many_mod

    a, b = W.many_problems(), W.many_problems()
    paths = []
    finish = Oracle._finish

    def spy(self, *args, **kw):
        paths.append(self.last_info.get("path"))
        return finish(self, *args, **kw)

    Oracle._finish, saved = spy, finish
    try:
        got = consensus_many(a, wide=True)
    finally:
        Oracle._finish = saved
    assert many_mod.consensus_many is consensus_many and isinstance(got, list) and len(got) == len(b)
    assert paths == ["ragged"] * len(b), paths
    for i, p in enumerate(b):
        ref = Oracle(**p).consensus()
        _same_layout(got[i], ref, (i,))
        assert got[i]["convergence"] == ref["convergence"] and got[i]["components"] == ref["components"], i
        bad, _ = P.compare(G.flat_result(ref), W.abi_named(G.flat_result(got[i])))
        assert not bad, (i, np.asarray(p["reports"]).shape, bad)
        assert_same_bits(np.asarray(a[i]["reports"], dtype=np.float64), np.asarray(p["reports"], dtype=np.float64),
                         (i, "caller's matrix"))
