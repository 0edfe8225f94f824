"""k-means in ragged batches on the GPU: consensus_ragged(kmeans_init=...) through
pcx_consensus_ragged_kmeans_f64 on both round kernels, and consensus_many under k-means on top.  Every
comparison is on bits, NaN equal to NaN: against consensus_batched of each round's shape with the
round's own book, and against the C SPEC on the round alone.  test_kmeans_ragged_cpu.py asserts that a
round's result depends on its own book, so a wrong offset, a wrong k_b or another round's book fails
here."""
import copy
import ctypes as C

import numpy as np
import pytest

import golden_cases as G
import kmeans_cases as K
import parity as P
import ragged_wide_cases as W

pytestmark = pytest.mark.gpu


def _sync():
    import torch

    torch.cuda.synchronize()


def _ragged(kind, **kw):
    from pyconsensus_amd.batched import consensus_ragged, ragged_to_host

    R, rep, sc, lo, hi = K.round_inputs(kind)
    return ragged_to_host(consensus_ragged(R, rep, sc, lo, hi, wide=kind != "wave", filled=True, original=True, **kw))


_BATCHED = {}


def batched_ref(kind, restarts):
    """{round of batch(kind): consensus_batched's outputs of that round}, one call per shape with the
    rounds' own books (the rule's k); computed once."""
    from pyconsensus_amd.batched import consensus_batched

    if (kind, restarts) not in _BATCHED:
        ref = {}
        for shape, (idx, book3) in K.shape_batches(kind, K.books(kind, restarts)).items():
            R, rep, sc, lo, hi = K.shape_rounds(shape[0], shape[1], K.per_shape(shape), K.shape_seed(shape))
            o = consensus_batched(R, rep, sc, lo, hi, algorithm="k-means", kmeans_init=book3, filled=True, original=True)
            _sync()
            o = {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}
            for r, b in enumerate(idx):
                ref[b] = {k: v[r] for k, v in o.items()}
        _BATCHED[(kind, restarts)] = ref
    return _BATCHED[(kind, restarts)]


def assert_round(g, want, what):
    assert set(g) == set(want) and len(g) == 25, (what, sorted(set(g) ^ set(want)))
    for name in want:
        assert K.same_bits(np.asarray(g[name]), np.asarray(want[name])), (what, name)


def check_kind(kind, restarts):
    from pyconsensus_amd.batched import ragged_round

    the_books = K.books(kind, restarts)
    got = _ragged(kind, algorithm="k-means", kmeans_init=the_books)
    assert got["this_rep"].shape == (sum(s[0] for s, _ in K.batch(kind)),)
    ref = batched_ref(kind, restarts)
    for b, (shape, i) in enumerate(K.batch(kind)):
        assert_round(ragged_round(got, b), ref[b], (kind, restarts, b, shape))
    for shape, (idx, book3) in K.shape_batches(kind, the_books).items():  # and the SPEC, round by round
        spec = K.spec_shape(shape, book3)
        for r, b in enumerate(idx):
            g = ragged_round(got, b)
            for name in K.OUTPUTS_N + K.OUTPUTS_E + K.OUTPUTS_1:
                assert K.same_bits(np.asarray(g[name]), np.asarray(spec[name][r])), ("SPEC", kind, restarts, shape, name)
    return got


@pytest.mark.parametrize("restarts", K.RESTARTS)
def test_one_wave_rounds_equal_their_batched_runs_and_the_spec(gpu_lib, restarts):
    got = check_kind("wave", restarts)
    if restarts == 1:  # both ends of the clustering are reached: NaN rounds and finite ones
        assert np.isnan(got["this_rep"]).any() and np.isfinite(got["this_rep"]).any()


@pytest.mark.parametrize("restarts", K.RESTARTS)
def test_wide_rounds_equal_their_batched_runs_and_the_spec(gpu_lib, restarts):
    check_kind("wide", restarts)


SETS = [{}, {"algorithm": "hierarchical", "hierarchy_threshold": 0.7}, {"algorithm": "k-means"},
        {"algorithm": "clusterfeck"}, {"algorithm": "big-five", "max_components": 5},
        {"algorithm": "k-means", "alpha": 0.3}]


def test_rounds_under_their_own_sets_equal_the_shared_parameter_calls(gpu_lib):
    from pyconsensus_amd.batched import ragged_round

    rounds = K.batch("wide")
    the_books = K.books("wide", 3)
    per_round = [SETS[b % len(SETS)] for b in range(len(rounds))]
    init = [the_books[b] if per_round[b].get("algorithm") == "k-means" else None for b in range(len(rounds))]
    mixed = _ragged("wide", per_round=per_round, kmeans_init=init)
    assert mixed["_shapes"].shape == (len(rounds), 2)
    for q, kw in enumerate(SETS):
        want = _ragged("wide", kmeans_init=the_books, **kw) if kw.get("algorithm") == "k-means" else _ragged("wide", **kw)
        for b in range(q, len(rounds), len(SETS)):
            assert_round(ragged_round(mixed, b), ragged_round(want, b), (q, b, rounds[b]))
    # the two k-means sets differ where alpha enters
    assert not K.same_bits(_ragged("wide", kmeans_init=the_books, **SETS[2])["smooth_rep"],
                           _ragged("wide", kmeans_init=the_books, **SETS[5])["smooth_rep"])


def test_the_callers_code_book_sizes(gpu_lib):
    """k_b = 1, the kernel's bound min(N_b, 8) / min(N_b, 16), and k_b = N_b where N_b <= 8: each
    round equals consensus_batched(kmeans_init=...) of that k."""
    from pyconsensus_amd.batched import consensus_batched, ragged_round

    rounds = K.batch("wide")
    ks = []
    for b, ((N, E), _) in enumerate(rounds):
        bound = min(N, 8 if N <= 64 and E <= 32 else 16)
        ks.append(N if N <= 8 and b % 3 == 2 else (1, bound, max(1, bound // 2))[b % 3])
    assert 1 in ks and 8 in ks and 16 in ks and any(k == N for k, ((N, _), _) in zip(ks, rounds) if 1 < N <= 8)
    the_books = K.books("wide", 3, k=tuple(ks))
    got = _ragged("wide", algorithm="k-means", kmeans_init=the_books)
    also = _ragged("wide", algorithm="k-means", kmeans_init=the_books, kmeans_k=ks, kmeans_restarts=3)
    R, rep, sc, lo, hi = K.round_inputs("wide")
    for b in range(len(rounds)):
        o = consensus_batched(R[b][None], rep[b][None], sc[b][None], lo[b][None], hi[b][None], algorithm="k-means",
                              kmeans_init=the_books[b][None], filled=True, original=True)
        want = {k: v.cpu().numpy()[0] for k, v in o.items() if not k.startswith("_")}
        assert_round(ragged_round(got, b), want, (b, rounds[b], ks[b]))
        assert_round(ragged_round(also, b), want, (b, rounds[b], ks[b]))


def test_device_resident_books_on_a_side_stream_twice(gpu_lib):
    import torch

    from pyconsensus_amd.batched import consensus_ragged, ragged_plan, ragged_to_host

    the_books = K.books("wide", 3)
    want = _ragged("wide", algorithm="k-means", kmeans_init=the_books)
    R, rep, sc, lo, hi = K.round_inputs("wide")
    _, _, off = ragged_plan([r.shape for r in R], "k-means", wide=True, kmeans_restarts=3)
    flat = torch.from_numpy(np.concatenate([b.reshape(-1) for b in the_books])).cuda()
    assert flat.numel() == off[-1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = consensus_ragged(R, rep, sc, lo, hi, wide=True, filled=True, original=True, algorithm="k-means",
                             kmeans_init=flat, kmeans_restarts=3)
        b = consensus_ragged(R, rep, sc, lo, hi, wide=True, filled=True, original=True, algorithm="k-means",
                             kmeans_init=flat, kmeans_restarts=3)
    side.synchronize()
    assert a["_kmeans_init"] is flat and (a["_kmeans_offsets"] == off).all()
    ha, hb = ragged_to_host(a), ragged_to_host(b)
    for name in want:
        if not name.startswith("_"):
            assert K.same_bits(ha[name], want[name]) and K.same_bits(hb[name], want[name]), name
    with pytest.raises(ValueError, match="needs kmeans_restarts"):
        consensus_ragged(R, rep, sc, lo, hi, wide=True, algorithm="k-means", kmeans_init=flat)
    with pytest.raises(ValueError, match="holds %d rows" % (flat.numel() - 1)):
        consensus_ragged(R, rep, sc, lo, hi, wide=True, algorithm="k-means", kmeans_init=flat[:-1].contiguous(),
                         kmeans_restarts=3)


def test_refusals_launch_nothing(gpu_lib):
    """The C entry with NULL books, restarts < 1, a k_b past each bound and cokurtosis without scores:
    a sentinel output keeps its bytes, and a valid call afterwards works."""
    import torch

    from pyconsensus_amd import _abi, _device, _lib
    from pyconsensus_amd.batched import _params_array, param_sets

    shapes = [(10, 4), (100, 50), (5, 3)]
    mats = [K.shape_rounds(n, e, 1, 5)[0][0] for n, e in shapes]
    ns = np.array([s[0] for s in shapes], dtype=np.int32)
    es = np.array([s[1] for s in shapes], dtype=np.int32)
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).cuda()
    defaults = dict(algorithm="k-means", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
                    hierarchy_threshold=0.5, cluster_threshold=None)
    inp = _abi.Ragged(3, ns.ctypes.data, es.ctypes.data, flat.data_ptr(), None, None, None, None, 0, 0, 0.1, 0.1, 5, 0.9,
                      None, 0.5, 0.0)
    sentinel = torch.full((int(ns.sum()),), -7.25, dtype=torch.float64, device="cuda")
    res = _abi.BatchResult()
    res.smooth_rep = sentinel.data_ptr()
    books_host = [np.zeros((2, K.rule(n)), dtype=np.int32) + np.arange(K.rule(n), dtype=np.int32) for n in ns]
    init = torch.from_numpy(np.concatenate([b.reshape(-1) for b in books_host])).cuda()
    h = _lib.bind_stream(0, _device.current_stream_handle(torch.device("cuda", 0)))
    lib = _lib.lib()

    def call(per_round, books):
        sets, of = param_sets(per_round, defaults, "per_round")
        arr = _params_array(sets)
        rc = lib.pcx_consensus_ragged_kmeans_f64(h, C.byref(inp), len(sets), C.cast(arr, C.c_void_p), of.ctypes.data,
                                                 None if books is None else C.byref(books), C.byref(res))
        return rc, lib.pcx_last_error().decode()

    def k_array(*k):
        a = np.array(k, dtype=np.int32)
        return a, a.ctypes.data

    all_km = [{}] * 3
    refused = [(all_km, None, "books is NULL"),
               (all_km, _abi.KmeansBooks(0, None, init.data_ptr()), "restarts must be >= 1"),
               (all_km, _abi.KmeansBooks(2, None, None), "books->init is NULL"),
               ([{}, {}, {"algorithm": "cokurtosis"}], _abi.KmeansBooks(2, None, init.data_ptr()), "cokurtosis needs aux_scores")]
    for bad_k, words in (((0, 10, 3), "round 0"), ((9, 10, 3), r"round 0"), ((4, 17, 3), "round 1"),
                         ((4, 10, 6), "round 2")):
        keep, ptr = k_array(*bad_k)
        refused.append((all_km, _abi.KmeansBooks(2, ptr, init.data_ptr()), words))
        refused[-1] += (keep,)
    for case in refused:
        rc, msg = call(case[0], case[1])
        assert rc == -1 and case[2] in msg, (case[2], rc, msg)
    _sync()
    assert (sentinel.cpu().numpy() == -7.25).all()
    rc, msg = call(all_km, _abi.KmeansBooks(2, None, init.data_ptr()))
    assert rc == 0, msg
    _sync()
    got = sentinel.cpu().numpy()
    assert (got != -7.25).all()  # (a NaN round counts: it was written)
    # the Python layer: the old path still raises without the keyword, the new one checks its books
    from pyconsensus_amd.batched import consensus_ragged

    with pytest.raises(_lib.PcxError, match="k-means is not supported"):
        consensus_ragged(mats, algorithm="k-means", wide=True)
    with pytest.raises(ValueError, match=r"kmeans_init\[1\] rows must lie in \[0, 100\)"):
        consensus_ragged(mats, algorithm="k-means", wide=True,
                         kmeans_init=[books_host[0], books_host[1] + 95, books_host[2]])
    with pytest.raises(_lib.PcxError, match="round 1 is 100 x 50"):
        consensus_ragged(mats, algorithm="k-means", kmeans_init="draw")


# ---------------------------------------------------------------- consensus_many
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
        assert K.same_bits(np.ma.getdata(a), np.ma.getdata(b)), path
    elif isinstance(a, np.ndarray):
        assert K.same_bits(a, b), path
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def _many_problems():
    """ragged_wide_cases' problems with the 70 x 5 one (too large for the one-wave batch) moved into
    the middle of the list."""
    ps = W.many_problems()
    ps.insert(3, ps.pop(len(ps) - len(W.MANY_WIDE)))
    assert np.asarray(ps[3]["reports"]).shape == (70, 5)
    return ps


def test_consensus_many_under_kmeans_equals_the_oracle_loop_and_leaves_its_state(gpu_lib):
    from pyconsensus_amd import Oracle, consensus_many

    a, b = _many_problems()[:-2], _many_problems()[:-2]  # (the two largest: the wide test below)
    np.random.seed(20261020)
    many = consensus_many(a, algorithm="k-means")
    state = np.random.get_state()
    np.random.seed(20261020)
    oracles = [Oracle(**p, algorithm="k-means") for p in b]
    loop = [o.consensus() for o in oracles]
    after = np.random.get_state()
    assert state[0] == after[0] and (state[1] == after[1]).all() and state[2:] == after[2:]
    assert len(many) == len(loop) == len(W.many_problems()) - 2
    for i in range(len(loop)):
        _same_value(many[i], loop[i], (i,))


def test_consensus_many_wide_under_kmeans(gpu_lib):
    from pyconsensus_amd import Oracle, consensus_many

    a, b = _many_problems(), _many_problems()
    paths = []
    finish = Oracle._finish

    def spy(self, *args, **kw):
        paths.append(self.last_info.get("path"))
        return finish(self, *args, **kw)

    np.random.seed(77)
    Oracle._finish, saved = spy, finish
    try:
        got = consensus_many(a, wide=True, algorithm="k-means")
    finally:
        Oracle._finish = saved
    state = np.random.get_state()
    assert paths == ["ragged"] * len(b), paths
    np.random.seed(77)
    for i, p in enumerate(b):
        ref = Oracle(**p, algorithm="k-means").consensus()
        assert got[i]["convergence"] == ref["convergence"] and got[i]["components"] == ref["components"], i
        bad, _ = P.compare(G.flat_result(ref), W.abi_named(G.flat_result(got[i])))
        assert not bad, (i, np.asarray(p["reports"]).shape, bad)
    after = np.random.get_state()
    assert (state[1] == after[1]).all() and state[2] == after[2]
