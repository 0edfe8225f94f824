"""The four ragged entries back to back on one context and one stream (pcx_ragged.cpp): they share
the context's two staging slots, so a call's tables must stay intact until its launches have read
them whichever entry comes next -- the slots taken in turn, a slot grown under a later call, the
event waits across entry kinds.  Six calls with no synchronise between them; each call's outputs,
`filled` included, equal bit for bit the same call made alone on a fresh context."""
import threading

import numpy as np
import pytest

import kmeans_cases as K

pytestmark = pytest.mark.gpu

# small rounds that reach the one-wave kernel, the workgroup kernel's launch classes 2 and 3 (class 1
# too under big-five) and, under hierarchical or k-means, the clustering launches of both
SHAPES = [(1, 1), (5, 3), (64, 32), (65, 3), (256, 64), (100, 50)]
WAVE = [b for b, (n, e) in enumerate(SHAPES) if n <= 64 and e <= 32]
KMEANS_ROUNDS = (1, 3, 5)  # one-wave, and workgroup rounds of two launch classes
RESTARTS = 2
PAD_SETS = 100  # 48 bytes each: past the staging slot's first 4 KiB


def _inputs():
    out = [[] for _ in range(5)]
    for N, E in SHAPES:
        for lst, a in zip(out, K.shape_rounds(N, E, 1, K.shape_seed((N, E)))):
            lst.append(a[0])
    return out


def _fresh_context():
    """Destroy this thread's context of the current device: the next call creates one."""
    import torch

    from pyconsensus_amd import _lib

    torch.cuda.synchronize()
    h = _lib._ctx.pop((threading.get_ident(), torch.cuda.current_device()), None)
    if h is not None:
        _lib.lib().pcx_destroy(h)


def _calls(algorithm, monkeypatch):
    """The six calls as thunks returning consensus_ragged's device outputs."""
    from pyconsensus_amd import batched

    R, rep, sc, lo, hi = _inputs()
    pick = lambda seq, idx: [seq[b] for b in idx]
    kw = dict(algorithm=algorithm, filled=True, original=True, hierarchy_threshold=0.7)
    two_sets = [{"alpha": 0.3} if b % 2 else {} for b in range(len(SHAPES))]
    with_kmeans = [{"algorithm": "k-means"} if b in KMEANS_ROUNDS else {} for b in range(len(SHAPES))]
    drawn = batched.kmeans_draws_ragged([SHAPES[b][0] for b in KMEANS_ROUNDS], RESTARTS, np.random.RandomState(20261020))
    init = [None] * len(SHAPES)
    for b, book in zip(KMEANS_ROUNDS, drawn):
        init[b] = book
    real_sets = batched.param_sets

    def many_sets(entries, defaults, what):  # the same rounds on the same sets, and sets that no round takes
        sets, of = real_sets(entries, defaults, what)
        return sets + [dict(defaults, alpha=0.5 + 0.001 * i) for i in range(PAD_SETS)], of

    def grown():
        monkeypatch.setattr(batched, "param_sets", many_sets)
        try:
            return batched.consensus_ragged(R, rep, sc, lo, hi, wide=True, per_round=two_sets, **kw)
        finally:
            monkeypatch.setattr(batched, "param_sets", real_sets)

    wide = lambda: batched.consensus_ragged(R, rep, sc, lo, hi, wide=True, **kw)
    return [
        ("wide", wide),
        ("narrow", lambda: batched.consensus_ragged(*(pick(x, WAVE) for x in (R, rep, sc, lo, hi)), **kw)),
        ("params", lambda: batched.consensus_ragged(R, rep, sc, lo, hi, wide=True, per_round=two_sets, **kw)),
        ("k-means", lambda: batched.consensus_ragged(R, rep, sc, lo, hi, wide=True, per_round=with_kmeans,
                                                     kmeans_init=init, **kw)),
        ("params, more sets", grown),
        ("wide again", wide),
    ]


# (big-five: the three workgroup rounds then fall into launch classes 1, 2 and 3, so every class runs,
# in the shared walk and in the table walk's plain segments)
@pytest.mark.parametrize("algorithm", ["PCA", "hierarchical", "big-five"])
def test_six_calls_in_a_row_equal_each_call_alone(gpu_lib, algorithm, monkeypatch):
    import torch

    from pyconsensus_amd.batched import ragged_to_host

    calls = _calls(algorithm, monkeypatch)
    _fresh_context()
    outs = [call() for _, call in calls]  # no synchronise between the calls
    torch.cuda.synchronize()
    got = [ragged_to_host(o) for o in outs]
    assert len(outs[4]["_param_sets"]) == 2 + PAD_SETS and len(outs[2]["_param_sets"]) == 2
    for (what, call), g in zip(calls, got):
        _fresh_context()
        want = ragged_to_host(call())
        names = [k for k in want if not k.startswith("_")]
        assert len(names) == 25 and "filled" in names and sorted(names) == sorted(k for k in g if not k.startswith("_"))
        for name in names:
            assert K.same_bits(np.asarray(g[name]), np.asarray(want[name])), (algorithm, what, name)
    _fresh_context()
    # the calls differ where they should: the second set's alpha and the k-means rounds show
    assert not K.same_bits(got[0]["smooth_rep"], got[2]["smooth_rep"])
    assert not K.same_bits(got[2]["this_rep"], got[3]["this_rep"])
    assert K.same_bits(got[0]["this_rep"], got[5]["this_rep"]) and K.same_bits(got[2]["filled"], got[4]["filled"])
